"""The forward entry of the box kernel (lk_kernel_fw<10, true>, csrc/psn_lk_bx.hip)
on the CPU: the built library's code objects, and what the launch planner
(csrc/psn_lk_plan.cpp, linked alone into a small program) gives which window.

The entry shares lk_kernel_bx<10, true>'s body, launch bounds and LDS plan; the
planner picks it per launch, so a call's queries, launch groups, key and kernel
tag (psn_lk_timing_launches) are those of lk_kernel_bx<10, true> and only the
launch's `fw` and the call's entry tag (psn_lk_timing_entries) tell the two apart.
"""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "mcmtt_opticalflow_amd", "csrc")
LIB = os.path.join(ROOT, "mcmtt_opticalflow_amd", "lib", "libpsn_lk.so")
ACCUM_SCALAR = 0x100

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="hipcc absent")

# no-tail windows (SSE2 order, w % 8 == 0) of 2,049 - 2,560 units of 4 px: the forward entry's
# (the first four are the windows of tests/test_lk_fw_gpu.py)
INSIDE = [(64, 132), (40, 232), (72, 136), (64, 160), (40, 205), (40, 256), (64, 129), (56, 152), (64, 136)]
# no-tail windows outside the range: 2,048 units and fewer (8 per thread), 2,561 and more (12)
OUTSIDE = [(64, 128), (32, 256), (56, 183), (64, 161), (72, 160), (64, 64), (64, 100), (64, 200), (128, 128)]
# a scalar tail (w % 8 != 0) inside the unit range: lk_kernel_bx<10, false>
TAIL = [(60, 160), (44, 200), (68, 140)]

PROGRAM = r"""
#include <cstdio>
#include "psn_lk_plan.h"
using namespace psn;
static bool first = true;
static void plan(const char *set, int w, int h, int flags, int fw) {
    PlanCfg g;
    g.width = 1920, g.height = 1080, g.nlevels = 4, g.user_slots = 4, g.nslots = 6;
    g.fw = fw;
    psn_lk_query q{};
    q.prev_slot = 0, q.next_slot = 1, q.num_pts = 100;
    q.params.win_w = w, q.params.win_h = h, q.params.max_level = 3;
    q.params.term_type = PSN_LK_TERM_COUNT | PSN_LK_TERM_EPS, q.params.max_count = 30, q.params.epsilon = 0.01;
    q.params.flags = flags, q.params.min_eig_threshold = 1e-4;
    const char filled[6] = {1, 1, 1, 1, 1, 1};
    LkCallPlan p;
    std::string err;
    const int rc = plan_call(g, &q, 1, filled, false, false, 1, p, err);
    const int n = (int)p.launches.size();
    const LkLaunchPlan z{}, &L = n ? p.launches[0] : z;
    std::printf("%s{\"set\": \"%s\", \"w\": %d, \"h\": %d, \"flags\": %d, \"knob\": %d, \"rc\": %d, \"launches\": %d, "
                "\"bx\": %d, \"key\": %d, \"upt\": %d, \"notail\": %d, \"nt\": %d, \"fw\": %d, \"lds\": %d, \"tag\": %d, "
                "\"entry\": %d}",
                first ? "" : ", ", set, w, h, flags, fw, rc, n, (int)(L.cls == kClsBx), L.key, L.upt, (int)L.notail, L.nt,
                (int)L.fw, L.lds, p.tag, p.entry);
    first = false;
}
int main() {
    const int inside[][2] = {@INSIDE@}, outside[][2] = {@OUTSIDE@}, tail[][2] = {@TAIL@};
    std::printf("{\"target\": %d, \"fw_upt\": %d, \"fits_10\": %d, \"fits_8\": %d, \"fits_tail\": %d, \"fits_two_wave\": %d, \"plans\": [",
                kBxLdsTarget, kBxFwUPT, (int)bx_fw_fits(10, true, kBxNT), (int)bx_fw_fits(8, true, kBxNT),
                (int)bx_fw_fits(10, false, kBxNT), (int)bx_fw_fits(kBxUPT2, true, kBxNT2));
    for (int fw = 0; fw <= 2; fw++) {
        for (auto &w : inside) plan("inside", w[0], w[1], 0, fw);
        for (auto &w : inside) plan("scalar", w[0], w[1], PSN_LK_ACCUM_SCALAR, fw);
        for (auto &w : outside) plan("outside", w[0], w[1], 0, fw);
        for (auto &w : tail) plan("tail", w[0], w[1], 0, fw);
    }
    std::printf("]}\n");
    return 0;
}
"""


def _kernel_resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    return kernel_resources


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    d = tmp_path_factory.mktemp("fwplan")
    src, exe = d / "plan.hip", d / "plan"
    fmt = lambda wins: ", ".join("{%d, %d}" % wh for wh in wins)  # noqa: E731
    src.write_text(PROGRAM.replace("@INSIDE@", fmt(INSIDE)).replace("@OUTSIDE@", fmt(OUTSIDE)).replace("@TAIL@", fmt(TAIL)))
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, str(src), os.path.join(CSRC, "psn_lk_plan.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    p = json.loads(out.stdout)
    assert all(e["rc"] == 0 and e["launches"] == 1 and e["bx"] == 1 for e in p["plans"]), p["plans"]
    return p


def _units(w, h):
    return h * ((w + 3) // 4)


def _of(plans, kind, knob):
    got = [e for e in plans["plans"] if e["set"] == kind and e["knob"] == knob]
    assert got
    return got


def test_windows_are_what_they_claim():
    for w, h in INSIDE:
        assert w % 8 == 0 and 2049 <= _units(w, h) <= 2560, (w, h)
    for w, h in OUTSIDE:
        assert w % 8 == 0 and not 2049 <= _units(w, h) <= 2560, (w, h)
    for w, h in TAIL:
        assert w % 8 != 0 and 2049 <= _units(w, h) <= 2560, (w, h)
    units = sorted(_units(w, h) for w, h in INSIDE + OUTSIDE)
    # both edges (w % 8 == 0: an even number of units per row, so of the window)
    assert {2048, 2050, 2560, 2562} <= set(units), units


def test_built_library_holds_the_forward_entry():
    """Exactly the kernels of PSN_FW_KERNELS under the name lk_kernel_fw, outside the
    lk_kernel_bx family, within three workgroups per CU: <= 168 VGPRs, no spill, no scratch."""
    assert os.path.exists(LIB), "build() first: " + LIB
    kr = _kernel_resources()
    src = open(os.path.join(CSRC, "psn_lk_bx.hip")).read()
    hdr = open(os.path.join(CSRC, "psn_lk_kernels.h")).read()
    const = {k: int(v) for k, v in re.findall(r"\b(kBx(?:NT2?|UPT2|FwUPT)) = (\d+)[,;]", hdr)}
    body = re.search(r"#define PSN_FW_KERNELS\(X\)(.*)\n", src).group(1)
    want = ["lk_kernel_fwILi%dELb%dELi%dE" % (const.get(u) or int(u), nt == "true", const.get(n) or int(n))
            for u, nt, n in re.findall(r"X\((\w+), (true|false), (\w+)\)", body)]
    assert want == ["lk_kernel_fwILi10ELb1ELi256E"], want
    built = kr.kernels(LIB)
    have = {n: r for n, r in built.items() if "lk_kernel_fw" in n}
    assert len(have) == len(want) and all(sum(k in n for n in have) == 1 for k in want), sorted(have)
    assert not any("lk_kernel_bx" in n for n in have)
    for n, r in have.items():
        print(kr.pretty(n), r)
        assert int(r["vgpr"]) <= 168 and int(r["vgpr_spill"]) == 0 and int(r["scratch"]) == 0, (n, r)
        assert kr.pretty(n) == "lk_kernel_fw<10, true>"


def test_names_agree():
    """The entry tag's name (_lib.kernel_of_tag), the code object's and the profiler's."""
    kr = _kernel_resources()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import pmc_summary
    finally:
        sys.path.pop(0)
    from mcmtt_opticalflow_amd import _lib

    assert _lib.kernel_of_tag(103) == "lk_kernel_fw<10, true>" and _lib.kernel_of_tag(1103) == "mixed:lk_kernel_fw<10, true>"
    assert kr.pretty("_ZN3psn12lk_kernel_fwILi10ELb1ELi256EEEvNS_12LkLaunchArgsE") == "lk_kernel_fw<10, true>"
    assert pmc_summary.short("void psn::lk_kernel_fw<10, true, 256>(psn::LkLaunchArgs)") == "lk_kernel_fw<10, true>"
    assert _lib.kernel_of_tag(101) == "lk_kernel_bx<10, true>"
    assert _lib.VARIANTS["fw"] == 13
    hdr = open(os.path.join(ROOT, "include", "psn_lk.h")).read()
    assert re.search(r"#define PSN_LK_VARIANT_FW 13\b", hdr)


def test_fits_is_the_ten_unit_no_tail_build(plans):
    assert plans["fw_upt"] == 10
    assert (plans["fits_10"], plans["fits_8"], plans["fits_tail"], plans["fits_two_wave"]) == (1, 0, 0, 0)


@pytest.mark.parametrize("knob", [0, 2])
def test_planner_gives_the_entry_to_its_windows(plans, knob):
    """By default (0) and when forced (2): every no-tail window of 2,049 - 2,560 units,
    as the launch lk_kernel_bx<10, true> would get."""
    never = {(e["w"], e["h"]): e for e in _of(plans, "inside", 1)}
    for e in _of(plans, "inside", knob):
        assert (e["upt"], e["notail"], e["nt"], e["fw"]) == (10, 1, 256, 1), e
        assert (e["key"], e["tag"], e["entry"]) == (101, 101, 103), e
        assert e["lds"] == never[e["w"], e["h"]]["lds"] <= plans["target"] == 53 * 1024, e


def test_variant_one_gives_the_box_kernel(plans):
    for e in _of(plans, "inside", 1):
        assert (e["upt"], e["notail"], e["nt"], e["fw"]) == (10, 1, 256, 0), e
        assert (e["key"], e["tag"], e["entry"]) == (101, 101, 101), e


@pytest.mark.parametrize("knob", [0, 1, 2])
@pytest.mark.parametrize("kind", ["outside", "tail", "scalar"])
def test_other_windows_never_get_the_entry(plans, kind, knob):
    """Windows outside the unit range, windows with a scalar tail and scalar-order
    queries, under every value of the variant."""
    for e in _of(plans, kind, knob):
        assert e["fw"] == 0 and e["entry"] == e["tag"] == e["key"] and e["key"] % 10 != 3, e
        if kind != "outside":
            assert (e["upt"], e["notail"]) == (10, 0), e  # the scalar-tail build of the same size
        else:
            assert e["upt"] != 10, e
