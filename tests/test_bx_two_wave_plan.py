"""The plan arithmetic of the two-wave box build (CPU, no GPU): the host-side LDS
layout of csrc/psn_lk_kernels.h with quarter-wave fallback tiles, and the
workgroups per CU that LDS and registers allow -- six, against four of the
4-unit four-wave build. The register side is read from the built library's code
objects (tools/kernel_resources.py)."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
LIB = os.path.join(ROOT, "mcmtt_opticalflow_amd", "lib", "libpsn_lk.so")
CU_LDS = 160 * 1024
SIMD_VGPRS, VGPR_GRANULE, SIMDS = 512, 8, 4

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="hipcc absent")

# the windows of tests/test_lk_bx_two_wave_gpu.py, then windows the build must not take
FITS = [(64, 64), (32, 128), (72, 56), (40, 50), (40, 32), (16, 72)]
NOT = [(64, 160), (128, 128), (8, 512), (72, 64)]

PROGRAM = r"""
#include <cstdio>
#include "psn_lk_kernels.h"
using namespace psn;
int main() {
    const int wins[][2] = {%s};
    std::printf("{\"target6\": %%d, \"occ2\": %%d, \"waves2\": %%d, \"occ4\": %%d, \"scr\": %%d, \"pc16\": %%d, \"pc32\": %%d, \"wins\": [",
                kBxLdsTarget6, bx_occupancy(kBxUPT2, true, kBxNT2), bx_waves_per_simd(kBxUPT2, true, kBxNT2),
                bx_occupancy(4, true), align16(kBxScrBytes), bx_pc(kBxUPT2, kBxTile2), bx_pc(kBxUPT2, kBxTile));
    bool first = true;
    for (auto &wh : wins) {
        const int w = wh[0], h = wh[1];
        const BxLayout q(w, h, kBxUPT2, 1, kBxTile2), q2(w, h, kBxUPT2, 2, kBxTile2), hw(w, h, kBxUPT2, 1, kBxTile),
            t24(w, h, kBxUPT2, 1, 24), four(w, h, 4);
        std::printf("%%s{\"w\": %%d, \"h\": %%d, \"fits\": %%d, \"jr\": %%d, \"un\": %%d, \"pb\": %%d, \"total\": %%d, "
                    "\"total_hw2\": %%d, \"total32\": %%d, \"total24\": %%d, \"total_four\": %%d, \"tre\": %%d}",
                    first ? "" : ", ", w, h, (int)bx_two_wave_fits(w, h, true), q.jr, q.un, q.pb, q.total, q2.total,
                    hw.total, t24.total, four.total, bx_err_rows(w, h, q.pb));
        first = false;
    }
    std::printf("]}\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("bxplan")
    src, exe = d / "plan.hip", d / "plan"
    src.write_text(PROGRAM % ", ".join("{%d, %d}" % wh for wh in FITS + NOT))
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mcmtt_opticalflow_amd", "csrc"),
                        str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    p = json.loads(out.stdout)
    p["by_win"] = {(e["w"], e["h"]): e for e in p["wins"]}
    return p


def test_headline_window_layout(plan):
    """64 x 64: records 4,160 + J region 6,144 + planes 24 x (64*8 + 96) = 14,592
    + slack 1,024 = 25,920 B; half-wave tiles would need 38,208 B (four per CU),
    24-thread tiles 32,064 B (five per CU)."""
    e = plan["by_win"][(64, 64)]
    assert plan["scr"] == 4160 and e["jr"] == 4160
    assert e["un"] - e["jr"] == 6144
    assert plan["pc16"] == 64 * 8 + 96 and e["pb"] == 24 * plan["pc16"] == 14592
    assert e["total"] == 4160 + 6144 + 14592 + 1024 == 25920
    assert e["total32"] == 38208 and CU_LDS // e["total32"] == 4
    assert e["total24"] == 32064 and CU_LDS // e["total24"] == 5
    assert plan["target6"] == CU_LDS // 6 == 27306
    # a second quarter-wave tile per fallback step would leave the six-per-CU target
    assert e["total_hw2"] > plan["target6"]


@pytest.mark.parametrize("win", FITS)
def test_six_workgroups_per_cu(plan, win):
    """LDS and registers both allow six two-wave workgroups per CU."""
    e = plan["by_win"][win]
    assert e["fits"] == 1
    assert e["total"] <= plan["target6"]
    by_lds = CU_LDS // e["total"]
    vgprs = SIMD_VGPRS // plan["waves2"] // VGPR_GRANULE * VGPR_GRANULE  # per lane at the build's waves per SIMD
    assert plan["waves2"] == 3 and vgprs == 168
    by_regs = plan["waves2"] * SIMDS // 2  # two waves per workgroup
    assert by_regs == plan["occ2"] == 6
    assert min(by_lds, by_regs) == 6
    assert plan["occ4"] == 4
    # the err fallback's row tiles fit the plane region
    assert 1 <= e["tre"] <= win[1] and 4 * ((e["tre"] * win[0] + 3) & ~3) <= e["pb"]


@pytest.mark.parametrize("win", NOT)
def test_windows_the_two_wave_build_leaves(plan, win):
    """More than 1,024 units, or an LDS plan above the six-per-CU target."""
    e = plan["by_win"][win]
    assert e["fits"] == 0
    units = win[1] * ((win[0] + 3) // 4)
    assert units > 1024 or e["total"] > plan["target6"]


def test_built_kernel_registers():
    """The built library: the two-wave build within 168 VGPRs without spills or
    scratch, every other no-tail box build at its registers (four, three and
    three workgroups per CU)."""
    assert os.path.exists(LIB), "build() first: " + LIB
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    ks = {n: r for n, r in kernel_resources.kernels(LIB).items() if "lk_kernel_bx" in n}
    two = [r for n, r in ks.items() if "ILi8ELb1ELi128E" in n]
    assert len(two) == 1, sorted(ks)
    assert int(two[0]["vgpr"]) <= 168 and int(two[0]["vgpr_spill"]) == 0 and int(two[0]["scratch"]) == 0, two
    for upt, vgpr in ((4, 122), (8, 152), (10, 167)):
        r = [r for n, r in ks.items() if f"ILi{upt}ELb1ELi256E" in n]
        assert len(r) == 1, sorted(ks)
        assert int(r[0]["vgpr"]) == vgpr and int(r[0]["vgpr_spill"]) == 0 and int(r[0]["scratch"]) == 0, (upt, r)


def test_instantiation_lists_match_built_kernels():
    """Each family's instantiation list, in the unit that owns the family, against the
    built library's code objects: exactly 17 lk_kernel_st and 11 lk_kernel_bx kernels,
    and every list entry among them (a variant cannot launch without its instantiation,
    also with the lists in separate files)."""
    assert os.path.exists(LIB), "build() first: " + LIB
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    csrc = os.path.join(ROOT, "mcmtt_opticalflow_amd", "csrc")
    hdr = open(os.path.join(csrc, "psn_lk_kernels.h")).read()
    const = {k: int(v) for k, v in re.findall(r"\b(kBx(?:NT2?|UPT2)) = (\d+)[,;]", hdr)}

    def entries(unit, macro):
        src = open(os.path.join(csrc, unit)).read()
        body = re.search(r"#define " + macro + r"\(X\)((?:.*\\\n)*.*)\n", src).group(1)
        return [[a.strip() for a in e.split(",")] for e in re.findall(r"X\(([^)]*)\)", body)]

    def num(a):
        return const[a] if a in const else int(a)

    st = ["lk_kernel_stILi%dELi%dELi%dELi%dE" % tuple(num(a) for a in e) for e in entries("psn_lk_st.hip", "PSN_ST_KERNELS")]
    bx = ["lk_kernel_bxILi%dELb%dELi%dE" % (num(u), nt == "true", num(n)) for u, nt, n in entries("psn_lk_bx.hip", "PSN_BX_KERNELS")]
    assert len(st) == len(set(st)) == 17 and len(bx) == len(set(bx)) == 11, (st, bx)
    built = list(kernel_resources.kernels(LIB))
    for family, want in (("lk_kernel_st", st), ("lk_kernel_bx", bx)):
        have = [n for n in built if family + "I" in n]
        assert len(have) == len(want), (family, sorted(have))
        for key in want:
            assert sum(key in n for n in have) == 1, (key, sorted(have))


def test_box_kernel_names_agree():
    """One spelling of every box build: the launch tag's name (_lib.kernel_of_tag,
    which bench.py looks up in the round profile), the code objects' (tools/
    kernel_resources.py) and the profiler's demangled one as tools/pmc_summary.py
    and tools/profile_summary.py key it -- the builds of 256 threads without the
    default workgroup size, the two-wave build with its 128."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
        import pmc_summary
    finally:
        sys.path.pop(0)
    from mcmtt_opticalflow_amd import _lib

    for tag, traced, mangled in [
        (41, "void psn::lk_kernel_bx<4, true, 256>(psn::LkLaunchArgs)", "_ZN3psn12lk_kernel_bxILi4ELb1ELi256EEEvNS_12LkLaunchArgsE"),
        (100, "void psn::lk_kernel_bx<10, false, 256>(psn::LkLaunchArgs)", "_ZN3psn12lk_kernel_bxILi10ELb0ELi256EEEvNS_12LkLaunchArgsE"),
        (101, "void psn::lk_kernel_bx<10, true, 256>(psn::LkLaunchArgs)", "_ZN3psn12lk_kernel_bxILi10ELb1ELi256EEEvNS_12LkLaunchArgsE"),
        (82, "void psn::lk_kernel_bx<8, true, 128>(psn::LkLaunchArgs)", "_ZN3psn12lk_kernel_bxILi8ELb1ELi128EEEvNS_12LkLaunchArgsE"),
    ]:
        name = _lib.kernel_of_tag(tag)
        assert pmc_summary.short(traced) == name, (traced, name)
        assert kernel_resources.pretty(mangled) == name, (mangled, name)
    assert _lib.kernel_of_tag(82) == "lk_kernel_bx<8, true, 128>" and _lib.kernel_of_tag(81) == "lk_kernel_bx<8, true>"
    # the names of a trace taken before the workgroup size was a parameter stay as they are
    assert pmc_summary.short("void psn::lk_kernel_bx<4, true>(psn::LkLaunchArgs)") == "lk_kernel_bx<4, true>"
