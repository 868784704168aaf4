"""The gate of the two-wave box build's sliding A pass (CPU, no GPU). The pass
carries a unit's right-hand columns to the unit on its right (bx_unit_slide,
csrc/psn_lk_bx.h), so it is taken only where every thread's run of kBxUPT2 units
is adjacent quads of ONE window row: psn::bx_slides (csrc/psn_lk_kernels.h).
Thread t's run starts at unit t * kBxUPT2 of the row-major units (QW = w / 4 a
row), so that is QW % kBxUPT2 == 0, and a run is then also wholly inside or
wholly past the window's U = h * QW units: the pass treats a thread's units
alike. Checked here by listing every run's cells for every no-tail window the
build can hold; the header's own predicate is compiled and compared. The
register side of the build is read from the built library."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmtt_opticalflow_amd", "csrc")
KERNELS_H = os.path.join(CSRC, "psn_lk_kernels.h")
LIB = os.path.join(ROOT, "mcmtt_opticalflow_amd", "lib", "libpsn_lk.so")
HIPCC = "/opt/rocm/bin/hipcc"


def _const(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, open(KERNELS_H).read()).group(1))


NT2, UPT2 = _const("kBxNT2"), _const("kBxUPT2")
MAX_UNITS = NT2 * UPT2
# every no-tail window (SSE2 order, w % 8 == 0) of at most NT2 * UPT2 units
WINDOWS = [(w, h) for w in range(8, 4 * MAX_UNITS + 1, 8) for h in range(1, MAX_UNITS // (w // 4) + 1)]


def _runs(w):
    """(row, quad) of every thread's run: arrays [NT2, UPT2]."""
    qw = w // 4
    u = np.arange(MAX_UNITS).reshape(NT2, UPT2)
    return u // qw, u % qw


def _whole_runs(w, h):
    """Every thread's run is wholly inside or wholly past the window's units."""
    inside = np.arange(MAX_UNITS).reshape(NT2, UPT2) < h * (w // 4)
    return bool((inside.all(1) | ~inside.any(1)).all())


def test_constants():
    assert (NT2, UPT2) == (128, 8)
    assert len(WINDOWS) > 3000 and (64, 64) in WINDOWS and (40, 40) in WINDOWS and (64, 72) not in WINDOWS
    assert all(h * (w // 4) <= 1024 for w, h in WINDOWS)


def test_no_run_wraps_a_row_iff_the_gate():
    """Both directions, per window width: the runs of all NT2 threads stay in one
    row with adjacent quads iff QW % UPT2 == 0."""
    for w in sorted({w for w, _ in WINDOWS}):
        row, quad = _runs(w)
        one_row = bool((row == row[:, :1]).all())
        adjacent = bool((quad == quad[:, :1] + np.arange(UPT2)).all())
        assert one_row == adjacent, w
        assert one_row == ((w // 4) % UPT2 == 0), w


def test_a_gated_run_is_inside_or_past_the_window():
    gated = [(w, h) for w, h in WINDOWS if (w // 4) % UPT2 == 0]
    assert (64, 64) in gated and (32, 32) in gated and (32, 8) in gated and (64, 8) in gated
    for w, h in gated:
        assert _whole_runs(w, h), (w, h)
        # ... and the run of a thread past the window reads inside the patch's first
        # rows: quads 0 .. UPT2 - 1 of row 0, dwords up to UPT2 + 1 < QW + 2
        assert UPT2 + 1 < w // 4 + 2
    # without the gate a run can be partly inside
    assert not _whole_runs(40, 25)  # U = 250


PROGRAM = r"""
#include <cstdio>
#include "psn_lk_kernels.h"
using namespace psn;
int main() {
    std::printf("{\"slides\": [");
    for (int w = 8; w <= 4 * kBxNT2 * kBxUPT2; w += 8) std::printf("%s%d", w > 8 ? ", " : "", (int)bx_slides(w, kBxNT2));
    std::printf("], \"four_wave\": [");
    for (int w = 8; w <= 4 * kBxNT2 * kBxUPT2; w += 8) std::printf("%s%d", w > 8 ? ", " : "", (int)bx_slides(w, kBxNT));
    std::printf("], \"lds64\": %d}\n", BxLayout(64, 64, kBxUPT2, 1, kBxTile2).total);
    return 0;
}
"""


@pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="hipcc absent")
def test_header_predicate(tmp_path):
    """psn::bx_slides is that gate for the two-wave build and false for the
    256-thread builds; the LDS plan of the headline window is what it was."""
    src, exe = tmp_path / "gate.hip", tmp_path / "gate"
    src.write_text(PROGRAM)
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    p = json.loads(out.stdout)
    widths = list(range(8, 4 * MAX_UNITS + 1, 8))
    assert p["slides"] == [int((w // 4) % UPT2 == 0) for w in widths]
    assert not any(p["four_wave"])
    assert p["lds64"] == 25920


def test_two_wave_build_resources():
    """With the sliding pass: at most 168 VGPRs (three waves per SIMD), no spill,
    no scratch."""
    assert os.path.exists(LIB), "build() first: " + LIB
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    two = [r for n, r in kernel_resources.kernels(LIB).items() if "lk_kernel_bx" in n and f"ILi{UPT2}ELb1ELi{NT2}E" in n]
    assert len(two) == 1, two
    assert int(two[0]["vgpr"]) <= 168 and int(two[0]["vgpr_spill"]) == 0 and int(two[0]["scratch"]) == 0, two
