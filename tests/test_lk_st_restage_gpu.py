"""The single-tile kernel's J-region restage inside the iterations, in both level
loops: one-wave (21x21: 7 rows per lane, 9x15: 4 rows) and multi-wave (40x20, and
21x21 with onewave 0).

The second frame is the first moved down by S = 7 rows on a smooth synth texture,
one level, no initial flow: a point has to walk the 7 rows in its iterations. The
staged region covers the window starts floor(y0 - hwy) - 4 ... + 4 exactly
(st_jreg_h, jr_covers), so a point whose window start ends at least 6 rows from
where it began has been restaged, whatever the path of its iterations. S and the
texture seed were chosen on the CPU with the oracle (of seeds 0-5 and S = 6, 7, 8
every combination gives at least 10 such points per window; this one 24, 22 and 24
of 24); the test asserts at least 8 from the oracle's output before it compares.
"""
import functools

import numpy as np
import pytest

from mcmtt_opticalflow_amd import _lib, synth
from mcmtt_opticalflow_amd import lk as glk
from test_lk_gpu import assert_same

pytestmark = pytest.mark.gpu

W, H, S, SEED = 192, 128, 7, 1
CASES = [((21, 21), {}), ((21, 21), {"poison_lds": 1}), ((21, 21), {"onewave": 0}),
         ((9, 15), {}), ((9, 15), {"poison_lds": 1}),
         ((40, 20), {}), ((40, 20), {"poison_lds": 1})]


@functools.lru_cache(maxsize=None)
def _inputs():
    tex = synth.texture(W, H + S, SEED)
    f0, f1 = np.ascontiguousarray(tex[S:]), np.ascontiguousarray(tex[:H])  # the content moves down by S rows
    grid = np.stack(np.meshgrid(np.linspace(44, 148, 6), np.linspace(34, 92, 4)), -1).reshape(-1, 2)
    pts = (grid + np.array([0.25, 0.5])).astype(np.float32)  # 24 interior points, windows well inside
    for a in (f0, f1, pts):
        a.setflags(write=False)
    return f0, f1, pts


@functools.lru_cache(maxsize=None)
def _ref(win):
    """The oracle's result of one window, computed once."""
    import oracle

    f0, f1, pts = _inputs()
    ref = oracle.calc_optical_flow_pyr_lk(f0, f1, pts, win, 0)
    for a in ref:
        a.setflags(write=False)
    return ref


@pytest.mark.parametrize("win,env", CASES)
def test_restage_inside_the_iterations(oracle_mod, win, env):
    f0, f1, pts = _inputs()
    ref = _ref(win)
    hwy = np.float32((win[1] - 1) * 0.5)
    moved = np.abs(np.floor(ref[0][:, 1] - hwy) - np.floor(pts[:, 1] - hwy))
    restaged = int(((ref[1] == 1) & (moved >= 6)).sum())
    print(f"{win} {env}: {restaged} of {len(pts)} points tracked with a window start >= 6 rows away")
    assert restaged >= 8
    with glk.LKContext(W, H, ring_slots=1, max_level_cap=0, variants=env) as ctx:
        ctx.enable_timing(4, 1)
        gpu = ctx.calc_optical_flow_pyr_lk(f0, f1, pts, win, 0)
        ctx.sync()
        names = set(_lib.launched_kernels(_lib.load(), ctx.handle, 4))
    assert names == {"lk_kernel_st"}, names
    assert_same(gpu, ref, f"{win} {env}")
