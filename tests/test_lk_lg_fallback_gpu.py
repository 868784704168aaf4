"""The ordered-chain fallbacks of the large-window kernel (lk_kernel_lg, forced with
variant large=1) on the smallest windows that reach each branch of its tile writer and
of its chains-to-result step, for both tile sizes (lg_jr 1: 192 quads, lg_jr 0: 128),
bit for bit against the CPU oracle.

Uniform-random 480 x 480 frames: the A sums of every window inside the image pass
2^24 per SSE2 lane (asserted on the CPU from the frames alone), so the A fallback
runs at level 0 for certain. Which b chains fall back is not claimed: the fallback
covers all chains once one fails, and the oracle comparison covers the rest.

  (38, 45)  450 quads, 2 per thread: three 192-quad tiles (four of 128), a partial
            last one; A tail 2 px, b tail 6 px. Also with ACCUM_SCALAR: every term in
            the tail chain.
  (13, 37)  148 quads: a single 192-quad tile (the ntiles == 1 path; two of 128), 1 quad
            per thread with idle threads; A tail 1 px, b tail 5 px.
  (64, 24)  384 quads, no tail: exactly two full 192-quad tiles (three of 128), no pad
            block.
"""
import numpy as np
import pytest

from lk_window_sums import lane_sums
from mcmtt_opticalflow_amd import _lib
from mcmtt_opticalflow_amd import lk as glk
from mcmtt_opticalflow_amd._lib import ACCUM_SCALAR
from test_lk_gpu import assert_same, oracle_ref

pytestmark = pytest.mark.gpu

W = H = 480
ML, CRIT = 1, (1, 2, 0.0)
EXACT = 1 << 24
CASES = [((38, 45), 0), ((38, 45), ACCUM_SCALAR), ((13, 37), 0), ((64, 24), 0)]

_SCENE, _REFS = [], {}


def _scene():
    if not _SCENE:
        rng = np.random.default_rng(19)
        f0 = rng.integers(0, 256, (H, W), dtype=np.uint8)
        f1 = rng.integers(0, 256, (H, W), dtype=np.uint8)
        pts = np.concatenate([rng.uniform(100, 380, (12, 2)), [[2, 3], [478.5, 300]]]).astype(np.float32)
        for a in (f0, f1, pts):
            a.setflags(write=False)
        _SCENE.append((f0, f1, pts))
    return _SCENE[0]


def _ref(oracle_mod, win, flags):
    """The oracle's result of one case, computed once for both tile sizes."""
    if (win, flags) not in _REFS:
        f0, f1, pts = _scene()
        r = oracle_ref(oracle_mod, f0, f1, pts, win, ML, criteria=CRIT, flags=flags)
        for a in r:
            a.setflags(write=False)
        _REFS[win, flags] = r
    return _REFS[win, flags]


def _inside(pts, win):
    """The points whose window, with its bilinear and Scharr taps, lies inside the image."""
    w, h = win
    ox, oy = pts[:, 0] - (w - 1) * 0.5, pts[:, 1] - (h - 1) * 0.5
    return pts[(ox >= 1) & (oy >= 1) & (ox + w + 1 <= W - 1) & (oy + h + 1 <= H - 1)]


def test_cases_reach_their_branches():
    quads = {win: win[1] * ((win[0] + 3) // 4) for win, _ in CASES}
    assert quads == {(38, 45): 450, (13, 37): 148, (64, 24): 384}
    assert [-(-quads[38, 45] // t) for t in (192, 128)] == [3, 4] and quads[38, 45] % 192 and quads[38, 45] % 128
    assert 128 < quads[13, 37] <= 192  # a single 192-quad tile (two of 128), fewer quads than the 256 threads
    assert quads[64, 24] == 2 * 192 == 3 * 128 and 64 % 8 == 0  # full tiles only, no tail chain
    assert (38 % 4, 38 % 8, 13 % 4, 13 % 8) == (2, 6, 1, 5)  # A and b tail pixels per row


@pytest.mark.parametrize("jr", [1, 0], ids=["tq192", "tq128"])
@pytest.mark.parametrize("win,flags", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"flags{v}")
def test_lg_ordered_chains(oracle_mod, win, flags, jr):
    f0, f1, pts = _scene()
    inner = _inside(pts, win)
    assert len(inner) == 12  # all but the two border points
    s = lane_sums(oracle_mod, f0, inner, win)
    print(f"{win}: weakest largest per-lane sum of Ix^2 {s[:, 0].min() / EXACT:.2f} x 2^24")
    assert len(s) == 12 and (s[:, 0] > EXACT).all()  # the A fallback runs for each of them
    ref = _ref(oracle_mod, win, flags)
    with glk.LKContext(W, H, ring_slots=1, max_level_cap=ML, variants={"large": 1, "lg_jr": jr}) as ctx:
        ctx.enable_timing(4, 1)
        gpu = ctx.calc_optical_flow_pyr_lk(f0, f1, pts, win, ML, criteria=CRIT, flags=flags)
        ctx.sync()
        kernels = {_lib.kernel_of_tag(t) for _, t in _lib.timing_launches(ctx._L, ctx.handle, 4)}
    assert kernels == {"lk_kernel_lg"}, kernels
    assert_same(gpu, ref, f"win {win} flags {flags} lg_jr {jr}")
