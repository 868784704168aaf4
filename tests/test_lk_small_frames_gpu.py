"""LK where the border dominates (tests/lk_small_cases.py): frames whose top pyramid level
is only just larger than the window, frames smaller than the window, frames at most half
the window in one dimension and points outside the frame (taps that reflect-101 more than
once through Stager, dma_region, dma_patch_t, dma_rows and the J readers), strips and
1..8-pixel frames, through every kernel class and its fallback builds; nextPts, status and
err bit for bit against oracle/lk_oracle.c. tests/test_lk_small_frames.py holds the cases'
liveness on the CPU, and which of them hold tracked points with a twice-reflected tap."""
import numpy as np
import pytest

import lk_small_cases as sc
from mcmtt_opticalflow_amd import _lib
from mcmtt_opticalflow_amd import lk as glk
from mcmtt_opticalflow_amd._lib import ACCUM_SCALAR, USE_INITIAL_FLOW, PsnLkError
from test_lk_gpu import assert_same, oracle_ref

pytestmark = pytest.mark.gpu

# variant sets: every class; + what classes A and B add
V_ALL = [({}, 0), ({"poison_lds": 1}, 0)]
V_AB = V_ALL + [({}, ACCUM_SCALAR), ({"generic": 1}, 0), ({"large": 1}, 0)]


def _vid(v):
    env, flags = v
    return "-".join(f"{k}{x}" for k, x in env.items()) + ("scalar" if flags else "") or "default"


def _run(oracle_mod, W, H, win, ml, env, flags, outside=False):
    """One calcOpticalFlowPyrLK on the device as glk.calc_optical_flow_pyr_lk issues it (a ring
    as deep as the call needs), with its launches recorded -> (kernels, entries)."""
    f0, f1, pts, ref = sc.reference(oracle_mod, W, H, win, ml, scalar=bool(flags & ACCUM_SCALAR), outside=outside)
    cap = max(0, glk.effective_max_level(W, H, win[0], win[1], ml))
    with glk.LKContext(W, H, ring_slots=1, max_level_cap=min(cap, 5), variants=env) as ctx:
        ctx.enable_timing(4, 1)
        gpu = ctx.calc_optical_flow_pyr_lk(f0, f1, pts, win, ml, flags=flags)
        ctx.sync()
        kernels = {_lib.kernel_of_tag(t) for _, t in _lib.timing_launches(ctx._L, ctx.handle, 4)}
        entries = set(_lib.launched_kernels(ctx._L, ctx.handle, 4))
    assert_same(gpu, ref, f"{W}x{H} win {win} maxLevel {ml} {env} flags {flags}{' outside grid' if outside else ''}")
    return kernels, entries


@pytest.mark.parametrize("variant", V_AB, ids=_vid)
@pytest.mark.parametrize("case", sc.CLASS_A + sc.CLASS_B + sc.CLASS_N, ids=sc.case_id)
def test_lk_window_against_the_border(oracle_mod, case, variant):
    """Classes A, B and N on the grid over the frame. Only class N's taps reflect twice there."""
    W, H, win, ml, _ = case
    env, flags = variant
    kernels, entries = _run(oracle_mod, W, H, win, ml, env, flags)
    if not env and not flags:  # the default plan: the class is the window's, whatever the frame
        assert kernels == {sc.KERNEL[win]} and entries == {sc.ENTRY[win]}, (kernels, entries)
    if env.get("large"):
        assert kernels == {"lk_kernel_lg"}, kernels


@pytest.mark.parametrize("variant", V_AB, ids=_vid)
@pytest.mark.parametrize("case", sc.CLASS_B, ids=sc.case_id)
def test_lk_points_outside_the_frame(oracle_mod, case, variant):
    """Class B with points up to half a window outside the frame: most of such a window is
    reflected image, where it exceeds the frame more than once (err sums |J - I| over all of it)."""
    W, H, win, ml, _ = case
    env, flags = variant
    _run(oracle_mod, W, H, win, ml, env, flags, outside=True)


@pytest.mark.parametrize("case", [c for c in sc.CLASS_A + sc.CLASS_B + sc.CLASS_N if sc.KERNEL[c[2]] == "lk_kernel_lg"],
                         ids=sc.case_id)
def test_lk_large_window_j_from_the_level(oracle_mod, case):
    """The lk_kernel_lg cases with the iterations' J taps read from the level (lg_jr 0: the
    reflect-101 tap by tap branch of lg_diffs wherever the window leaves the level)."""
    W, H, win, ml, _ = case
    for env in ({"lg_jr": 0}, {"lg_jr": 0, "poison_lds": 1}):
        kernels, _ = _run(oracle_mod, W, H, win, ml, env, 0)
        assert kernels == {"lk_kernel_lg"}, kernels


@pytest.mark.parametrize("variant", V_ALL, ids=_vid)
@pytest.mark.parametrize("case", sc.CLASS_C, ids=sc.case_id)
def test_lk_tiny_frames(oracle_mod, case, variant):
    """Frames of 1..8 pixels a side: the oracle's outputs (mostly rejections), never an error
    code -- include/psn_lk.h documents no refusal for a frame smaller than the window."""
    W, H, win, ml = case
    env, flags = variant
    kernels, _ = _run(oracle_mod, W, H, win, ml, env, flags)
    assert kernels == {"lk_kernel_st"}, kernels


def test_lk_mixed_windows_on_a_small_frame(oracle_mod):
    """One track call on 130 x 100 at cap 2 with 21 x 21, 40 x 32, 64 x 64 and 33 x 37 queries
    (effective depths 2, 1, 0, 1): three launches, each query the oracle's."""
    W, H, cap = 130, 100, 2
    f0, f1 = sc.frames(W, H)
    wins = [(21, 21), (40, 32), (64, 64), (33, 37)]
    grids = [sc.grid(W, H, w) for w in wins]
    pts = np.concatenate(grids)
    first = np.cumsum([0] + [len(g) for g in grids])
    with glk.LKContext(W, H, ring_slots=2, max_level_cap=cap) as ctx:
        ctx.push_frame(0, f0)
        ctx.push_frame(1, f1)
        qs = [glk.make_query(0, 1, int(first[i]), len(grids[i]), glk.make_params(w, cap)) for i, w in enumerate(wins)]
        gn, gs, ge = ctx.track(qs, pts)
    for i, w in enumerate(wins):
        sl = slice(int(first[i]), int(first[i + 1]))
        ref = oracle_ref(oracle_mod, f0, f1, pts[sl], w, cap)
        assert_same((gn[sl], gs[sl], ge[sl]), ref, f"mixed call, query {w}")
        assert ref[1].mean() >= 0.5


@pytest.mark.parametrize("env", [{}, {"poison_lds": 1}, {"generic": 1}, {"large": 1}], ids=lambda e: _vid((e, 0)))
def test_lk_initial_flow_on_a_small_frame(oracle_mod, env):
    """USE_INITIAL_FLOW on 45 x 33 with a 21 x 21 window (level 0 only): guesses (+-3, +-3) off the
    true position, and four far outside the frame (their J windows never touch it)."""
    W, H, win = 45, 33, (21, 21)
    f0, f1 = sc.frames(W, H)
    pts = sc.grid(W, H, win)
    off = np.array([[3, 3], [3, -3], [-3, 3], [-3, -3]], np.float32)[np.arange(len(pts)) % 4]
    guess = pts + np.float32([2, 1]) + off
    far = np.array([[-500, 10], [900, 700], [20, -300], [5000, -4000]], np.float32)
    pts = np.concatenate([pts, np.float32([[22, 16], [10.5, 8.25], [30, 20], [5, 28]])])
    guess = np.concatenate([guess, far]).astype(np.float32)
    ref = oracle_ref(oracle_mod, f0, f1, pts, win, 3, flags=USE_INITIAL_FLOW, next_pts=guess)
    gpu = glk.calc_optical_flow_pyr_lk(f0, f1, pts, win, 3, flags=USE_INITIAL_FLOW, next_pts=guess, variants=env)
    assert_same(gpu, ref, f"initial flow {env}")
    assert ref[1][:-4].mean() >= 0.5


def test_small_frame_refusals_stay_codes():
    """What include/psn_lk.h does document on these frames: a window of 2 is PSN_LK_ERR_WINSIZE,
    a query deeper than the ring PSN_LK_ERR_LEVEL_CAP -- codes, on a 2 x 2 frame as on any."""
    f = np.arange(4, dtype=np.uint8).reshape(2, 2)
    p = np.float32([[0.25, 0.25]])
    with pytest.raises(PsnLkError) as e:
        glk.calc_optical_flow_pyr_lk(f, f, p, (2, 3), 0)
    assert e.value.code == -2
    f = np.zeros((40, 40), np.uint8)
    with glk.LKContext(40, 40, ring_slots=2, max_level_cap=0) as ctx:
        ctx.push_frame(0, f)
        ctx.push_frame(1, f)
        with pytest.raises(PsnLkError) as e:  # 3 x 3 on 40 x 40 reaches level 3
            ctx.track([glk.make_query(0, 1, 0, 1, glk.make_params((3, 3), 3))], p)
        assert e.value.code == -6
