"""PSN_LK_ERR_STATUS_ONLY: a call that requests err only for the level-0 bounds
re-check that comes with it. next and status with the flag are the oracle's of a
call with err, bit for bit, and those of the same launch without the flag; what
err[] holds is unspecified and not looked at. With GET_MIN_EIGENVALS the flag
does nothing: err is the minimum eigenvalue. Variant err_status=1 drops the flag
(the A/B switch): err is the oracle's again.

One window per kernel that honours the flag, 48 points each on a 320 x 240 pair
of uncorrelated binary-noise frames, three iterations (COUNT, 3): the updates
are erratic, and the last one is checked by nothing but the re-check. 12 points
lie inside the image; 36 start with their window 1 - 2.5 px inside one of the four
limits of win_outside (the window then overlaps the image by one to three
columns or rows: the gradients' border is zero, a window wholly outside fails the
eigenvalue test first). The re-check is what clears status where the oracle
reports 1 without err and 0 with it; the seed of each window's points was chosen
on the CPU so that this happens for at least 4 of its points, and the test
asserts that count from the oracle.
"""
import functools

import numpy as np
import pytest

from mcmtt_opticalflow_amd import _lib
from mcmtt_opticalflow_amd import lk as glk
from mcmtt_opticalflow_amd._lib import ERR_STATUS_ONLY, GET_MIN_EIGENVALS

pytestmark = pytest.mark.gpu

W, H, ML = 320, 240, 3
CRIT = (1, 3, 0.0)
N_IN, N_EDGE = 12, 36
# window -> (the seed of its points, the kernel of its launch, variants that select it)
CASES = {
    (64, 64): (1, "lk_kernel_bx<8, true, 128>", {}),   # the two-wave build
    (64, 160): (1, "lk_kernel_fw<10, true>", {}),      # the forward entry
    (21, 21): (8, "lk_kernel_st", {}),
    (100, 250): (0, "lk_kernel_lg", {}),
    (30, 70): (6, "lk_kernel_bx<4, false>", {}),       # a scalar-tail build of the box kernel
}
TILED = ((30, 70), "lk_kernel", {"generic": 1})        # the row-tiled kernel, same points


@functools.lru_cache(maxsize=None)
def _frames():
    rng = np.random.default_rng(31)
    f0, f1 = [(128 + (254 * rng.integers(0, 2, (H, W)) - 127)).astype(np.uint8) for _ in range(2)]
    for f in (f0, f1):
        f.setflags(write=False)
    return f0, f1


@functools.lru_cache(maxsize=None)
def _points(win):
    rng = np.random.default_rng(CASES[win][0])
    w, h = win
    hwx, hwy = (w - 1) * 0.5, (h - 1) * 0.5
    inner = np.stack([rng.uniform(20, W - 20, N_IN), rng.uniform(20, H - 20, N_IN)], 1)
    d = rng.uniform(1.0, 2.5, N_EDGE)
    ax, ay = rng.uniform(30, W - 30, N_EDGE), rng.uniform(30, H - 30, N_EDGE)
    edge = []
    for k in range(N_EDGE):  # floor(x - hw) = -w and W - 1 are the last values inside; the same in y
        edge.append([[-w + hwx + d[k], ay[k]], [W + hwx - d[k], ay[k]],
                     [ax[k], -h + hwy + d[k]], [ax[k], H + hwy - d[k]]][k % 4])
    pts = np.concatenate([inner, np.array(edge)]).astype(np.float32)
    pts.setflags(write=False)
    return pts


_REFS = {}


def _ref(oracle_mod, win, flags=0, want_err=True):
    """The oracle's result of one case, computed once."""
    if (win, flags, want_err) not in _REFS:
        f0, f1 = _frames()
        r = oracle_mod.calc_optical_flow_pyr_lk(f0, f1, _points(win), win, ML, criteria=CRIT, flags=flags, want_err=want_err)
        for a in r:
            if a is not None:
                a.setflags(write=False)
        _REFS[win, flags, want_err] = r
    return _REFS[win, flags, want_err]


def _run(ctx, win, flags):
    f0, f1 = _frames()
    ctx.enable_timing(4, 1)
    out = ctx.calc_optical_flow_pyr_lk(f0, f1, _points(win), win, ML, criteria=CRIT, flags=flags)
    ctx.sync()
    names = set(_lib.launched_kernels(_lib.load(), ctx.handle, 4))
    return out, names


def _same_bits(a, b, what, fields=("next", "status", "err")):
    for x, y, n in zip(a, b, ("next", "status", "err")):
        if n in fields:
            assert x.tobytes() == y.tobytes(), f"{what}: {n} differs"


def _check(oracle_mod, win, kernel, variants):
    ref = _ref(oracle_mod, win)
    cleared = int(((_ref(oracle_mod, win, want_err=False)[1] == 1) & (ref[1] == 0)).sum())
    print(f"{win} {kernel}: the re-check clears status of {cleared} points; {int(ref[1].sum())} of {len(ref[1])} tracked")
    assert cleared >= 4
    with glk.LKContext(W, H, ring_slots=1, max_level_cap=ML, variants=variants) as ctx:
        plain, names = _run(ctx, win, 0)
        assert names == {kernel}, names
        flagged, names = _run(ctx, win, ERR_STATUS_ONLY)
        assert names == {kernel}, names
        ctx.set_variant("err_status", 1)
        ignored, _ = _run(ctx, win, ERR_STATUS_ONLY)
    _same_bits(plain, ref, f"{win} without the flag vs oracle")
    _same_bits(flagged, ref, f"{win} with the flag vs oracle", ("next", "status"))
    _same_bits(flagged, plain, f"{win} with the flag vs without", ("next", "status"))
    _same_bits(ignored, ref, f"{win} flag dropped by the variant vs oracle")


@pytest.mark.parametrize("win", list(CASES))
def test_err_status_only(oracle_mod, win):
    _, kernel, variants = CASES[win]
    _check(oracle_mod, win, kernel, variants)


def test_err_status_only_row_tiled(oracle_mod):
    win, kernel, variants = TILED
    _check(oracle_mod, win, kernel, variants)


def test_min_eigenvals_ignore_the_flag(oracle_mod):
    """GET_MIN_EIGENVALS | ERR_STATUS_ONLY: err is the minimum eigenvalue (forward entry and two-wave build)."""
    for win in ((64, 160), (64, 64)):
        ref = _ref(oracle_mod, win, GET_MIN_EIGENVALS)
        assert np.count_nonzero(ref[2]) >= 24
        with glk.LKContext(W, H, ring_slots=1, max_level_cap=ML) as ctx:
            got, names = _run(ctx, win, GET_MIN_EIGENVALS | ERR_STATUS_ONLY)
        assert names == {CASES[win][1]}, names
        _same_bits(got, ref, f"{win} minEig with the flag vs oracle")
