"""gridfast_cell_kernel and gridfast_select_kernel (csrc/psn_gridfast.hip) on the edge
cases of tests/gridfast_cases.py: strip height 16, frames past 4096 (no keypoint list),
one image under both pass counts, keepStrongest ties carried across strips and thread
runs, equal responses across a strip seam / the roi edge / a cell's 3-px border, the
8-bit score's extremes, the select kernel's rank and sort paths around their boundary,
tiny cells; then the documented refusals and what a call leaves outside its rows.
Totals and every point against oracle/gridfast_oracle.c, exact.
tests/test_gridfast_edges.py proves on the CPU that each case reaches its branch."""
import ctypes

import numpy as np
import pytest

import gridfast_cases as gc
from mcmtt_opticalflow_amd import hip
from mcmtt_opticalflow_amd import lk as glk
from mcmtt_opticalflow_amd._lib import PsnLkError
from test_gridfast import _compare

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -8


@pytest.fixture(scope="module")
def context():
    """context(w, h): one LKContext per frame size, kept while the cases stay at that size."""
    held = {}

    def get(w, h):
        if (w, h) not in held:
            for c in held.values():
                c.close()
            held.clear()
            held[w, h] = glk.LKContext(w, h, ring_slots=2, max_level_cap=0)
        return held[w, h]

    yield get
    for c in held.values():
        c.close()


def _params(c, **over):
    return glk.gridfast_params(**{**dict(threshold=c.threshold, nonmax=c.nonmax, max_total=c.max_total, grid=c.grid,
                                         cap=c.cap), **over})


def _run(oracle_mod, context, c):
    ctx = context(*c.size)
    ctx.push_frame(0, c.frame)
    g_pts, g_tot = ctx.gridfast_detect(0, c.rois, _params(c), seed=c.seed)
    r_pts, r_tot = gc.reference(oracle_mod, c)
    _compare(g_pts, g_tot, r_pts, r_tot, c.rois)


@pytest.mark.parametrize("case", sorted(gc.ALL, key=lambda c: c.size), ids=gc.case_id)
def test_edge_case(oracle_mod, context, case):
    _run(oracle_mod, context, case)


@pytest.mark.parametrize("cap", (0,) + gc.SELECT_CAPS)
def test_select_caps_at_n4096(oracle_mod, context, cap):
    """4,096 candidates through the rank path (caps to 496; 511 with seed 0: 512 keys), the
    sort (511 with seed 3: 513 keys; every larger cap, cap > n included) and cap 0 (counts
    0, totals 4,096); then rois of 4,096, 0, 4,096 and 1 keypoints in one launch."""
    for seed in gc.SELECT_SEEDS:
        _run(oracle_mod, context, gc.select_case(cap, seed))
    _run(oracle_mod, context, gc.select_mixed(cap, 5))


def test_sets_split_by_the_launch_boundary(oracle_mod, context):
    """The seam image and a lattice on two slots in one psn_gridfast_detect_device_sets call
    of 70 rois: the second set is split by the 64-roi launch boundary; the shuffle key is
    the roi's index in its set."""
    a, b = gc.sets_case()
    ctx = context(*a.size)
    ctx.push_frame(1, a.frame)
    ctx.push_frame(0, b.frame)
    got = ctx.gridfast_detect_sets([1, 0], [a.rois, b.rois], _params(a), seed=a.seed)
    for (g_pts, g_tot), c in zip(got, (a, b)):
        r_pts, r_tot = gc.reference(oracle_mod, c)
        _compare(g_pts, g_tot, r_pts, r_tot, c.rois)


def test_refusals_leave_the_context_usable(oracle_mod, context):
    """A 4200-wide frame in 4 columns (cells of 1050 > 1030) is PSN_LK_ERR_UNSUPPORTED and
    the same context detects in 5 columns; a 17 x 16 grid, max_total 4097 and cap -1 are
    PSN_LK_ERR_ARG, and the next valid call is exact. (psn_lk_create takes the 4200 x 40
    and 4100 x 40 frames as they are.)"""
    c = gc.Case("wide4200", lambda: gc.lattice(4200, 40, 18), [(0, 0, 4199, 39), (4100, 0, 100, 40)], grid=(1, 5))
    ctx = context(*c.size)
    ctx.push_frame(0, c.frame)
    with pytest.raises(PsnLkError) as e:
        ctx.gridfast_detect(0, c.rois, _params(c, grid=(1, 4)))
    assert e.value.code == ERR_UNSUPPORTED
    _run(oracle_mod, context, c)
    assert gc.reference(oracle_mod, c)[1].tolist() == [1000, 192]
    for bad in (dict(grid=(17, 16)), dict(max_total=4097), dict(cap=-1), dict(grid=(0, 4))):
        with pytest.raises(PsnLkError) as e:
            ctx.gridfast_detect(0, c.rois, _params(c, **bad))
        assert e.value.code == ERR_ARG, bad
        _run(oracle_mod, context, c)


SENTINEL = np.float32(-12345.5)
SENTINEL_I = np.int32(-77)


@pytest.mark.parametrize("cap", (5000, 100, 1))
def test_device_call_writes_only_its_rows(oracle_mod, context, cap):
    """psn_gridfast_detect_device into sentinel-filled buffers, rois of 4,096, 0, 4,096 and 1
    keypoints: roi r's points are rows [r * cap, r * cap + count[r]); the rows from count[r] on
    (cap 5000 > n; at caps 100 and 1 the whole of the empty roi after a capped one) and the
    rows and counters behind the last roi keep the sentinel."""
    c = gc.select_mixed(cap, 5)
    n = len(c.rois)
    ctx = context(*c.size)
    ctx.push_frame(0, c.frame)
    d_xy = hip.DeviceBuffer.from_array(np.full(((n + 1) * cap, 2), SENTINEL))
    d_cnt, d_tot = (hip.DeviceBuffer.from_array(np.full(n + 1, SENTINEL_I)) for _ in range(2))
    try:
        ctx.gridfast_detect_device(0, c.rois, _params(c), c.seed, d_xy.addr, d_cnt.addr, d_tot.addr)
        ctx.sync()
        xy = d_xy.to_array((n + 1, cap, 2), np.float32)
        cnt, tot = d_cnt.to_array(n + 1, np.int32), d_tot.to_array(n + 1, np.int32)
    finally:
        for b in (d_xy, d_cnt, d_tot):
            b.free()
    r_pts, r_tot = gc.reference(oracle_mod, c)
    assert tot.tolist() == r_tot.tolist() + [SENTINEL_I] and cnt.tolist() == [len(p) for p in r_pts] + [SENTINEL_I]
    for r in range(n):
        np.testing.assert_array_equal(xy[r, :cnt[r]], r_pts[r], err_msg=f"roi {r}")
        assert (xy[r, cnt[r]:] == SENTINEL).all(), f"roi {r}: rows past its count"
    assert (xy[n] == SENTINEL).all()


def test_host_call_writes_only_its_rows(oracle_mod, context):
    """psn_gridfast_detect into sentinel-filled host arrays: nroi * cap rows and nroi counters
    are the call's; what lies behind them keeps the sentinel."""
    c = gc.select_mixed(600, 5)
    n = len(c.rois)
    ctx = context(*c.size)
    ctx.push_frame(0, c.frame)
    xy = np.full((n + 1, c.cap, 2), SENTINEL)
    cnt, tot = np.full(n + 1, SENTINEL_I), np.full(n + 1, SENTINEL_I)
    rois = np.ascontiguousarray(np.asarray(c.rois, np.int32))
    rc = ctx._L.psn_gridfast_detect(ctx.handle, 0, rois.ctypes.data, n, ctypes.byref(_params(c)), ctypes.c_uint32(c.seed),
                                    xy.ctypes.data, cnt.ctypes.data, tot.ctypes.data)
    assert rc == 0
    r_pts, r_tot = gc.reference(oracle_mod, c)
    assert tot.tolist() == r_tot.tolist() + [SENTINEL_I] and cnt.tolist() == [len(p) for p in r_pts] + [SENTINEL_I]
    for r in range(n):
        np.testing.assert_array_equal(xy[r, :cnt[r]], r_pts[r], err_msg=f"roi {r}")
    assert (xy[n] == SENTINEL).all()
