"""The sliding A pass of the two-wave box build (lk_kernel_bx<8, true, 128>)
against the CPU oracle, bit for bit (next, status). Where a thread's eight units
are adjacent quads of one window row (w % 32 == 0, psn::bx_slides) each unit
takes its left neighbour's columns instead of computing them again; every other
window keeps the stand-alone units. The plan says which pass a call's workgroups
take (psn_lk_timing_slides), and every case asserts it.

160 x 120 frames, maxLevel 2, 16 points a case: ten inside the image and six whose
window crosses the left, right, top and bottom border and two corners at level 0
(the border form of the pass: the column and row masks act on carried values).
Small windows reach the box kernel through variant box=2, the two-wave build
through bx_waves=2.
  64 x 64   slides, eight fallback tiles     40 x 40   stand-alone units (QW = 10)
  32 x 32   slides, two tiles                24 x 24   stand-alone units (QW = 6)
  32 x 8, 64 x 8   slide, a single row group: 8 and 16 threads hold the window,
            the runs of all the others are past it
Scenes: "texture" (4-px cells of random gray, J moved by (2, 1): the exact integer
path) and "shift" (binary noise in 2-px cells, J moved by (3, 2): the A and b
sums leave 2^24 and run as ordered chains from the units' registers).
"""
import functools

import numpy as np
import pytest

from mcmtt_opticalflow_amd import _lib
from mcmtt_opticalflow_amd import lk as glk

pytestmark = pytest.mark.gpu

W, H, ML, NPTS = 160, 120, 2, 16
TWO_WAVE = "lk_kernel_bx<8, true, 128>"
SLIDE = [(64, 64), (32, 32), (32, 8), (64, 8)]
STAND_ALONE = [(40, 40), (24, 24)]
SCENES = ["texture", "shift"]
VARIANTS = dict(bx_waves=2, box=2)


@functools.lru_cache(maxsize=None)
def _frames(scene):
    rng = np.random.default_rng(21)
    if scene == "texture":
        f0 = np.kron(rng.integers(0, 256, (H // 4, W // 4)), np.ones((4, 4), np.int64))
        f1 = np.roll(f0, (1, 2), axis=(0, 1))
    else:
        f0 = 255 * np.kron(rng.integers(0, 2, (H // 2, W // 2)), np.ones((2, 2), np.int64))
        f1 = np.roll(f0, (2, 3), axis=(0, 1))
    f0, f1 = np.ascontiguousarray(f0, np.uint8), np.ascontiguousarray(f1, np.uint8)
    f0.setflags(write=False)
    f1.setflags(write=False)
    return f0, f1


@functools.lru_cache(maxsize=None)
def _points(win):
    """Ten points whose window is inside the image, then left, right, top, bottom,
    top-left and bottom-right: windows that cross those borders at level 0."""
    w, h = win
    rng = np.random.default_rng(5)
    xs = rng.uniform((w - 1) * 0.5 + 2, W - 3 - (w - 1) * 0.5, NPTS - 6)
    ys = rng.uniform((h - 1) * 0.5 + 2, H - 3 - (h - 1) * 0.5, NPTS - 6)
    edge = [(3.3, 60.2), (156.6, 59.7), (80.4, 2.2), (79.1, 117.5), (2.7, 1.6), (157.2, 118.3)]
    pts = np.concatenate([np.stack([xs, ys], 1), np.array(edge)]).astype(np.float32)
    pts.setflags(write=False)
    return pts


def _crosses(win):
    """Per point: its level-0 window's derivative columns / rows leave the image."""
    w, h = win
    p = _points(win)
    x0, y0 = np.floor(p[:, 0] - (w - 1) * 0.5), np.floor(p[:, 1] - (h - 1) * 0.5)
    return (x0 < 0) | (y0 < 0) | (x0 + w + 2 > W) | (y0 + h + 1 > H)


_REFS = {}


def _ref(oracle_mod, scene, win):
    """The oracle's result of one case, computed once."""
    if (scene, win) not in _REFS:
        f0, f1 = _frames(scene)
        r = oracle_mod.calc_optical_flow_pyr_lk(f0, f1, _points(win), win, ML)
        for a in r:
            a.setflags(write=False)
        _REFS[scene, win] = r
    return _REFS[scene, win]


def _run(scene, wins, **variants):
    """One track call with a query of NPTS points per window: the results per
    window, the kernels launched and the call's workgroups on the sliding pass."""
    f0, f1 = _frames(scene)
    L = _lib.load()
    pts = np.concatenate([_points(win) for win in wins])
    qs = [glk.make_query(0, 1, i * NPTS, NPTS, glk.make_params(win, ML)) for i, win in enumerate(wins)]
    with glk.LKContext(W, H, ring_slots=2, max_level_cap=ML, variants=dict(VARIANTS, **variants)) as ctx:
        ctx.push_frame(0, f0)
        ctx.push_frame(1, f1)
        ctx.enable_timing(4, 1)
        out = ctx.track(qs, pts)
        ctx.sync()
        names = {_lib.kernel_of_tag(t) for _, t in _lib.timing_launches(L, ctx.handle, 4)}
        slides = _lib.timing_slides(L, ctx.handle, 4)
    return [tuple(a[i * NPTS:(i + 1) * NPTS] for a in out) for i in range(len(wins))], names, slides


def _same_bits(a, b, what):
    for x, y, n in zip(a[:2], b[:2], ("next", "status")):
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), f"{what}: {n} differs"


def test_points_cross_every_border():
    for win in SLIDE + STAND_ALONE:
        c = _crosses(win)
        assert not c[:NPTS - 6].any() and c[NPTS - 6:].all(), (win, c)
    assert all(w % 8 == 0 for w, _ in SLIDE + STAND_ALONE)
    assert all((w // 4) % 8 == 0 for w, _ in SLIDE) and all((w // 4) % 8 for w, _ in STAND_ALONE)


@pytest.mark.parametrize("win", SLIDE)
@pytest.mark.parametrize("scene", SCENES)
def test_sliding_windows(oracle_mod, scene, win):
    (got,), names, slides = _run(scene, [win])
    assert names == {TWO_WAVE} and slides == [NPTS], (names, slides)
    ref = _ref(oracle_mod, scene, win)
    assert ref[1][:NPTS - 6].all() and ref[1][NPTS - 6:].any(), ref[1]  # tracked points, also among the border ones
    _same_bits(got, ref, f"{scene} {win} sliding pass vs oracle")


@pytest.mark.parametrize("win", STAND_ALONE)
@pytest.mark.parametrize("scene", SCENES)
def test_windows_that_keep_their_pass(oracle_mod, scene, win):
    (got,), names, slides = _run(scene, [win])
    assert names == {TWO_WAVE} and slides == [0], (names, slides)
    _same_bits(got, _ref(oracle_mod, scene, win), f"{scene} {win} stand-alone units vs oracle")


@pytest.mark.parametrize("scene", SCENES)
def test_one_launch_of_both(oracle_mod, scene):
    """Sliding and stand-alone queries in one launch of the build: the pass is the
    query's, picked per workgroup."""
    wins = [(64, 64), (40, 40), (32, 32), (24, 24)]
    got, names, slides = _run(scene, wins)
    assert names == {TWO_WAVE} and slides == [2 * NPTS], (names, slides)
    for g, win in zip(got, wins):
        _same_bits(g, _ref(oracle_mod, scene, win), f"{scene} {win} in a mixed launch vs oracle")


@pytest.mark.parametrize("win", [(64, 64), (32, 8)])
def test_poisoned_lds(oracle_mod, win):
    """LDS filled with a pattern first: the pass reads no byte it did not stage."""
    (got,), names, slides = _run("shift", [win], poison_lds=1)
    assert names == {TWO_WAVE} and slides == [NPTS], (names, slides)
    _same_bits(got, _ref(oracle_mod, "shift", win), f"shift {win} poisoned LDS vs oracle")
