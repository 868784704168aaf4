"""The two box builds that share the CUs in the Tracker2D pass, with their LDS
requests rounded to CU slots (bx_lds_request, csrc/psn_lk_kernels.h), against the
CPU oracle bit for bit (next, status, err). The LDS is filled with a pattern first
(PSN_LK_VARIANT_POISON_LDS: the whole request, padded tail included), so a read of
the tail, or of anything the kernel did not stage, shows. The two-wave build
lk_kernel_bx<8, true, 128>, the forward entry lk_kernel_fw<10, true>, and one call
that holds a window of each, with the slots (bx_pack=0) and with the planned
requests (bx_pack=1).

320 x 240 frames, maxLevel 2, 8 points a window: six inside the image, two whose
window crosses a border at level 0. Small windows reach the box kernel through
variant box=2.
  two-wave build (tiles of 16 threads x 8 units = 128 units)
    24 x 24   144 units: one tile and a partial one
    32 x 32   256 units: two tiles
    64 x 64   1,024 units: the build's largest window
  forward entry (windows of 2,049 - 2,560 units)
    56 x 147  2,058 units
    64 x 160  2,560 units
Scenes: "texture" (4-px cells of random gray, J moved by (2, 1): the exact integer
path) and "shift" (binary noise in 2-px cells, J moved by (3, 2): the sums leave
2^24 and run as ordered chains through the LDS planes).
"""
import functools

import numpy as np
import pytest

from mcmtt_opticalflow_amd import _lib
from mcmtt_opticalflow_amd import lk as glk

pytestmark = pytest.mark.gpu

W, H, ML, NPTS = 320, 240, 2, 8
TWO_WAVE, FW, BX10 = "lk_kernel_bx<8, true, 128>", "lk_kernel_fw<10, true>", "lk_kernel_bx<10, true>"
TWO_WAVE_WINS = [(24, 24), (32, 32), (64, 64)]
FORWARD_WINS = [(56, 147), (64, 160)]
SCENES = ["texture", "shift"]
BORDER = np.array([[3.3, 118.2], [300.4, 236.5]], np.float32)


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
    w, h = win
    rng = np.random.default_rng(5)
    xs = rng.uniform((w - 1) * 0.5 + 2, W - 3 - (w - 1) * 0.5, NPTS - 2)
    ys = rng.uniform((h - 1) * 0.5 + 2, H - 3 - (h - 1) * 0.5, NPTS - 2)
    pts = np.concatenate([np.stack([xs, ys], 1), BORDER]).astype(np.float32)
    pts.setflags(write=False)
    return pts


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


def _run(scene, wins, bx_pack=0):
    """One track call with a query of NPTS points per window, LDS poisoned: the
    results per window and the builds / entries launched."""
    f0, f1 = _frames(scene)
    L = _lib.load()
    pts = np.concatenate([_points(win) for win in wins])
    qs = [glk.make_query(0, 1, i * NPTS, NPTS, glk.make_params(win, ML)) for i, win in enumerate(wins)]
    with glk.LKContext(W, H, ring_slots=2, max_level_cap=ML, variants={"box": 2, "poison_lds": 1, "bx_pack": bx_pack}) as ctx:
        ctx.push_frame(0, f0)
        ctx.push_frame(1, f1)
        ctx.enable_timing(4, 1)
        out = ctx.track(qs, pts)
        ctx.sync()
        builds = {_lib.kernel_of_tag(t) for _, t in _lib.timing_launches(L, ctx.handle, 4)}
        entries = {_lib.kernel_of_tag(t) for t in _lib.timing_entries(L, ctx.handle, 4)}
    return [tuple(a[i * NPTS:(i + 1) * NPTS] for a in out) for i in range(len(wins))], builds, entries


def _same_bits(a, b, what):
    for x, y, n in zip(a, b, ("next", "status", "err")):
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), f"{what}: {n} differs"


def test_window_units():
    units = lambda w, h: h * ((w + 3) // 4)  # noqa: E731
    assert [units(*w) for w in TWO_WAVE_WINS] == [144, 256, 1024]
    assert [units(*w) for w in FORWARD_WINS] == [2058, 2560]
    assert all(w % 8 == 0 for w, _ in TWO_WAVE_WINS + FORWARD_WINS)  # no scalar tail


@pytest.mark.parametrize("win", TWO_WAVE_WINS)
@pytest.mark.parametrize("scene", SCENES)
def test_two_wave_build(oracle_mod, scene, win):
    (got,), builds, entries = _run(scene, [win])
    assert builds == entries == {TWO_WAVE}, (builds, entries)
    ref = _ref(oracle_mod, scene, win)
    assert ref[1][:NPTS - 2].all(), ref[1]  # the inner points track
    _same_bits(got, ref, f"{scene} {win} two-wave build vs oracle")


@pytest.mark.parametrize("win", FORWARD_WINS)
@pytest.mark.parametrize("scene", SCENES)
def test_forward_entry(oracle_mod, scene, win):
    (got,), builds, entries = _run(scene, [win])
    assert builds == {BX10} and entries == {FW}, (builds, entries)
    _same_bits(got, _ref(oracle_mod, scene, win), f"{scene} {win} forward entry vs oracle")


@pytest.mark.parametrize("scene", SCENES)
def test_one_call_of_both(oracle_mod, scene):
    """A 64 x 64 and a 64 x 160 query in one call, once with the slots and once with
    the planned requests: the same bits, the oracle's."""
    wins = [(64, 64), (64, 160)]
    slots, _, _ = _run(scene, wins, bx_pack=0)
    planned, _, _ = _run(scene, wins, bx_pack=1)
    for a, b, win in zip(slots, planned, wins):
        _same_bits(a, b, f"{scene} {win} bx_pack=0 vs bx_pack=1")
        _same_bits(a, _ref(oracle_mod, scene, win), f"{scene} {win} in a call of both vs oracle")
