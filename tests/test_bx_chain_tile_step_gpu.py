"""The chain lanes' tile step against the CPU oracle, bit for bit (next, status).
The forward entry (lk_kernel_fw<10, true>) sums full fallback tiles by the
straight-line chain_sum_nt with the tile geometry taken once per fallback and a
partial last tile by chain_sum_pl, in the A barrier loop and the b flag loop; the
two-wave build (lk_kernel_bx<8, true, 128>) keeps chain_sum_pl for every tile
(the straight-line sum measured no gain there) and is held to the same windows
by tile count: many full tiles, two, and one with a partial tile.

320 x 240 frames, maxLevel 2, 16 points a case, each case with and without LDS
poisoned first (PSN_LK_VARIANT_POISON_LDS). No-tail windows (w % 8 == 0, SSE2
order) picked by their tile arithmetic (tests/test_bx_chain_tile_step.py holds the
counts): the forward entry's 64 x 160 (8 full tiles of 320 units), 56 x 160 (7)
and 64 x 129 (6 and a partial tile of 144 units); the two-wave build's 64 x 64 (8
full tiles of 128 units), 32 x 32 (2) and 24 x 24 (1 and a partial tile of 16
units) -- the last two through variant box=2, without which the single-tile
kernel takes them. The forward windows are taller than half the frame, so level 0
is their only level; the two-wave windows run two or three levels, and the
preconditions below are those of level 0.

Scenes (preconditions on the CPU in exact integers: the oracle's Scharr gradients,
the window's 14-bit bilinear weights, per-lane (x & 3) prefixes in unit order):
  stripes, checker  0 / 255 in 2-px stripes / cells: a prefix of an A11 lane chain
           passes 2^24 inside tile 0 for every point -- the A chains start at tile 0;
  half     128 above row 120, the checkerboard below: the first such prefix falls
           in a later tile (and, where the window has more than one half wave, in
           a later half wave: the chains start mid-window);
  shift    binary noise in 2-px cells, J the frame moved by (3, 2) px: the b
           prefixes pass 2^24 as well, the ordered b chains run several tiles.
           From d * gx of the oracle's first level-0 iteration in exact integers:
           J sampled at the point itself for the forward windows (one level), at
           twice the oracle's result on the level-1 images for the two-wave windows.
The forward entry is also compared with lk_kernel_bx<10, true> of the same call
(variant fw=1), which keeps chain_sum_pl and the parent's loops.
"""
import functools

import numpy as np
import pytest

from mcmtt_opticalflow_amd import _lib
from mcmtt_opticalflow_amd import lk as glk

pytestmark = pytest.mark.gpu

W, H, ML, NPTS = 320, 240, 2, 16
FW, BX, TWO_WAVE = "lk_kernel_fw<10, true>", "lk_kernel_bx<10, true>", "lk_kernel_bx<8, true, 128>"
FW_WINDOWS = [(64, 160), (56, 160), (64, 129)]
TW_WINDOWS = [(64, 64), (32, 32), (24, 24)]
WINDOWS = FW_WINDOWS + TW_WINDOWS
SCENES = ["stripes", "checker", "half", "shift"]
EXACT = 1 << 24
MID = 120  # scene "half": flat above this row
CRIT_SHIFT = (1, 3, 0.0)  # three iterations on the moved frame


def _geo(win):
    """(units per tile, units per half wave, quads per row) of the window's build."""
    w, _ = win
    return (320, 320, w // 4) if win in FW_WINDOWS else (128, 256, w // 4)


@functools.lru_cache(maxsize=None)
def _frames(scene):
    y, x = np.mgrid[0:H, 0:W]
    if scene == "stripes":
        f0 = 255 * ((x >> 1) & 1)
        f1 = f0
    elif scene in ("checker", "half"):
        f0 = 255 * (((x >> 1) + (y >> 1)) & 1)
        if scene == "half":
            f0 = np.where(y < MID, 128, f0)
        f1 = f0
    else:
        rng = np.random.default_rng(14)  # (a seed for which the b precondition holds for every point of every window)
        f0 = 255 * np.kron(rng.integers(0, 2, (H // 2, W // 2)), np.ones((2, 2), np.int64))
        f1 = np.roll(f0, (2, 3), axis=(0, 1))
    f0, f1 = np.ascontiguousarray(f0, np.uint8), np.ascontiguousarray(f1, np.uint8)
    f0.setflags(write=False)
    f1.setflags(write=False)
    return f0, f1


@functools.lru_cache(maxsize=None)
def _points(scene, win):
    """16 points whose windows are inside the image, at fractional x. Scene "half":
    integer window tops (the rows above the first row with a gradient, MID - 1, are
    then exactly flat) such that the flat rows cover the first half wave's units (the
    first tile's where the window is a single half wave) and the window still
    reaches the checkerboard."""
    w, h = win
    tu, hwu, qw = _geo(win)
    rng = np.random.default_rng(3)
    xs = rng.uniform((w - 1) * 0.5 + 2, W - 3 - (w - 1) * 0.5, NPTS)
    if scene == "half":
        need = hwu if h * qw > hwu else tu
        rows = -(-need // qw)  # flat window rows wanted
        top = min(MID - 1 - rows, H - 2 - h)
        assert top >= 1 and top + h > MID, (win, top)  # the window's last row is a checkerboard row
        ys = np.full(NPTS, top + (h - 1) * 0.5)
    else:
        ys = rng.uniform((h - 1) * 0.5 + 2, H - 3 - (h - 1) * 0.5, NPTS)
    pts = np.stack([xs, ys], 1).astype(np.float32)
    pts.setflags(write=False)
    return pts


def _crit(scene):
    return CRIT_SHIFT if scene == "shift" else (3, 30, 0.01)


_REFS = {}


def _ref(oracle_mod, scene, win):
    """The oracle's result of one case, computed once."""
    if (scene, win) not in _REFS:
        f0, f1 = _frames(scene)
        r = oracle_mod.calc_optical_flow_pyr_lk(f0, f1, _points(scene, win), win, ML, criteria=_crit(scene))
        for a in r:
            a.setflags(write=False)
        _REFS[scene, win] = r
    return _REFS[scene, win]


def _run(scene, win, **variants):
    """One call on the GPU: (next, status, err), the kernel names of its launches
    (the build) and of its entries."""
    f0, f1 = _frames(scene)
    L = _lib.load()
    with glk.LKContext(W, H, ring_slots=1, max_level_cap=ML, variants=variants) as ctx:
        ctx.enable_timing(4, 1)
        out = ctx.calc_optical_flow_pyr_lk(f0, f1, _points(scene, win), win, ML, criteria=_crit(scene))
        ctx.sync()
        names = {_lib.kernel_of_tag(t) for _, t in _lib.timing_launches(L, ctx.handle, 4)}
        entries = {_lib.kernel_of_tag(t) for t in _lib.timing_entries(L, ctx.handle, 4)}
    return out, names, entries


def _same_bits(a, b, what):
    for x, y, n in zip(a[:2], b[:2], ("next", "status")):
        assert x.tobytes() == y.tobytes(), f"{what}: {n} differs"


def _weights(x, y, win):
    """Integer window origin and the 14-bit bilinear weights of the window at (x, y)."""
    w, h = win
    px = np.float32(x) - np.float32((w - 1) * 0.5)
    py = np.float32(y) - np.float32((h - 1) * 0.5)
    ix, iy = int(np.floor(px)), int(np.floor(py))
    a, b = float(px - np.float32(ix)), float(py - np.float32(iy))
    w00, w01, w10 = round((1 - a) * (1 - b) * 16384), round(a * (1 - b) * 16384), round((1 - a) * b * 16384)
    return ix, iy, (w00, w01, w10, 16384 - w00 - w01 - w10)


def _interp(src, ix, iy, win, wts, rnd, shift):
    """src (2-D int64) at the window's pixels: the fixed-point bilinear of calcOpticalFlowPyrLK."""
    w, h = win
    r = src[iy:iy + h + 1, ix:ix + w + 1]
    return (r[:-1, :-1] * wts[0] + r[:-1, 1:] * wts[1] + r[1:, :-1] * wts[2] + r[1:, 1:] * wts[3] + rnd) >> shift


def _first_over(terms, qw):
    """The unit index (row-major, qw units a row) at which a lane chain's (x & 3)
    prefix of `terms` (h x w, exact integers) first leaves +-2^24; None: never."""
    first = None
    for lane in range(4):
        pre = np.abs(np.cumsum(terms[:, lane::4].ravel()))
        over = np.nonzero(pre > EXACT)[0]
        if len(over) and (first is None or over[0] < first):
            first = int(over[0])
    return first


def _a11_first(oracle_mod, scene, win):
    """Per point the unit at which an A11 lane-chain prefix first passes 2^24 at level 0."""
    f0, _ = _frames(scene)
    g = oracle_mod.scharr(f0).astype(np.int64)
    out = []
    for x, y in _points(scene, win):
        ix, iy, wts = _weights(x, y, win)
        gx = _interp(g[..., 0], ix, iy, win, wts, 8192, 14)
        out.append(_first_over(gx * gx, _geo(win)[2]))
    return out


def _level0_start(oracle_mod, scene, win):
    """The position the oracle's level-0 iterations start from, per point: the point
    itself where level 0 is the only level, else twice the result of the same call
    on the level-1 images with the points halved (the coarser levels' arithmetic is
    the same: the scales are powers of two)."""
    f0, f1 = _frames(scene)
    pts = _points(scene, win)
    ml = oracle_mod.effective_max_level(W, H, win[0], win[1], ML)
    if ml == 0:
        return pts
    g0, g1 = oracle_mod.build_pyramid(f0, 2)[1], oracle_mod.build_pyramid(f1, 2)[1]
    assert oracle_mod.effective_max_level(g0.shape[1], g0.shape[0], win[0], win[1], ml - 1) == ml - 1
    half = (pts * np.float32(0.5)).astype(np.float32)
    nxt, _, _ = oracle_mod.calc_optical_flow_pyr_lk(g0, g1, half, win, ml - 1, criteria=_crit(scene))
    return (nxt * np.float32(2)).astype(np.float32)


def _b_first_exact(oracle_mod, scene, win):
    """Per point the unit at which a lane-chain prefix of d * gx of the oracle's FIRST
    level-0 iteration (I and gx with the window's weights at the point, J with its
    own at the iteration's start) first leaves +-2^24, in exact integers. Points
    whose J window is not inside the image are left out."""
    w, h = win
    f0, f1 = _frames(scene)
    g = oracle_mod.scharr(f0).astype(np.int64)
    out = []
    for (x, y), (sx, sy) in zip(_points(scene, win), _level0_start(oracle_mod, scene, win)):
        ix, iy, wts = _weights(x, y, win)
        jx, jy, jwts = _weights(sx, sy, win)
        if jx < 0 or jy < 0 or jx + w + 1 > W or jy + h + 1 > H:
            continue
        gx = _interp(g[..., 0], ix, iy, win, wts, 8192, 14)
        d = _interp(f1.astype(np.int64), jx, jy, win, jwts, 256, 9) - _interp(f0.astype(np.int64), ix, iy, win, wts, 256, 9)
        out.append(_first_over(d * gx, _geo(win)[2]))
    return out


def _preconditions(oracle_mod, scene, win):
    tu, hwu, qw = _geo(win)
    units = win[1] * qw
    a = _a11_first(oracle_mod, scene, win)
    print(f"{scene} {win}: A11 lane prefixes first pass 2^24 at units {sorted(set(a), key=lambda v: (v is None, v))}")
    if scene in ("stripes", "checker"):
        assert all(v is not None and v < tu for v in a), a  # inside tile 0: the chains start there
    elif scene == "half":
        assert all(v is not None and v >= tu for v in a), a  # in a later tile
        if units > hwu:
            assert all(v >= hwu for v in a), a  # in a later half wave: the chains start mid-window
    else:
        b = _b_first_exact(oracle_mod, scene, win)
        print(f"{scene} {win}: first-iteration b lane prefixes first leave 2^24 at units "
              f"{sorted(set(b), key=lambda v: (v is None, v))} ({len(b)} points)")
        assert len(b) >= NPTS // 2 and all(v is not None for v in b), b
        # the ordered b chains run from that unit's half wave to the window's end: several tiles
        assert all((units - 1) // tu - (v // hwu) * (hwu // tu) + 1 >= 2 for v in b), b


def test_windows_and_levels():
    L = _lib.load()
    assert all(L.psn_lk_effective_max_level(W, H, w, h, ML) == 0 for w, h in FW_WINDOWS)  # one level a call
    assert [h * (w // 4) for w, h in WINDOWS] == [2560, 2240, 2064, 1024, 256, 144]
    assert all(w % 8 == 0 for w, _ in WINDOWS)


@pytest.mark.parametrize("win", FW_WINDOWS)
@pytest.mark.parametrize("scene", SCENES)
def test_forward_entry_tile_step(oracle_mod, scene, win):
    _preconditions(oracle_mod, scene, win)
    ref = _ref(oracle_mod, scene, win)
    for poison in (0, 1):
        fw, names, entries = _run(scene, win, poison_lds=poison)
        assert names == {BX} and entries == {FW}, (names, entries)  # the planner's choice: the forward entry
        bx, names, entries = _run(scene, win, poison_lds=poison, fw=1)
        assert names == {BX} and entries == {BX}, (names, entries)
        _same_bits(fw, ref, f"{scene} {win} poison {poison} forward entry vs oracle")
        _same_bits(bx, ref, f"{scene} {win} poison {poison} lk_kernel_bx vs oracle")
        _same_bits(fw, bx, f"{scene} {win} poison {poison} forward entry vs lk_kernel_bx")


@pytest.mark.parametrize("win", TW_WINDOWS)
@pytest.mark.parametrize("scene", SCENES)
def test_two_wave_tile_step(oracle_mod, scene, win):
    _preconditions(oracle_mod, scene, win)
    ref = _ref(oracle_mod, scene, win)
    for poison in (0, 1):
        two, names, _ = _run(scene, win, poison_lds=poison, bx_waves=2, box=2)
        assert names == {TWO_WAVE}, names
        _same_bits(two, ref, f"{scene} {win} poison {poison} two-wave vs oracle")
