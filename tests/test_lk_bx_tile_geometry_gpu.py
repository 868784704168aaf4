"""The fallback tile geometry of the no-tail box builds (lk_kernel_bx<UPT, true>:
the tile's chain slots from its unit range, csrc/psn_lk_kernels.h bx_tile_slots_nt)
against the CPU oracle, bit for bit, one window set per build.

640 x 480 frames with maxLevel 3, about 48 scene points plus border points. Two
image pairs: the full-contrast synthetic scene, whose A sums pass 2^24 (the
ordered chains run over every tile up to the window's last, the only one with a
pad), and a low-contrast copy of it that stays on the exact path. Both are
asserted as preconditions on the oracle's Scharr gradients. The windows vary the
last tile's length (printed per case, in 16-float blocks, from the plan
arithmetic); a tail build keeps the general formula and runs beside them.
"""
import functools

import numpy as np
import pytest

from mcmtt_opticalflow_amd import _lib
from mcmtt_opticalflow_amd import lk as glk
from mcmtt_opticalflow_amd import synth

pytestmark = pytest.mark.gpu

W, H, ML = 640, 480, 3
TWO_WAVE = "lk_kernel_bx<8, true, 128>"
# (window, variant bx_waves or None: the planner, kernel, units per thread, tile threads)
CASES = [((64, 64), None, TWO_WAVE, 8, 16),
         ((40, 50), None, TWO_WAVE, 8, 16),
         ((40, 32), None, TWO_WAVE, 8, 16),
         ((16, 72), None, TWO_WAVE, 8, 16),
         ((64, 100), None, "lk_kernel_bx<8, true>", 8, 32),
         ((64, 136), None, "lk_kernel_bx<10, true>", 10, 32),
         ((56, 152), None, "lk_kernel_bx<10, true>", 10, 32),
         ((64, 64), 4, "lk_kernel_bx<4, true>", 4, 32),
         ((44, 40), None, "lk_kernel_bx<4, false>", 4, 32)]  # a tail build: 44 % 8
IDS = [f"{w}x{h}-{k.split('<')[1].rstrip('>').replace(', ', '_')}" for (w, h), _, k, _, _ in CASES]
POISON = [CASES[i] for i in (1, 4, 6, 7, 8)]  # one window per build
BORDER = np.array([[3, 4], [636.5, 477.25], [-20, 200], [320, 479.5]], np.float32)
LOW_CONTRAST_DIV = 4  # the low-contrast pair: 128 + (frame - 128) / 4
EXACT = 1 << 24


@functools.lru_cache(maxsize=None)
def _pair(kind):
    sc = synth.make_scene(2, W, H, 48)
    f0, f1 = sc.frame(0), sc.frame(1)
    if kind == "low":
        f0, f1 = [(128 + (f.astype(np.int32) - 128) // LOW_CONTRAST_DIV).astype(np.uint8) for f in (f0, f1)]
    pts = np.concatenate([sc.points_at(0), BORDER])
    for a in (f0, f1, pts):
        a.setflags(write=False)
    return f0, f1, pts


_REFS = {}


def _ref(oracle_mod, kind, win):
    """The oracle's result of one case, computed once."""
    if (kind, win) not in _REFS:
        f0, f1, pts = _pair(kind)
        r = oracle_mod.calc_optical_flow_pyr_lk(f0, f1, pts, win, ML)
        for a in r:
            a.setflags(write=False)
        _REFS[kind, win] = r
    return _REFS[kind, win]


def _run(kind, win, waves, **env):
    f0, f1, pts = _pair(kind)
    variants = dict(env)
    if waves is not None:
        variants["bx_waves"] = waves
    L = _lib.load()
    with glk.LKContext(W, H, ring_slots=1, max_level_cap=ML, variants=variants) as ctx:
        ctx.enable_timing(4, 1)
        out = ctx.calc_optical_flow_pyr_lk(f0, f1, pts, win, ML)
        ctx.sync()
        names = {_lib.kernel_of_tag(t) for _, t in _lib.timing_launches(L, ctx.handle, 4)}
    return out, names


def _check(oracle_mod, kind, case, **env):
    win, waves, kern, _, _ = case
    ref = _ref(oracle_mod, kind, win)
    out, names = _run(kind, win, waves, **env)
    assert names == {kern}, names
    for x, y, n in zip(out, ref, ("next", "status", "err")):
        assert x.tobytes() == y.tobytes(), f"{kind} {win} {kern} {env}: {n} differs from the oracle"
    return ref


def _last_tile(case):
    """(tiles, units of the last tile, its 16-float blocks, blocks of a full tile):
    the window's units of 4 px row-major, tiles of `tile threads x units per
    thread` units (one half-wave / quarter-wave granule per tile at these sizes)."""
    (w, h), _, _, upt, tg = case
    units, tile = h * ((w + 3) // 4), tg * upt
    g_last = (units - 1) // tile
    last = units - g_last * tile
    return g_last + 1, last, (last + 15) // 16, tile // 16


def _lane_sums(oracle_mod, img, pts, win):
    """Per point the largest per-lane (x & 3) sum of Ix^2, of Iy^2 and of |Ix Iy|
    over the level-0 window: the oracle's Scharr gradients, interpolated with the
    window's 14-bit bilinear weights as calcOpticalFlowPyrLK does (edge-padded)."""
    w, h = win
    pad = max(w, h) + 32
    g = np.pad(oracle_mod.scharr(img).astype(np.int64), ((pad, pad), (pad, pad), (0, 0)), mode="edge")
    out = []
    for x, y in pts:
        px = np.float32(x) - np.float32((w - 1) * 0.5)
        py = np.float32(y) - np.float32((h - 1) * 0.5)
        ix, iy = int(np.floor(px)), int(np.floor(py))
        if ix < -w or iy < -h or ix > W or iy > H:
            continue  # the window is outside the image: status 0, no sums
        a, b = float(px - np.float32(ix)), float(py - np.float32(iy))
        w00, w01, w10 = round((1 - a) * (1 - b) * 16384), round(a * (1 - b) * 16384), round((1 - a) * b * 16384)
        w11 = 16384 - w00 - w01 - w10
        r = g[iy + pad:iy + pad + h + 1, ix + pad:ix + pad + w + 1]
        v = (r[:-1, :-1] * w00 + r[:-1, 1:] * w01 + r[1:, :-1] * w10 + r[1:, 1:] * w11 + 8192) >> 14
        gx, gy = v[..., 0], v[..., 1]
        out.append([max(int(t[:, l::4].sum()) for l in range(4)) for t in (gx * gx, gy * gy, np.abs(gx * gy))])
    return np.array(out, np.int64)


def test_windows_vary_the_last_tile():
    """The no-tail cases hold a full last tile, a padded one (its length no multiple
    of 16) and short ones; a full tile is whole blocks in every build."""
    seen = []
    for case in CASES[:-1]:
        tiles, last, blocks, full = _last_tile(case)
        print(f"{case[0]} {case[2]}: {tiles} tiles, last {last} units = {blocks} of {full} blocks, pad {-last % 16}")
        assert (case[3] * case[4]) % 16 == 0 and 1 <= blocks <= full
        seen.append((blocks == full, last % 16 != 0, blocks < full, blocks % 2 == 1))
    assert all(any(s[i] for s in seen) for i in range(4)), seen


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_full_contrast_ordered_chains(oracle_mod, case):
    """The full-contrast scene: the largest per-lane sum of Ix^2 of the windows
    passes 2^24, so the ordered A chains run over the tiles."""
    f0, _, pts = _pair("full")
    s = _lane_sums(oracle_mod, f0, pts, case[0])
    print(f"full {case[0]}: max per-lane sum Ix^2 {s[:, 0].max() / EXACT:.2f} x 2^24; last tile {_last_tile(case)}")
    assert s[:, 0].max() > EXACT
    ref = _check(oracle_mod, "full", case)
    assert ref[1].sum() >= 24


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_low_contrast_exact_path(oracle_mod, case):
    """The low-contrast pair: every per-lane sum of Ix^2, Iy^2 and |Ix Iy| of every
    window stays below 2^24 at level 0 (the integer sums ARE the float sums)."""
    f0, _, pts = _pair("low")
    s = _lane_sums(oracle_mod, f0, pts, case[0])
    print(f"low {case[0]}: max per-lane sums {s.max() / EXACT:.3f} x 2^24")
    assert s.max() < EXACT
    _check(oracle_mod, "low", case)


@pytest.mark.parametrize("case", POISON, ids=[IDS[CASES.index(c)] for c in POISON])
def test_unwritten_lds_never_read(oracle_mod, case):
    """LDS filled with pseudo-random words first: a full tile's chain regions have
    no pad to zero, the last tile's pad is zeroed by its chain lanes."""
    _check(oracle_mod, "full", case, poison_lds=1)
