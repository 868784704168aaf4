"""The two-wave build of the box kernel (lk_kernel_bx<8, true, 128>: 128 threads,
8 units per thread, quarter-wave fallback tiles) against the CPU oracle, bit for
bit, and against the four-wave builds of the same call (variant bx_waves=4).

640 x 480 frames with maxLevel 3, about 48 scene points plus border points. Two
image pairs: the full-contrast synthetic scene, whose A sums pass 2^24 (the
ordered chains run), and a low-contrast copy of it that stays on the exact path.
Both are asserted as preconditions on the oracle's Scharr gradients.
"""
import functools

import numpy as np
import pytest

from mcmtt_opticalflow_amd import _lib
from mcmtt_opticalflow_amd import lk as glk
from mcmtt_opticalflow_amd import synth
from mcmtt_opticalflow_amd._lib import ACCUM_SCALAR, GET_MIN_EIGENVALS, USE_INITIAL_FLOW

pytestmark = pytest.mark.gpu

W, H, ML = 640, 480, 3
TWO_WAVE = "lk_kernel_bx<8, true, 128>"
# window -> units of 4 px (all w % 8 == 0, above 1,024 px, at most 1,024 units)
WINDOWS = [(64, 64),   # 1,024: the headline window, full
           (32, 128),  # 1,024: 8 quads per row
           (72, 56),   # 1,008: a thread's units straddle rows
           (40, 50),   # 500: the last thread is partial, wave 1 almost empty
           (40, 32),   # 320: wave 1 entirely idle
           (16, 72)]   # 288: 4 quads per row
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


def _ref(oracle_mod, kind, win, flags=0, criteria=(3, 30, 0.01), next_pts=None):
    """The oracle's result of one case, computed once."""
    key = (kind, win, flags, criteria, next_pts is not None)
    if key not in _REFS:
        f0, f1, pts = _pair(kind)
        accum = oracle_mod.ACCUM_SCALAR if flags & ACCUM_SCALAR else oracle_mod.ACCUM_SSE2
        r = oracle_mod.calc_optical_flow_pyr_lk(f0, f1, pts, win, ML, criteria=criteria, flags=flags & ~ACCUM_SCALAR,
                                                accum=accum, next_pts=next_pts)
        for a in r:
            a.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def _run(kind, win, waves, flags=0, criteria=(3, 30, 0.01), next_pts=None, **env):
    """One call on the GPU with variant bx_waves=`waves` (None: the planner):
    (next, status, err), the kernel names of its launches."""
    f0, f1, pts = _pair(kind)
    variants = dict(env)
    if waves is not None:
        variants["bx_waves"] = waves
    L = _lib.load()
    with glk.LKContext(W, H, ring_slots=1, max_level_cap=ML, variants=variants) as ctx:
        ctx.enable_timing(4, 1)
        out = ctx.calc_optical_flow_pyr_lk(f0, f1, pts, win, ML, criteria=criteria, flags=flags, next_pts=next_pts)
        ctx.sync()
        names = {_lib.kernel_of_tag(t) for _, t in _lib.timing_launches(L, ctx.handle, 4)}
    return out, names


def _same_bits(a, b, what):
    for x, y, n in zip(a, b, ("next", "status", "err")):
        assert x.tobytes() == y.tobytes(), f"{what}: {n} differs"


def _check(oracle_mod, kind, win, **kw):
    env = {k: kw.pop(k) for k in list(kw) if k in _lib.VARIANTS}
    ref = _ref(oracle_mod, kind, win, **kw)
    two, n2 = _run(kind, win, 2, **kw, **env)
    four, n4 = _run(kind, win, 4, **kw, **env)
    assert n2 == {TWO_WAVE}, n2
    assert n4 == {"lk_kernel_bx<4, true>"}, n4
    _same_bits(two, ref, f"{kind} {win} {kw} {env} two-wave vs oracle")
    _same_bits(two, four, f"{kind} {win} {kw} {env} two-wave vs four-wave")
    return ref


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


@pytest.mark.parametrize("win", WINDOWS)
def test_two_wave_full_contrast(oracle_mod, win):
    """The full-contrast scene: the largest per-lane sum of Ix^2 of the windows
    passes 2^24, so the ordered A chains (quarter-wave tiles) run."""
    f0, _, pts = _pair("full")
    s = _lane_sums(oracle_mod, f0, pts, win)
    print(f"full {win}: max per-lane sum Ix^2 {s[:, 0].max()} = {s[:, 0].max() / EXACT:.2f} x 2^24")
    assert s[:, 0].max() > EXACT
    ref = _check(oracle_mod, "full", win)
    assert ref[1].sum() >= 24


@pytest.mark.parametrize("win", WINDOWS)
def test_two_wave_low_contrast_exact_path(oracle_mod, win):
    """The low-contrast pair: every per-lane sum of Ix^2, Iy^2 and |Ix Iy| of
    every window stays below 2^24 at level 0 (the integer sums ARE the float sums)."""
    f0, _, pts = _pair("low")
    s = _lane_sums(oracle_mod, f0, pts, win)
    print(f"low {win}: max per-lane sums {s.max(axis=0)} = {s.max() / EXACT:.3f} x 2^24")
    assert s.max() < EXACT
    _check(oracle_mod, "low", win)


@pytest.mark.parametrize("win,flags,kern", [((44, 40), 0, "lk_kernel_bx<4, false>"),             # a tail: 44 % 8
                                            ((64, 64), ACCUM_SCALAR, "lk_kernel_bx<4, false>"),  # the scalar order
                                            ((64, 160), 0, "lk_kernel_bx<10, true>")])           # the forward window
@pytest.mark.parametrize("waves", [None, 2])
def test_four_wave_builds_keep_their_windows(oracle_mod, win, flags, kern, waves):
    """Windows the two-wave build does not take name their four-wave builds, under
    the planner and under bx_waves=2 alike."""
    out, names = _run("full", win, waves, flags=flags)
    assert names == {kern}, names
    _same_bits(out, _ref(oracle_mod, "full", win, flags=flags), f"{win} flags {flags} waves {waves}")
    four, n4 = _run("full", win, 4, flags=flags)
    assert n4 == {kern}, n4
    _same_bits(out, four, f"{win} flags {flags} waves {waves} vs bx_waves=4")


def test_two_wave_min_eigenvals(oracle_mod):
    _check(oracle_mod, "full", (64, 64), flags=GET_MIN_EIGENVALS)


def test_two_wave_initial_flow(oracle_mod):
    _, _, pts = _pair("full")
    guess = (pts + np.float32([1.5, -0.75])).astype(np.float32)
    guess.setflags(write=False)
    for win in [(64, 64), (40, 50)]:
        _check(oracle_mod, "full", win, flags=USE_INITIAL_FLOW, next_pts=guess)


@pytest.mark.parametrize("criteria", [(2, 30, 0.05),   # ends on epsilon
                                      (1, 3, 0.01)])   # ends on the count
def test_two_wave_criteria(oracle_mod, criteria):
    for win in [(64, 64), (72, 56)]:
        _check(oracle_mod, "full", win, criteria=criteria)


@pytest.mark.parametrize("win", [(64, 64), (40, 50)])
@pytest.mark.parametrize("kind", ["full", "low"])
def test_two_wave_unwritten_lds_never_read(oracle_mod, kind, win):
    """LDS filled with pseudo-random words first: the absent waves' record slots,
    the quarter-wave tiles' pads and ends, the J region."""
    _check(oracle_mod, kind, win, poison_lds=1)


def _bilinear(img, x0, y0, w, h):
    """img (2-D, any integer type) sampled at (x0 + i, y0 + j), i < w, j < h, float64."""
    ix, iy = int(np.floor(x0)), int(np.floor(y0))
    a, b = x0 - ix, y0 - iy
    r = img[iy:iy + h + 1, ix:ix + w + 1].astype(np.float64)
    return (1 - a) * (1 - b) * r[:-1, :-1] + a * (1 - b) * r[:-1, 1:] + (1 - a) * b * r[1:, :-1] + a * b * r[1:, 1:]


@pytest.mark.parametrize("win", [(64, 64), (40, 50)])
def test_two_wave_ordered_b_chains(oracle_mod, win):
    """Uncorrelated frames: the b sums leave the exact range, so the iterations take
    the ordered b chains -- the quarter-wave b writer with its transposed J offsets.
    Precondition, from the oracle's gradients and its own result: at the position
    the oracle ends on, the largest |prefix| of a lane chain (x & 3, row-major) of
    sum (J - I) * 32 * Ix passes 4 x 2^24 for most points (a margin of 4: the last
    iteration's position is within one update of that one, and the prefixes of
    uncorrelated frames do not depend on the position)."""
    w, h = win
    rng = np.random.default_rng(23)
    f0 = rng.integers(0, 256, (H, W), dtype=np.uint8)
    f1 = rng.integers(0, 256, (H, W), dtype=np.uint8)
    pts = rng.uniform(150, 330, (24, 2)).astype(np.float32)
    crit = (1, 3, 0.0)
    ref = oracle_mod.calc_optical_flow_pyr_lk(f0, f1, pts, win, 1, criteria=crit)
    gxy = oracle_mod.scharr(f0).astype(np.int64)
    big = 0
    for (x, y), (nx, ny), ok in zip(pts, ref[0], ref[1]):
        if not ok:
            continue
        ox, oy = float(x) - (w - 1) * 0.5, float(y) - (h - 1) * 0.5
        d = 32.0 * (_bilinear(f1, float(nx) - (w - 1) * 0.5, float(ny) - (h - 1) * 0.5, w, h) - _bilinear(f0, ox, oy, w, h))
        t = d * _bilinear(gxy[..., 0], ox, oy, w, h)
        worst = max(np.abs(np.cumsum(t[:, l::4].ravel())).max() for l in range(4))
        big += worst > 4 * EXACT
    print(f"ordered b {win}: {big} of {int(ref[1].sum())} tracked points pass 4 x 2^24")
    assert ref[1].sum() >= 12 and 2 * big > ref[1].sum()
    L = _lib.load()
    got = {}
    for waves, kern in ((2, TWO_WAVE), (4, "lk_kernel_bx<4, true>")):
        with glk.LKContext(W, H, ring_slots=1, max_level_cap=1, variants={"bx_waves": waves, "poison_lds": 1}) as ctx:
            ctx.enable_timing(4, 1)
            got[waves] = ctx.calc_optical_flow_pyr_lk(f0, f1, pts, win, 1, criteria=crit)
            ctx.sync()
            names = {_lib.kernel_of_tag(t) for _, t in _lib.timing_launches(L, ctx.handle, 4)}
        assert names == {kern}, names
    _same_bits(got[2], ref, f"ordered b {win} two-wave vs oracle")
    _same_bits(got[2], got[4], f"ordered b {win} two-wave vs four-wave")


@pytest.mark.parametrize("stride", [1, 3])
def test_two_wave_merged_counted_queries(oracle_mod, stride):
    """Counted queries of two-wave windows (more than a launch's table of 32)
    merge into sub-queries: blocks of 12-point capacity 16 points apart, device
    counts 0..12 at stride `stride`, a window change and an empty query in the
    middle. Points inside a count carry the oracle's bits, the rest stay untouched;
    the same call with bx_waves=4 writes the same bytes."""
    import hiprt

    CAP, GAP = 12, 16
    wins = [(64, 64)] * 22 + [(40, 50)] * 18
    nq = len(wins)
    sc = synth.make_scene(7, W, H, GAP * nq)
    f0, f1, pts = sc.frame(0), sc.frame(1), sc.points_at(0)[:GAP * nq]
    rng = np.random.default_rng(5)
    counts = rng.integers(0, CAP + 1, nq).astype(np.int32)
    counts[[3, 21, 39]] = [0, CAP, CAP]
    dc = np.zeros(nq * stride, np.int32)
    dc[::stride] = counts
    sentinel = np.full(pts.shape, -7.0, np.float32)
    qs = [glk.make_query(0, 1, GAP * i, CAP if i != 30 else 0, glk.make_params(w, ML)) for i, w in enumerate(wins)]
    L = _lib.load()
    got = {}
    for waves, kern in ((2, TWO_WAVE), (4, "lk_kernel_bx<4, true>")):
        d_p, d_n = hiprt.DeviceBuffer.from_array(pts), hiprt.DeviceBuffer.from_array(sentinel)
        d_s, d_e = hiprt.DeviceBuffer.from_array(np.full(len(pts), 9, np.uint8)), hiprt.DeviceBuffer(4 * len(pts))
        d_c = hiprt.DeviceBuffer.from_array(dc)
        with glk.LKContext(W, H, ring_slots=2, max_level_cap=ML, variants={"bx_waves": waves}) as ctx:
            ctx.push_frame(0, f0)
            ctx.push_frame(1, f1)
            ctx.enable_timing(4, 1)
            if stride == 1:
                ctx.track_device_counted(qs, d_c.addr, d_p.addr, d_n.addr, d_s.addr, d_e.addr)
            else:
                ctx.track_device_counted_strided(qs, d_c.addr, stride, d_p.addr, d_n.addr, d_s.addr, d_e.addr)
            ctx.sync()
            names = {_lib.kernel_of_tag(t) for _, t in _lib.timing_launches(L, ctx.handle, 4)}
        assert names == {kern}, names
        got[waves] = (d_n.to_array(pts.shape, np.float32), d_s.to_array(len(pts), np.uint8),
                      d_e.to_array(len(pts), np.float32))
    g_n, g_s, g_e = got[2]
    for i, (w, c) in enumerate(zip(wins, counts)):
        lo = GAP * i
        c = 0 if i == 30 else int(c)
        if c:
            ref = oracle_mod.calc_optical_flow_pyr_lk(f0, f1, pts[lo:lo + c], w, ML)
            _same_bits((g_n[lo:lo + c], g_s[lo:lo + c], g_e[lo:lo + c]), ref, f"query {i} {w}")
            _same_bits((g_n[lo:lo + c], g_s[lo:lo + c], g_e[lo:lo + c]),
                       tuple(a[lo:lo + c] for a in got[4]), f"query {i} {w} vs four-wave")
        np.testing.assert_array_equal(g_n[lo + c:lo + GAP], sentinel[lo + c:lo + GAP], f"query {i} untouched")
        assert (g_s[lo + c:lo + GAP] == 9).all(), i


def test_two_wave_mixed_call(oracle_mod):
    """One call holding two-wave windows, four-wave windows (a tail build and the
    forward window) and a single-tile window, as Tracker2D's calls mix them: one
    launch per class, every query the oracle's bits, the same under bx_waves=4.
    The two-wave queries hold the most window pixels of the call (the forward
    query takes 20 points), so the call's tag names their launch: the two-wave
    build under bx_waves=2, the 4-unit four-wave build under bx_waves=4."""
    f0, f1, pts = _pair("full")
    n = len(pts)
    specs = [((64, 64), n), ((44, 40), n), ((21, 21), n), ((64, 160), 20), ((40, 50), n)]
    px = {win: win[0] * win[1] * m for win, m in specs}
    assert px[(64, 64)] + px[(40, 50)] > max(px[(64, 160)], px[(44, 40)], px[(21, 21)])
    allpts = np.concatenate([pts[:m] for _, m in specs])
    first = np.concatenate([[0], np.cumsum([m for _, m in specs])])
    L = _lib.load()
    got = {}
    for waves, kern in ((2, "mixed:" + TWO_WAVE), (4, "mixed:lk_kernel_bx<4, true>")):
        with glk.LKContext(W, H, ring_slots=2, max_level_cap=ML, variants={"bx_waves": waves}) as ctx:
            ctx.push_frame(0, f0)
            ctx.push_frame(1, f1)
            qs = [glk.make_query(0, 1, int(first[k]), m, glk.make_params(win, ML)) for k, (win, m) in enumerate(specs)]
            ctx.enable_timing(4, 1)
            got[waves] = ctx.track(qs, allpts)
            ctx.sync()
            names = {_lib.kernel_of_tag(t) for _, t in _lib.timing_launches(L, ctx.handle, 4)}
        assert names == {kern}, names
    for k, (win, m) in enumerate(specs):
        sl = slice(int(first[k]), int(first[k]) + m)
        ref = tuple(a[:m] for a in _ref(oracle_mod, "full", win))
        _same_bits(tuple(a[sl] for a in got[2]), ref, f"mixed {win}")
        _same_bits(tuple(a[sl] for a in got[2]), tuple(a[sl] for a in got[4]), f"mixed {win} vs four-wave")
