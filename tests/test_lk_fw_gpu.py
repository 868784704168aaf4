"""The forward entry of the box kernel (lk_kernel_fw<10, true>) against the CPU
oracle and against lk_kernel_bx<10, true> of the same call (variant fw=1), bit for
bit: next, status, err.

320 x 240 frames at maxLevel 2, 40 points a case (the cost is per point). Every
window is taller than half the frame, so calcOpticalFlowPyrLK's level rule leaves
level 0 as the only level of these calls (asserted below): "every level" is that
one. Two image pairs. The low-contrast pair is a synthetic scene squeezed round mid grey: every
sum is an exact integer and nothing falls back. The full-contrast pair is two
uncorrelated binary-noise images, damped to a twentieth in the upper left part:
the A sums pass 2^24 (ordered A chains at the call's level), and the b chains leave
the exact range in the first half wave's units for windows in the right half and
only in a later half wave's for windows that start in the damped part (the
ordered b chains start at half wave 0 and later). The A precondition is the
oracle's integer gradients summed per lane; the b precondition is an estimate in
float64 at the position the oracle ends on, with a factor of 4 to either side of
2^24 -- not the kernel's own per-half-wave verdict, which also fails a half wave on
its threads' max |d| x max |g| bound. The points of the full-contrast pair
include windows across every image border (reflected patch rows, masked units).
"""
import functools

import numpy as np
import pytest

from lk_window_sums import lane_sums as _lane_sums
from lk_window_sums import window_grads as _window_grads
from mcmtt_opticalflow_amd import _lib
from mcmtt_opticalflow_amd import lk as glk
from mcmtt_opticalflow_amd import synth
from mcmtt_opticalflow_amd._lib import GET_MIN_EIGENVALS

pytestmark = pytest.mark.gpu

W, H, ML = 320, 240, 2
FW, BX = "lk_kernel_fw<10, true>", "lk_kernel_bx<10, true>"
# window -> units of 4 px (all w % 8 == 0: no scalar tail)
WINDOWS = [(64, 132),  # 2,112: just above 2,048 -- idle trailing threads
           (40, 232),  # 2,320: 7.25 half-wave tiles -- a partial last tile and its pad
           (72, 136),  # 2,448
           (64, 160)]  # 2,560: exactly full
HALF_WAVE_UNITS = 32 * 10  # exactness is decided per half wave: 32 threads x 10 units
BORDER = np.array([[3, 4], [316.5, 237.25], [-20, 100], [160, 239.5], [300, -30], [30, 120], [290, 118.5]], np.float32)
LOW_CONTRAST_DIV = 4
EXACT = 1 << 24
CRIT_FULL = (1, 3, 0.0)  # three iterations on uncorrelated frames
# the full-contrast pair: binary noise, damped in the upper left part of the image (every
# window's first 32 rows there: the first half wave's units)
LOW_BAND_ROWS, LOW_BAND_CONTRAST = 90, 0.05


@functools.lru_cache(maxsize=None)
def _pair(kind):
    if kind == "low":
        sc = synth.make_scene(2, W, H, 40)
        f0, f1 = [(128 + (f.astype(np.int32) - 128) // LOW_CONTRAST_DIV).astype(np.uint8) for f in (sc.frame(0), sc.frame(1))]
        pts = sc.points_at(0)[:40]
    else:
        rng = np.random.default_rng(31)
        contrast = np.ones((H, W))
        contrast[:LOW_BAND_ROWS, :W // 2] = LOW_BAND_CONTRAST
        f0, f1 = [(128 + contrast * (254 * rng.integers(0, 2, (H, W)) - 127)).astype(np.uint8) for _ in range(2)]
        # windows of every size inside the image (centre rows 117 - 121): left of the middle
        # column they start in the low band, right of it in full contrast, some straddle it
        xs = np.concatenate([rng.uniform(45, 120, 12), rng.uniform(200, 275, 12), rng.uniform(125, 195, 9)])
        inner = np.stack([xs, rng.uniform(117, 121, 33)], 1).astype(np.float32)
        pts = np.concatenate([inner, BORDER])
    for a in (f0, f1, pts):
        a.setflags(write=False)
    return f0, f1, pts


def _crit(kind):
    return CRIT_FULL if kind == "full" else (3, 30, 0.01)


_REFS = {}


def _ref(oracle_mod, kind, win, flags=0):
    """The oracle's result of one case, computed once."""
    if (kind, win, flags) not in _REFS:
        f0, f1, pts = _pair(kind)
        r = oracle_mod.calc_optical_flow_pyr_lk(f0, f1, pts, win, ML, criteria=_crit(kind), flags=flags)
        for a in r:
            a.setflags(write=False)
        _REFS[kind, win, flags] = r
    return _REFS[kind, win, flags]


def _run(kind, win, fw, flags=0, **env):
    """One call on the GPU with variant fw=`fw` (None: the planner): (next, status,
    err), the names of the kernels (psn_lk_timing_launches: the build) and of the
    entries (psn_lk_timing_entries) of its launches."""
    f0, f1, pts = _pair(kind)
    variants = dict(env)
    if fw is not None:
        variants["fw"] = fw
    L = _lib.load()
    with glk.LKContext(W, H, ring_slots=1, max_level_cap=ML, variants=variants) as ctx:
        ctx.enable_timing(4, 1)
        out = ctx.calc_optical_flow_pyr_lk(f0, f1, pts, win, ML, criteria=_crit(kind), flags=flags)
        ctx.sync()
        names = {_lib.kernel_of_tag(t) for _, t in _lib.timing_launches(L, ctx.handle, 4)}
        entries = {_lib.kernel_of_tag(t) for t in _lib.timing_entries(L, ctx.handle, 4)}
    return out, names, entries


def _same_bits(a, b, what):
    for x, y, n in zip(a, b, ("next", "status", "err")):
        assert x.tobytes() == y.tobytes(), f"{what}: {n} differs"


def _check(oracle_mod, kind, win, flags=0, **env):
    ref = _ref(oracle_mod, kind, win, flags)
    fw, names, entries = _run(kind, win, None, flags, **env)
    assert names == {BX} and entries == {FW}, (names, entries)  # the planner's choice: the build's tag, the forward entry
    bx, names, entries = _run(kind, win, 1, flags, **env)
    assert names == {BX} and entries == {BX}, (names, entries)
    _same_bits(fw, ref, f"{kind} {win} flags {flags} {env} forward entry vs oracle")
    _same_bits(bx, ref, f"{kind} {win} flags {flags} {env} lk_kernel_bx vs oracle")
    _same_bits(fw, bx, f"{kind} {win} flags {flags} {env} forward entry vs lk_kernel_bx")
    return ref


def _bilinear(img, x0, y0, w, h):
    """img (2-D) sampled at (x0 + i, y0 + j), i < w, j < h, float64 (edge-padded)."""
    pad = max(w, h) + 40
    p = np.pad(img.astype(np.float64), pad, mode="edge")
    ix, iy = int(np.floor(x0)), int(np.floor(y0))
    a, b = x0 - ix, y0 - iy
    r = p[iy + pad:iy + pad + h + 1, ix + pad:ix + pad + w + 1]
    return (1 - a) * (1 - b) * r[:-1, :-1] + a * (1 - b) * r[:-1, 1:] + (1 - a) * b * r[1:, :-1] + a * b * r[1:, 1:]


def _b_first_half_waves(oracle_mod, win):
    """Of the interior points of the full-contrast pair, with a window inside the
    image: how many b chains (lane x & 3 of sum (J - I) * 32 * Ix, row-major, at the
    position the oracle ends on) pass 4 x 2^24 within the first half wave's units,
    and how many stay below 2^24 / 4 there and pass 4 x 2^24 in a later one. The
    margins of 4: the iterations' positions are within an update of the last one,
    and the prefixes of uncorrelated frames do not depend on the position. A lane
    chain takes one term per unit, so a prefix's length is its unit count."""
    w, h = win
    f0, f1, pts = _pair("full")
    ref = _ref(oracle_mod, "full", win)
    at0 = later = 0
    for (x, y), (nx, ny), ok in zip(pts[:-len(BORDER)], ref[0], ref[1]):
        ox, oy = float(x) - (w - 1) * 0.5, float(y) - (h - 1) * 0.5
        if not ok or ox < 1 or oy < 1 or ox + w > W - 2 or oy + h > H - 2:
            continue
        gx, _ = _window_grads(oracle_mod, f0, x, y, win)
        d = 32.0 * (_bilinear(f1, float(nx) - (w - 1) * 0.5, float(ny) - (h - 1) * 0.5, w, h) - _bilinear(f0, ox, oy, w, h))
        t = d * gx
        pre = np.max([np.abs(np.cumsum(t[:, l::4].ravel())) for l in range(4)], axis=0)  # per unit count, worst lane
        head, tail = pre[:HALF_WAVE_UNITS].max(), pre[HALF_WAVE_UNITS:].max()
        at0 += head > 4 * EXACT
        later += head < EXACT / 4 and tail > 4 * EXACT
    return at0, later


def test_windows_are_the_forward_entrys():
    L = _lib.load()
    assert all(L.psn_lk_effective_max_level(W, H, w, h, ML) == 0 for w, h in WINDOWS)  # one level a call
    units = [h * (w // 4) for w, h in WINDOWS]
    assert units == [2112, 2320, 2448, 2560] and all(w % 8 == 0 and 2048 < u <= 2560 for (w, _), u in zip(WINDOWS, units))
    assert units[1] % HALF_WAVE_UNITS != 0 and units[3] == 8 * HALF_WAVE_UNITS  # a partial last tile; exactly full


@pytest.mark.parametrize("win", WINDOWS)
def test_fw_low_contrast_exact_path(oracle_mod, win):
    """Every per-lane sum of Ix^2, Iy^2 and |Ix Iy| stays below 2^24 at level 0: the
    integer sums are the float sums, nothing falls back."""
    f0, _, pts = _pair("low")
    s = _lane_sums(oracle_mod, f0, pts, win)
    print(f"low {win}: max per-lane sums {s.max(axis=0)} = {s.max() / EXACT:.3f} x 2^24")
    assert s.max() < EXACT
    ref = _check(oracle_mod, "low", win)
    assert ref[1].sum() >= 24


@pytest.mark.parametrize("win", WINDOWS)
def test_fw_full_contrast_fallbacks(oracle_mod, win):
    """The ordered A chains (the largest per-lane sum of Ix^2 passes 2^24 for 36 of the
    40 points at the least: all but windows that are mostly outside the image)
    and the ordered b chains from half wave 0 and from later half waves; windows
    across the image borders among the points."""
    f0, _, pts = _pair("full")
    s = _lane_sums(oracle_mod, f0, pts, win)
    at0, later = _b_first_half_waves(oracle_mod, win)
    print(f"full {win}: max per-lane sum Ix^2 above 2^24 for {(s[:, 0] > EXACT).sum()} of {len(s)} points; "
          f"b chains leaving the exact range in half wave 0: {at0} points, only later: {later}")
    assert (s[:, 0] > EXACT).sum() >= 36
    assert at0 >= 6 and later >= 6
    ref = _check(oracle_mod, "full", win)
    assert ref[1].sum() >= 12


def test_fw_unwritten_lds_never_read(oracle_mod):
    """LDS filled with pseudo-random words first (PSN_LK_VARIANT_POISON_LDS): the
    partial last tile's pad and the ends of the planes."""
    _check(oracle_mod, "full", (40, 232), poison_lds=1)


def test_fw_min_eigenvals(oracle_mod):
    """GET_MIN_EIGENVALS: err is the minimum eigenvalue, no err pass (every other case
    runs without the flag, so with the err pass)."""
    _check(oracle_mod, "full", (64, 160), flags=GET_MIN_EIGENVALS)


def test_fw_mixed_call(oracle_mod):
    """A 64 x 160 query beside a 64 x 64 query in one call, as Tracker2D's forward and
    backward windows: one launch each. The forward query holds the most window
    pixels, so the call's tags name its launch."""
    f0, f1, pts = _pair("full")
    n = len(pts)
    specs = [((64, 160), n), ((64, 64), n)]
    allpts = np.concatenate([pts, pts])
    L = _lib.load()
    got = {}
    for fw, entry in ((None, "mixed:" + FW), (1, "mixed:" + BX)):
        with glk.LKContext(W, H, ring_slots=2, max_level_cap=ML, variants={} if fw is None else {"fw": fw}) as ctx:
            ctx.push_frame(0, f0)
            ctx.push_frame(1, f1)
            qs = [glk.make_query(0, 1, k * n, m, glk.make_params(win, ML, criteria=CRIT_FULL)) for k, (win, m) in enumerate(specs)]
            ctx.enable_timing(4, 1)
            got[fw] = ctx.track(qs, allpts)
            ctx.sync()
            names = {_lib.kernel_of_tag(t) for _, t in _lib.timing_launches(L, ctx.handle, 4)}
            entries = {_lib.kernel_of_tag(t) for t in _lib.timing_entries(L, ctx.handle, 4)}
        assert names == {"mixed:" + BX} and entries == {entry}, (names, entries)
    for k, (win, m) in enumerate(specs):
        sl = slice(k * n, k * n + m)
        _same_bits(tuple(a[sl] for a in got[None]), _ref(oracle_mod, "full", win), f"mixed {win}")
        _same_bits(tuple(a[sl] for a in got[None]), tuple(a[sl] for a in got[1]), f"mixed {win} vs lk_kernel_bx")
