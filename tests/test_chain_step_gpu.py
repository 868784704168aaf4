"""The backward-chain kernels (csrc/psn_t2d_chain.hip: chain_step_kernel,
chain_begin_kernel, gate_counts_kernel) through their C entry points
(include/psn_t2d_device.h) against tests/chain_ref.py, the plain model on top
of the oracle's LocalSearchKLT, bit for bit.

One chain_step workgroup is one detection, so a family of a few hundred
constructed inputs is one launch. Every output buffer is filled with a
sentinel before the launch and the model is applied to arrays poisoned alike:
a write outside what the header promises fails the comparison (floats and
doubles are compared through their integer views, so -0.0 and the sentinel's
NaN payload count). Stopped detections (cnt = 0) sit between the live ones and
every family runs a second time in reversed order, so a result that depends on
blockIdx or on a neighbour's row shows.

The families are built to hit their targets, and each asserts from the model
alone (test_family_coverage, no GPU) that it does:
  a  the four kinds of chain_ref.klt_case and the window-edge family the host
     twin psn_t2d_local_search_klt is held to (test_tracker2d.py), w <= 0 included
  b  exactly ceil(n/2) movers (the step runs) against ceil(n/2) - 1 (it stops),
     the movers first, last, interleaved or in lanes >= 64 only
  c  the inlier radius: vector pairs for which sqrt(ex*ex + ey*ey) differs between
     the unfused double sum and both fused forms, with the window placed on the
     root between them, so a contracted kernel keeps another inlier set; and
     the movement threshold 0.1 * scale: the float32 vectors whose norm is the
     threshold itself (ON_THRESHOLD: they exist at the scales 1.0 and 0.5) and
     vectors one float32 step to either side (_near_threshold)
  d  a cluster of exactly 3, 4 and 5 equal moves among scattered outliers
  e  two clusters of the same size (equal neighbour counts): the first maximum
     in sorted order wins; at n = cap the sort's +inf padding must not count
  f  families a and c at the scales 0.5, 0.75 and 0.3
  g  last_step 0..3 mixed in one launch
then begin + three steps with the device pass's buffer hand-over, begin and the
gate alone, and the argument checks."""
import ctypes
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import chain_ref
import tracker2d_oracle as ORC

ERR_ARG = -1
CAPS = (100, 128, 7)  # production (PSN_T2D_CHAIN_CAP), the kernel's lane count, a short row
SCALES = (0.5, 0.75, 0.3)


def counts(cap):
    return [n for n in (0, 1, 3, 4, 5, 31, 63, 64, 65, 99, 100, 127, 128) if n <= cap]


# ---------------------------------------------------------------------------
# The C ABI
# ---------------------------------------------------------------------------

class ChainDev(ctypes.Structure):  # psn_t2d_chain_dev
    _fields_ = [("ndet", ctypes.c_int), ("cap", ctypes.c_int), ("boxes", ctypes.c_void_p), ("cur", ctypes.c_void_p),
                ("nxt", ctypes.c_void_p), ("cnt", ctypes.c_void_p), ("next_in", ctypes.c_void_p),
                ("out_boxes", ctypes.c_void_p), ("sets", ctypes.c_void_p), ("set_cnt", ctypes.c_void_p),
                ("nsteps", ctypes.c_void_p), ("last_step", ctypes.c_void_p), ("scale", ctypes.c_double)]


def _api():
    from mcmtt_opticalflow_amd import _lib

    L = _lib.load()
    vp = ctypes.c_void_p
    L.psn_t2d_chain_step_device.argtypes = [ctypes.POINTER(ChainDev), ctypes.c_int, vp]
    L.psn_t2d_chain_begin_device.argtypes = [ctypes.POINTER(ChainDev), ctypes.c_int, vp]
    L.psn_t2d_gate_counts_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp]
    for f in (L.psn_t2d_chain_step_device, L.psn_t2d_chain_begin_device, L.psn_t2d_gate_counts_device):
        f.restype = ctypes.c_int
    return L


class DevChain:
    """The device copy of a ChainState and its point buffers."""

    def __init__(self, state, scale, **points):
        import hiprt

        self.h = hiprt
        self.state = state
        self.buf = {}
        for name in ("boxes", "cnt") + chain_ref.ChainState.OUTPUTS:
            self.buf[name] = hiprt.DeviceBuffer.from_array(getattr(state, name))
        if state.last_step is not None:
            self.buf["last_step"] = hiprt.DeviceBuffer.from_array(state.last_step)
        for name, a in points.items():
            self.buf[name] = hiprt.DeviceBuffer.from_array(np.ascontiguousarray(a, np.float32))
        self.c = ChainDev(ndet=state.ndet, cap=state.cap, scale=scale)
        for name in ("boxes", "cnt", "last_step") + chain_ref.ChainState.OUTPUTS:
            setattr(self.c, name, self.buf[name].addr if name in self.buf else None)

    def put(self, name, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes == self.buf[name].nbytes
        assert self.h.rt().hipMemcpy(self.buf[name].ptr, a.ctypes.data, a.nbytes, self.h.H2D) == 0, name

    def get(self, next_in="next_in"):
        """The counts and every output buffer as a ChainState (next_in from the named buffer)."""
        s = self.state
        out = chain_ref.ChainState(s.ndet, s.cap, s.boxes, self.buf["cnt"].to_array(s.cnt.shape, np.int32), s.last_step)
        for name in chain_ref.ChainState.OUTPUTS:
            a = getattr(s, name)
            setattr(out, name, self.buf[next_in if name == "next_in" else name].to_array(a.shape, a.dtype))
        return out

    def free(self):
        for b in self.buf.values():
            b.free()


def _points(rows, ndet, cap):
    """[ndet][cap][2] float32 with row k = rows[k] and NaN behind it: the kernels
    must not read a row's unused tail."""
    a = np.full((ndet, cap, 2), np.nan, np.float32)
    for k, r in enumerate(rows):
        a[k, :len(r)] = r
    return a


def _launch_step(cases, cap, step, scale, last=None, klt=None, reverse=False, dead_every=2, what=""):
    """cases: (box, pre, cur) per live detection (pre = the step's input points,
    cur = its LK output). One launch with a stopped detection after every
    `dead_every` live ones against the model -> the model's state and the live slots."""
    assert ORC.SCALE == scale
    order = list(range(len(cases)))[::-1] if reverse else list(range(len(cases)))
    rng = np.random.default_rng(len(cases) + 7 * step)
    slots = []  # (case index or None)
    for j, i in enumerate(order):
        slots.append(i)
        if dead_every and j % dead_every == dead_every - 1:
            slots.append(None)
    ndet = len(slots)
    boxes, cnt, pre, cur, lst = [], [], [], [], []
    for i in slots:
        if i is None:  # a stopped chain with plausible rows behind its zero count
            p, c = chain_ref.klt_case(rng, min(cap, 20), "cluster")
            boxes.append((50.0, 60.0, 10.0, 40.0))
            cnt.append(0)
            lst.append(int(rng.integers(0, 4)))
        else:
            b, p, c = cases[i]
            assert len(p) == len(c) <= cap
            boxes.append(b)
            cnt.append(len(p))
            lst.append(3 if last is None else int(last[i]))
        pre.append(p)
        cur.append(c)
    st = chain_ref.poison(chain_ref.ChainState(ndet, cap, boxes, cnt, None if last is None else lst))
    pre, cur = _points(pre, ndet, cap), _points(cur, ndet, cap)
    dev = DevChain(st, scale, cur=pre, nxt=cur)
    dev.c.cur, dev.c.nxt = dev.buf["cur"].addr, dev.buf["nxt"].addr
    try:
        assert _api().psn_t2d_chain_step_device(ctypes.byref(dev.c), step, None) == 0
        got = dev.get()
    finally:
        dev.free()
    want = st.copy()
    chain_ref.step(want, step, pre, cur, klt)
    chain_ref.assert_states_equal(got, want, f"{what} cap {cap} step {step} scale {scale} reverse {reverse}")
    return want, [k for k, i in enumerate(slots) if i is not None]


def _check_step(cases, cap, step, scale, what, **kw):
    want, live = _launch_step(cases, cap, step, scale, what=what, **kw)
    _launch_step(cases, cap, step, scale, what=what, reverse=True, **kw)
    return want, live


# ---------------------------------------------------------------------------
# The families (pure functions of their arguments: seeded, no GPU)
# ---------------------------------------------------------------------------

def _grid(n, x0=3.0, y0=7.0):
    i = np.arange(n, dtype=np.float32)
    return np.stack([x0 + i, y0 + 2 * (i % 40)], 1).astype(np.float32)


def family_a(cap, seed=100):
    rng = np.random.default_rng(seed + cap)
    cases = []
    for kind in chain_ref.KLT_KINDS:
        for n in counts(cap):
            for _ in range(3):
                pre, cur = chain_ref.klt_case(rng, n, kind)
                cases.append((chain_ref.klt_box(rng), pre, cur))
    for n in counts(cap):
        for _ in range(8):
            cases.append(chain_ref.window_edge_case(rng, n))
        pre, _ = chain_ref.klt_case(rng, n, "uniform")
        cases.append((chain_ref.klt_box(rng), pre, pre.copy()))  # nothing moves
    for w in (0.0, -5.0):  # an empty window at every count: no neighbour, no inlier
        for n in counts(cap):
            box, pre, cur = chain_ref.window_edge_case(rng, n)
            cases.append(((box[0], box[1], w, box[3]), pre, cur))
    return cases


def cover_a(cases, cap):
    tr = [chain_ref.trace(b[2], p, c) for b, p, c in cases]
    assert any(t["half_stop"] and t["n"] > 0 for t in tr), "no case stops by 'fewer than half moving'"
    assert any(not t["half_stop"] and t["ninl"] < 4 for t in tr), "no case stops by 'fewer than 4 inliers'"
    assert any(t["ninl"] >= 4 for t in tr), "no case runs"
    assert any(t["tied_values"] for t in tr), "no case has tied maxima at distinct values"
    assert any(b[2] <= 0 and not t["half_stop"] and t["M"] > 0 and t["max_count"] == 0 for (b, _, _), t in zip(cases, tr)), \
        "no case searches a mode with a non-positive window"
    assert {t["n"] for t in tr} == set(counts(cap)), "a point count is missing"
    if cap >= 65:
        assert any(t["M"] > 64 and not t["half_stop"] for t in tr), "no case has M > 64 (the second wave)"


def family_b(cap):
    """-> cases, and per case (n, movers, layout)."""
    cases, info = [], []
    for n in counts(cap):
        if n == 0:
            continue
        half = (n + 1) // 2
        for movers in (half, half - 1):
            for layout in ("first", "last", "interleaved"):
                lanes = {"first": np.arange(movers), "last": np.arange(n - movers, n),
                         "interleaved": 2 * np.arange(movers)}[layout]
                pre = _grid(n)
                cur = pre.copy()
                cur[lanes, 0] += np.float32(1.0)
                cases.append(((20.0, 30.0, 10.0, 40.0), pre, cur))
                info.append((n, movers, layout))
    for n, lanes in ((100, range(64, 100)), (128, range(64, 128)), (128, range(65, 128)), (127, range(64, 127))):
        if n <= cap:  # movers in the second wave only: the scan's carry is all there is
            pre = _grid(n)
            cur = pre.copy()
            cur[list(lanes), 0] += np.float32(1.0)
            cases.append(((20.0, 30.0, 10.0, 40.0), pre, cur))
            info.append((n, len(lanes), "wave1"))
    return cases, info


def cover_b(cases, info, cap):
    for (b, p, c), (n, movers, layout) in zip(cases, info):
        t = chain_ref.trace(b[2], p, c)
        assert t["M"] == movers, (n, movers, layout)
        assert t["half_stop"] == (2 * movers < n), f"half-moving decision of {(n, movers, layout)}"
        if not t["half_stop"]:
            assert t["ninl"] == movers, (n, movers, layout)  # equal moves: every mover is an inlier
        if layout == "wave1":
            assert t["lanes"].min() >= 64
    assert any(2 * m == n for n, m, _ in info), "no even n with exactly half moving"
    assert any(2 * m == n + 1 for n, m, _ in info), "no odd n with ceil(n/2) moving"
    if cap >= 128:
        assert any(lay == "wave1" and 2 * m >= n for n, m, lay in info), "no running case with movers in lanes >= 64 only"
    if cap >= 100:
        assert any(lay == "wave1" and 2 * m < n for n, m, lay in info), "no stopping case with movers in lanes >= 64 only"


def _norm2_unfused(ex, ey):
    return ex * ex + ey * ey


def _norm2_fma_x(ex, ey):  # fma(ex, ex, ey * ey): one rounding of the exact ex^2 + fl(ey^2)
    return float(Fraction(ex) * Fraction(ex) + Fraction(ey * ey))


def _norm2_fma_y(ex, ey):  # fma(ey, ey, ex * ex)
    return float(Fraction(ey) * Fraction(ey) + Fraction(ex * ex))


def klt_with(norm2):
    """The oracle's LocalSearchKLT with the inlier norm's radicand from norm2
    (the unfused one must be the oracle itself: test_family_coverage checks it)."""
    def klt(pre_box, pre, cur):
        pre = np.asarray(pre, np.float32).reshape(-1, 2)
        cur = np.asarray(cur, np.float32).reshape(-1, 2)
        n = len(pre)
        d = (cur - pre).astype(np.float64)
        idx = np.nonzero(~(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) < 0.1 * ORC.SCALE))[0]
        mv = d[idx]
        m = len(idx)
        if float(m) < float(n) * 0.5:
            return ORC.Rect(*pre_box.tuple()), []
        dxs, dys = np.sort(mv[:, 0]), np.sort(mv[:, 1])
        window = pre_box.w * 0.2 * ORC.SCALE
        nx = (np.abs(dxs[:, None] - dxs[None, :]) < window).sum(1)
        ny = (np.abs(dys[:, None] - dys[None, :]) < window).sum(1)
        ex = float(dxs[int(np.argmax(nx))]) if m and nx.max() > 0 else 0.0
        ey = float(dys[int(np.argmax(ny))]) if m and ny.max() > 0 else 0.0
        inl = [int(idx[j]) for j in range(m)
               if math.sqrt(norm2(float(mv[j, 0]) - ex, float(mv[j, 1]) - ey)) < window]
        box = ORC.Rect(*pre_box.tuple())
        box.x += ex
        box.y += ey
        return box, inl
    return klt


@functools.lru_cache(maxsize=None)
def _contraction_pairs(want=40, seed=5):
    """Float32 vector pairs (a, b), (c, d) with c > a, d > b whose difference has
    a norm that contraction changes: the unfused root differs from both fused
    roots and lies on one side of them. -> [(a, b, c, d, unfused root, nearer fused root)]"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < want:
        # a small (a, b) against a (c, d) of a few pixels: the difference of two float32
        # values then carries up to 29 bits, its square does not fit a double, and the
        # product's rounding (which a fused multiply-add skips) can show in the root
        a, b = (float(v) for v in rng.uniform(0.11, 0.25, 2).astype(np.float32))
        c, d = (float(v) for v in rng.uniform(2.0, 8.0, 2).astype(np.float32))
        ex, ey = c - a, d - b
        ru = math.sqrt(_norm2_unfused(ex, ey))
        f1, f2 = math.sqrt(_norm2_fma_x(ex, ey)), math.sqrt(_norm2_fma_y(ex, ey))
        if ex > 0 and ey > 0 and (ru < min(f1, f2) or ru > max(f1, f2)):
            out.append((a, b, c, d, ru, min(f1, f2) if ru < f1 else max(f1, f2)))
    return out


def _width_for(window, scale):
    """A double bw with bw * 0.2 * scale == window (the kernel's and the oracle's expression), or None."""
    bw = window / scale / 0.2
    for _ in range(8):
        bw = math.nextafter(bw, 0.0)
    for _ in range(17):
        if bw * 0.2 * scale == window:
            return bw
        bw = math.nextafter(bw, math.inf)
    return None


def family_c_radius(cap, scale):
    """Four equal moves (a, b) and a fifth (c, d) whose distance from them is the
    window or one root below it, depending on contraction alone; c > a and d > b
    keep the mode at (a, b), so the fifth vector decides its own membership only.
    -> cases, and the cluster's move (a, b) of each."""
    cases, modes = [], []
    for j, (a, b, c, d, ru, rf) in enumerate(_contraction_pairs()):
        bw = _width_for(max(ru, rf), scale)
        if bw is None:
            continue
        vec = [(a, b)] * 4
        vec.insert(j % 5, (c, d))
        if j % 2 and cap >= 7:  # far outliers around them
            vec = [(60.0 + a, 70.0 + b)] + vec + [(90.0 + c, 95.0 + d)]
        cur = np.float32(vec)
        cases.append(((11.0, 12.0, bw, 30.0), np.zeros_like(cur), cur))  # input points 0: the LK output is the vector
        modes.append((a, b))
    return cases, modes


def _near_threshold(scale):
    """Float32 vectors whose double norm sqrt(dx*dx + dy*dy) sits next to the
    movement threshold T = 0.1 * scale: -> [(below, above)], below the largest
    reachable norm < T and above the smallest >= T along its direction. The
    squares of float32 values are exact in double, so this comparison cannot
    tell a fused kernel from an unfused one. These pairs hold the comparison
    from both sides; the vectors whose norm is T itself are ON_THRESHOLD."""
    T = 0.1 * scale
    norm = lambda v: math.sqrt(float(v[0]) * float(v[0]) + float(v[1]) * float(v[1]))  # noqa: E731
    pairs = []
    hi = np.float32(T)
    if float(hi) < T:
        hi = np.nextafter(hi, np.float32(1))
    lo = np.nextafter(hi, np.float32(0))
    for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        pairs.append((np.float32([sx * lo, sy * lo]), np.float32([sx * hi, sy * hi])))
    for frac in (0.3, 0.6, 0.8, 0.95):
        dx = np.float32(T * frac)
        dy = np.float32(math.sqrt(T * T - float(dx) * float(dx)))
        while norm((dx, dy)) >= T:
            dy = np.nextafter(dy, np.float32(0))
        while norm((dx, np.nextafter(dy, np.float32(1)))) < T:
            dy = np.nextafter(dy, np.float32(1))
        up = np.nextafter(dy, np.float32(1))
        pairs.append((np.float32([dx, dy]), np.float32([dx, up])))
        pairs.append((np.float32([-dy, dx]), np.float32([-up, dx])))
    for below, above in pairs:
        assert norm(below) < T <= norm(above)
    return pairs


# Every float32 vector (dx >= dy > 0) whose double norm sqrt(dx*dx + dy*dy) is the
# movement threshold T = 0.1 * scale bit for bit: an equal norm counts as moving
# (`!(norm < T)`, :481), which only these inputs tell from a `<=`. Found by
# exhaustive search: every float32 dx in [T / sqrt(2), T] with the float32 dy
# within three steps of sqrt(T*T - dx*dx); signs and the swap give the rest.
# T is 0x1.999999999999ap-4 at scale 1.0, and the halves of the same vectors have
# the norm 0.05 of scale 0.5. At the scales 0.75 and 0.3 the search finds none.
ON_THRESHOLD = {1.0: ((0.09954984486103058, 0.009477783925831318), (0.09968885034322739, 0.007882456295192242),
                      (0.09982965141534805, 0.00583444070070982))}
ON_THRESHOLD[0.5] = tuple((dx / 2, dy / 2) for dx, dy in ON_THRESHOLD[1.0])


def _threshold_case(v, scale, lane):
    """3 clear movers, 3 static points and the vector v at `lane` (n = 7): v moves
    (4 of 7: the step runs, 4 inliers) or it does not (3 of 7: the step stops)."""
    far = np.float32([0.11 * scale, 0.0])
    vec = [far, far, far, np.float32([0, 0]), np.float32([0, 0]), np.float32([0, 0])]
    vec.insert(lane % 7, np.float32(v))
    cur = np.float32(vec)
    return ((5.0, 6.0, 20.0, 30.0), np.zeros_like(cur), cur)


def family_c_moving(cap, scale):
    """-> cases alternating a vector just below the movement threshold and one on/above it."""
    return [_threshold_case(v, scale, j) for j, pair in enumerate(_near_threshold(scale)) for v in pair]


def family_c_on(cap, scale):
    """The vectors of ON_THRESHOLD with their sign and swap variants (none at 0.75 and 0.3)."""
    cases = []
    for dx, dy in ON_THRESHOLD.get(scale, ()):
        for v in ((dx, dy), (dy, dx)):
            for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                cases.append(_threshold_case((sx * v[0], sy * v[1]), scale, len(cases)))
    return cases


def cover_c(radius, modes, moving, on, scale):
    unf, fx, fy = klt_with(_norm2_unfused), klt_with(_norm2_fma_x), klt_with(_norm2_fma_y)
    differ = 0
    for (b, p, c), (ma, mb) in zip(radius, modes):
        r = ORC.local_search_klt(ORC.Rect(*b), p, c)
        u, x, y = (k(ORC.Rect(*b), p, c) for k in (unf, fx, fy))
        assert (u[0].tuple(), u[1]) == (r[0].tuple(), r[1]), "the unfused restatement is not the oracle"
        assert u[0].tuple() == (b[0] + ma, b[1] + mb, b[2], b[3]), "the fifth vector moved the mode"
        assert {len(u[1]), len(x[1])} == {4, 5} and x[1] == y[1], "contraction does not decide the fifth inlier"
        differ += u[1] != x[1]
    assert differ >= 20, f"only {differ} cases tell a contracted inlier norm from the oracle's"
    for j in range(0, len(moving), 2):
        lo, hi = (chain_ref.trace(b[2], p, c) for b, p, c in moving[j:j + 2])
        assert lo["half_stop"] and lo["M"] == 3, "the vector below the movement threshold moves"
        assert not hi["half_stop"] and hi["M"] == 4 and hi["ninl"] == 4, "the vector on/above the threshold does not move"
    T = 0.1 * scale
    assert len(on) == (24 if scale in (1.0, 0.5) else 0), "the vectors on the movement threshold are missing"
    for b, p, c in on:
        v = [c[k] for k in range(7) if c[k].any() and c[k, 0] != np.float32(0.11 * scale)]
        assert len(v) == 1 and math.sqrt(float(v[0][0]) * float(v[0][0]) + float(v[0][1]) * float(v[0][1])) == T, \
            "the vector's norm is not the movement threshold"
        t = chain_ref.trace(b[2], p, c)
        assert not t["half_stop"] and t["M"] == 4 and t["ninl"] == 4, "the vector on the threshold does not move"


def family_d(cap):
    """-> cases, and the cluster size of each."""
    cases, sizes = [], []
    for c in (3, 4, 5):
        for total in sorted({c, 7, 31, 64, 65, 100, 128}):
            if not c <= total <= cap:
                continue
            for layout in ("first", "last", "interleaved"):
                lanes = {"first": np.arange(c), "last": np.arange(total - c, total),
                         "interleaved": np.arange(c) * ((total - 1) // max(c - 1, 1) if total > c else 1)}[layout]
                pre = _grid(total)
                i = np.arange(total, dtype=np.float32)
                cur = pre + np.stack([10 * (i + 1), -7 * (i + 1)], 1)  # scattered: no two within the window
                cur[lanes] = pre[lanes] + np.float32([2.0, -1.0])
                cases.append(((40.0, 50.0, 4.0, 30.0), pre, cur.astype(np.float32)))
                sizes.append(c)
    return cases, sizes


def cover_d(cases, sizes):
    seen = set()
    for (b, p, c), size in zip(cases, sizes):
        t = chain_ref.trace(b[2], p, c)
        assert not t["half_stop"] and t["ninl"] == size, f"the cluster of {size} is not the inlier set"
        seen.add(t["ninl"])
    assert seen == {3, 4, 5}, "3, 4 and 5 inliers do not all occur"


def family_e(cap, seed=9):
    """Clusters A, B of dx and D, C of dy, each of n // 2 points, split so that
    A and D come first in sorted order and share ceil(n/4) points."""
    rng = np.random.default_rng(seed + cap)
    cases = []
    for n in counts(cap):
        s = n // 2
        if s < 1:
            continue
        for spread in (0.0, 0.0625):
            dx = np.concatenate([np.full(s, -3.0), np.full(s, 4.0)]) + spread * (np.arange(2 * s) % 4)
            in_d = np.concatenate([np.arange(s) % 2 == 0, np.arange(s) % 2 == 1])
            dy = np.where(in_d, -5.0, 2.0) + spread * (np.arange(2 * s) % 3)
            d = np.stack([dx, dy], 1)
            if n % 2:
                d = np.concatenate([d, [[40.0, 45.0]]])
            d = d[rng.permutation(n)]
            pre = _grid(n)
            cases.append(((7.0, 8.0, 5.0, 30.0), pre, (pre + d).astype(np.float32)))
    return cases


def cover_e(cases, cap):
    full = False
    for b, p, c in cases:
        t = chain_ref.trace(b[2], p, c)
        n = t["n"]
        assert t["M"] == n and t["tied_values"] and t["max_count"] == n // 2, f"n {n}: the clusters' counts are not tied"
        assert t["ninl"] == (n // 2 + 1) // 2, f"n {n}: the first maxima in sorted order did not win"
        full = full or n == cap
    assert full or cap not in counts(cap), "no case fills the row (n = cap)"


def family_g(cap, seed=21):
    rng = np.random.default_rng(seed + cap)
    ns = [n for n in counts(cap) if n >= 4]
    cases, last = [], []
    for j in range(96):
        n = ns[j % len(ns)]
        pre, cur = chain_ref.klt_case(rng, n, "cluster")
        cases.append(((30.0, 40.0, float(rng.integers(5, 13)), 50.0), pre, cur))
        last.append((j // len(ns)) % 4)  # every count meets every last_step
    return cases, last


def cover_g(want, live, step):
    run = [k for k in live if want.nsteps[k] == step]
    assert any(want.cnt[k] == 0 and step >= want.last_step[k] for k in run), "no chain ends at its last step"
    if step < 3:
        assert any(want.cnt[k] > 0 and step < want.last_step[k] for k in run), "no chain goes on past this step"
    assert all((want.cnt[k] == 0) == (step >= want.last_step[k]) for k in run)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("scale", (1.0,) + SCALES)
def test_family_coverage(monkeypatch, cap, scale):
    """Every family hits what it claims, from the model alone (no GPU)."""
    monkeypatch.setattr(ORC, "SCALE", scale)
    cover_a(family_a(cap), cap)
    cover_c(*family_c_radius(cap, scale), family_c_moving(cap, scale), family_c_on(cap, scale), scale)
    if scale == 1.0:
        cover_b(*family_b(cap), cap)
        cover_d(*family_d(cap))
        cover_e(family_e(cap), cap)
        cases, last = family_g(cap)
        for step in (1, 2, 3):
            st = chain_ref.ChainState(len(cases), cap, [b for b, _, _ in cases], [len(p) for _, p, _ in cases], last)
            chain_ref.step(st, step, _points([p for _, p, _ in cases], len(cases), cap),
                           _points([c for _, _, c in cases], len(cases), cap))
            cover_g(st, range(len(cases)), step)


# ---------------------------------------------------------------------------
# GPU: one step
# ---------------------------------------------------------------------------

CAP_STEP = [(100, 1), (100, 2), (100, 3), (128, 1), (128, 3), (7, 1), (7, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("cap,step", CAP_STEP)
def test_step_family_a_klt_cases(cap, step):
    cases = family_a(cap)
    cover_a(cases, cap)
    _check_step(cases, cap, step, 1.0, "family a")


@pytest.mark.gpu
@pytest.mark.parametrize("cap,step", CAP_STEP)
def test_step_family_b_half_moving(cap, step):
    cases, info = family_b(cap)
    cover_b(cases, info, cap)
    _check_step(cases, cap, step, 1.0, "family b")


@pytest.mark.gpu
@pytest.mark.parametrize("cap,step", [(100, 1), (128, 2), (7, 3)])
def test_step_family_c_thresholds(cap, step):
    (radius, modes), moving, on = family_c_radius(cap, 1.0), family_c_moving(cap, 1.0), family_c_on(cap, 1.0)
    cover_c(radius, modes, moving, on, 1.0)
    # the device equals the unfused model, which cover_c has shown to be the oracle and to differ from both fused ones
    _check_step(radius + moving + on, cap, step, 1.0, "family c", klt=klt_with(_norm2_unfused))


@pytest.mark.gpu
@pytest.mark.parametrize("cap,step", [(100, 1), (128, 2), (7, 3)])
def test_step_family_d_three_against_four(cap, step):
    cases, sizes = family_d(cap)
    cover_d(cases, sizes)
    _check_step(cases, cap, step, 1.0, "family d")


@pytest.mark.gpu
@pytest.mark.parametrize("cap,step", [(100, 1), (128, 2), (7, 3)])
def test_step_family_e_equal_counts(cap, step):
    cases = family_e(cap)
    cover_e(cases, cap)
    _check_step(cases, cap, step, 1.0, "family e")


@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("cap,step", [(100, 1), (128, 3)])
def test_step_family_f_scales(monkeypatch, cap, step, scale):
    monkeypatch.setattr(ORC, "SCALE", scale)
    a = family_a(cap)
    (radius, modes), moving, on = family_c_radius(cap, scale), family_c_moving(cap, scale), family_c_on(cap, scale)
    cover_a(a, cap)
    cover_c(radius, modes, moving, on, scale)
    _check_step(a + radius + moving + on, cap, step, scale, "family f")


@pytest.mark.gpu
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("step", [1, 2, 3])
def test_step_family_g_last_step(cap, step):
    cases, last = family_g(cap)
    want, live = _check_step(cases, cap, step, 1.0, "family g", last=last)
    cover_g(want, live, step)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", CAPS)
def test_step_single_detection(cap):
    pre = _grid(cap)
    i = np.arange(cap)
    cur = pre + np.stack([2.0 + (i % 3) * 0.125, -1.0 - (i % 2) * 0.25], 1).astype(np.float32)
    cur[cap // 2] += np.float32([30.0, 40.0])  # one outlier
    case = [((30.0, 40.0, 8.0, 50.0), pre, cur)]
    assert chain_ref.trace(8.0, pre, cur)["ninl"] == cap - 1
    want, _ = _launch_step(case, cap, 1, 1.0, dead_every=0, what="ndet 1")
    assert want.ndet == 1 and want.nsteps[0] == 1


# ---------------------------------------------------------------------------
# GPU: begin + three steps, buffers handed over as Tracker2DFlow's chain pass does
# ---------------------------------------------------------------------------

def _sequence_plan(ndet, cap):
    """Per detection: its feature count, the step it stops at (4: never), how
    (static: fewer than half move; scatter: fewer than 4 inliers), last_step."""
    ns = [n for n in (0, 3, 4, 5, 8, 31, 63, 64, 65, 99, 100, 127, 128) if n <= cap]
    plan = []
    for k in range(ndet):
        stop = (1, 1, 1, 2, 2, 2, 3, 3, 3, 4)[k % 10]
        plan.append((ns[k % len(ns)], stop, "static" if (k // 10) % 2 else "scatter", k % 4 if k % 7 == 0 else 3))
    return plan


def _sequence_next(plan, state, cur, step):
    """The prescribed LK output of `step` for every live detection (no LK)."""
    rows = []
    for k, (_, stop, how, _) in enumerate(plan):
        n = int(state.cnt[k])
        p = cur[k, :n].astype(np.float64)
        i = np.arange(n, dtype=np.float64)
        if step == stop and how == "static":
            d = np.zeros((n, 2))
        elif step == stop:
            d = np.stack([5 + 10 * i, 5 - 7 * i], 1)
        else:
            d = np.tile([1.5 + 0.25 * step, -0.75 * step], (n, 1)) + np.stack([(i % 3) * 0.125, (i % 2) * 0.25], 1)
            out = i % 5 == 4
            d[out] = np.stack([15 + 3 * i[out], -20 - 2 * i[out]], 1)
        rows.append((p + d).astype(np.float32))
    return _points(rows, len(plan), state.cap)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [100, 128])
def test_three_step_sequence(cap):
    ndet = 203
    plan = _sequence_plan(ndet, cap)
    rng = np.random.default_rng(cap + 1)
    feats = [rng.uniform(10, 300, (n, 2)).astype(np.float32) for n, _, _, _ in plan]
    st = chain_ref.poison(chain_ref.ChainState(ndet, cap, [(20.0, 30.0, 10.0, 40.0)] * ndet, [len(f) for f in feats],
                                               [p[3] for p in plan]))
    cur0 = _points(feats, ndet, cap)
    poison_pts = np.empty((ndet, cap, 2), np.float32)
    chain_ref.bits(poison_pts)[...] = chain_ref.POISON_F32
    dev = DevChain(st, 1.0, d_in=cur0, nxt=cur0, buf0=poison_pts, buf1=poison_pts)
    L = _api()
    try:
        dev.c.cur = dev.buf["d_in"].addr
        assert L.psn_t2d_chain_begin_device(ctypes.byref(dev.c), ORC.MIN_FEATURES, None) == 0
        chain_ref.begin(st, cur0, ORC.MIN_FEATURES)
        chain_ref.assert_states_equal(dev.get(), st, "begin")
        cur, stopped = cur0, []
        for step in (1, 2, 3):
            src = "d_in" if step == 1 else f"buf{step & 1}"
            dst = f"buf{(step + 1) & 1}"
            nxt = _sequence_next(plan, st, cur, step)
            dev.put("nxt", nxt)
            dev.put(dst, poison_pts)
            chain_ref.poison_next_in(st)
            dev.c.cur, dev.c.nxt, dev.c.next_in = dev.buf[src].addr, dev.buf["nxt"].addr, dev.buf[dst].addr
            live = st.cnt > 0
            assert L.psn_t2d_chain_step_device(ctypes.byref(dev.c), step, None) == 0
            chain_ref.step(st, step, cur, nxt)
            chain_ref.assert_states_equal(dev.get(next_in=dst), st, f"step {step}")
            stopped.append(int((live & (st.nsteps < step)).sum()))
            cur = st.next_in.copy()
    finally:
        dev.free()
    # roughly a third of the started chains stops at each step; the rest run to the end or to their last_step
    started = sum(1 for n, _, _, last in plan if n >= ORC.MIN_FEATURES and last >= 1)
    assert all(s >= started // 5 for s in stopped), (started, stopped)
    assert (st.nsteps == 3).sum() >= 5 and ((st.nsteps == 2) & (st.last_step == 2)).sum() >= 1


# ---------------------------------------------------------------------------
# GPU: chain_begin and gate_counts alone
# ---------------------------------------------------------------------------

def _begin_counts(cap):
    return [0, 3, 4, 5, cap - 1, cap, cap + 1, 2 * cap]


@pytest.mark.gpu
@pytest.mark.parametrize("mixed_last", [False, True])
@pytest.mark.parametrize("min_count", [0, 4, 101])
@pytest.mark.parametrize("cap", CAPS)
def test_chain_begin(cap, min_count, mixed_last):
    rng = np.random.default_rng(cap + min_count)
    for reverse in (False, True):
        cnt = (_begin_counts(cap) * 40)[::-1 if reverse else 1]
        ndet = len(cnt)
        last = rng.integers(0, 4, ndet) if mixed_last else None
        st = chain_ref.poison(chain_ref.ChainState(ndet, cap, None, cnt, last))
        cur = rng.uniform(0, 500, (ndet, cap, 2)).astype(np.float32)  # whole rows: a count above cap reads cap points
        dev = DevChain(st, 1.0, cur=cur)
        dev.c.cur = dev.buf["cur"].addr
        if reverse:  # begin needs neither the boxes nor the step's buffers
            dev.c.boxes = dev.c.nxt = dev.c.next_in = dev.c.out_boxes = None
        try:
            assert _api().psn_t2d_chain_begin_device(ctypes.byref(dev.c), min_count, None) == 0
            got = dev.get()
            dev.c.ndet = 0  # nothing to do: no launch, nothing touched
            assert _api().psn_t2d_chain_begin_device(ctypes.byref(dev.c), min_count, None) == 0
            assert _api().psn_t2d_chain_step_device(ctypes.byref(dev.c), 1, None) == 0
            again = dev.get()
        finally:
            dev.free()
        want = st.copy()
        chain_ref.begin(want, cur, min_count)
        chain_ref.assert_states_equal(got, want, f"begin cap {cap} min {min_count}")
        chain_ref.assert_states_equal(again, want, "ndet 0")
        assert (want.set_cnt[:, 0] <= cap).all(), "set 0 is not clamped to the cap"
        assert (want.set_cnt[:, 0] == cap).any() == any(c >= max(cap, min_count) for c in cnt)


@pytest.mark.gpu
@pytest.mark.parametrize("mixed_last", [False, True])
@pytest.mark.parametrize("min_count", [0, 4, 101])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_gate_counts(n, min_count, mixed_last):
    import hiprt

    rng = np.random.default_rng(n + min_count)
    pad = 64
    cnt = np.full(n + pad, chain_ref.POISON_I32, np.int32)
    cnt[:n] = rng.choice(_begin_counts(100) + [100, 101, 102], n)
    last = rng.integers(0, 4, n).astype(np.int32) if mixed_last else None
    d_cnt = hiprt.DeviceBuffer.from_array(cnt)
    d_last = hiprt.DeviceBuffer.from_array(last) if mixed_last else None
    try:
        assert _api().psn_t2d_gate_counts_device(d_cnt.addr, n, min_count, d_last.addr if d_last else None, None) == 0
        got = d_cnt.to_array(cnt.shape, np.int32)
        assert _api().psn_t2d_gate_counts_device(d_cnt.addr, 0, 1 << 30, None, None) == 0  # n = 0: nothing touched
        again = d_cnt.to_array(cnt.shape, np.int32)
    finally:
        d_cnt.free()
        if d_last:
            d_last.free()
    want = cnt.copy()
    chain_ref.gate(want[:n], min_count, last)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(again, want)


# ---------------------------------------------------------------------------
# Argument checks: rejected before any launch (no GPU needed)
# ---------------------------------------------------------------------------

def test_argument_checks():
    L = _api()
    keep = (ctypes.c_double * 64)()  # a non-null address no accepted call ever reaches
    p = ctypes.addressof(keep)

    def chain(ndet=0, cap=100, scale=1.0, **null):
        c = ChainDev(ndet=ndet, cap=cap, scale=scale)
        for name, _ in ChainDev._fields_[2:-1]:
            setattr(c, name, None if name in null else p)
        return c

    step = lambda c, s: L.psn_t2d_chain_step_device(ctypes.byref(c), s, None)  # noqa: E731
    begin = lambda c, m=4: L.psn_t2d_chain_begin_device(ctypes.byref(c), m, None)  # noqa: E731
    assert L.psn_t2d_chain_step_device(None, 1, None) == ERR_ARG
    assert L.psn_t2d_chain_begin_device(None, 4, None) == ERR_ARG
    # ndet = 0 is accepted without a launch, so every rejection below is the check named
    assert step(chain(), 1) == 0 and step(chain(), 3) == 0 and begin(chain()) == 0 and step(chain(cap=128), 1) == 0
    for cap in (0, 129, -1):
        assert step(chain(cap=cap), 1) == ERR_ARG and begin(chain(cap=cap)) == ERR_ARG, cap
    for s in (0, 4, -1):
        assert step(chain(), s) == ERR_ARG, s
    for scale in (0.0, -0.5, math.nan):
        assert step(chain(scale=scale), 1) == ERR_ARG, scale
    assert step(chain(ndet=-1), 1) == ERR_ARG and begin(chain(ndet=-1)) == ERR_ARG
    for name in ("cnt", "cur", "sets", "set_cnt", "nsteps"):
        assert begin(chain(ndet=1, **{name: True})) == ERR_ARG, name
    assert L.psn_t2d_gate_counts_device(None, 5, 4, None, None) == ERR_ARG
    assert L.psn_t2d_gate_counts_device(p, -1, 4, None, None) == ERR_ARG
    assert L.psn_t2d_gate_counts_device(None, 0, 4, None, None) == 0
