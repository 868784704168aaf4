"""A plain model of the backward-chain device entry points
(include/psn_t2d_device.h: psn_t2d_chain_begin_device, psn_t2d_gate_counts_device,
psn_t2d_chain_step_device) in numpy / Python floats, on top of the CPU
restatement's LocalSearchKLT (oracle/tracker2d_oracle.py), and the seeded
LocalSearchKLT input generators the host tests (test_tracker2d.py) and the
device tests (test_chain_step_gpu.py) share. No tests of its own:
test_chain_ref.py ties the model to the oracle's backward_tracking schedule.

The model writes into the caller's arrays exactly what the header promises
and nothing else, so a test that poisons the device buffers and these arrays
alike sees every write outside the promised set.
"""
import numpy as np

import tracker2d_oracle as ORC

STEPS = 4  # PSN_T2D_CHAIN_STEPS


class ChainState:
    """Host mirror of the buffers of psn_t2d_chain_dev (every array C-contiguous)."""

    def __init__(self, ndet, cap, boxes=None, cnt=None, last_step=None):
        self.ndet, self.cap = ndet, cap
        self.boxes = np.zeros((ndet, 4), np.float64) if boxes is None else \
            np.ascontiguousarray(boxes, np.float64).reshape(ndet, 4)
        self.cnt = np.zeros(ndet, np.int32) if cnt is None else np.ascontiguousarray(cnt, np.int32).reshape(ndet)
        self.last_step = None if last_step is None else np.ascontiguousarray(last_step, np.int32).reshape(ndet)
        self.next_in = np.zeros((ndet, cap, 2), np.float32)
        self.out_boxes = np.zeros((ndet, STEPS, 4), np.float64)
        self.sets = np.zeros((ndet, STEPS, cap, 2), np.float32)
        self.set_cnt = np.zeros((ndet, STEPS), np.int32)
        self.nsteps = np.zeros(ndet, np.int32)

    OUTPUTS = ("next_in", "out_boxes", "sets", "set_cnt", "nsteps")

    def copy(self):
        s = ChainState(self.ndet, self.cap, self.boxes.copy(), self.cnt.copy(),
                       None if self.last_step is None else self.last_step.copy())
        for name in self.OUTPUTS:
            setattr(s, name, getattr(self, name).copy())
        return s


POISON_F32 = 0x7FC0BEEF           # quiet NaNs with a payload: no kernel computes them
POISON_F64 = 0x7FF8DEADBEEF0BAD
POISON_I32 = -0x5EAD


def bits(a):
    """The integer view of a float array (-0.0 and NaN payloads count); ints as they are."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize]) if a.dtype.kind == "f" else a


def poison(state):
    """Every output buffer of the state filled with its sentinel."""
    for name in ChainState.OUTPUTS:
        a = getattr(state, name)
        if a.dtype.kind == "f":
            bits(a)[...] = POISON_F32 if a.itemsize == 4 else POISON_F64
        else:
            a[...] = POISON_I32
    return state


def poison_next_in(state):
    """next_in alone (a sequence hands it over between steps; the other outputs accumulate)."""
    bits(state.next_in)[...] = POISON_F32


def assert_states_equal(got, want, what=""):
    """Counts and every output buffer, bit for bit."""
    for name in ("cnt",) + ChainState.OUTPUTS:
        np.testing.assert_array_equal(bits(getattr(got, name)), bits(getattr(want, name)), err_msg=f"{what}: {name}")


def gate(cnt, min_count, last_step=None):
    """psn_t2d_gate_counts_device on a bare count array (in place)."""
    for k in range(len(cnt)):
        if cnt[k] < min_count or (last_step is not None and last_step[k] < 1):
            cnt[k] = 0


def begin(state, cur, min_count):
    """psn_t2d_chain_begin_device: counters cleared, set 0 = the first
    min(cnt, cap) points of cur where cnt >= min_count, then the gate."""
    for k in range(state.ndet):
        n = int(state.cnt[k])
        m = min(n, state.cap) if n >= min_count else 0
        state.nsteps[k] = 0
        state.set_cnt[k] = [m, 0, 0, 0]
        state.sets[k, 0, :m] = cur[k, :m]
    gate(state.cnt, min_count, state.last_step)


def step(state, step, cur, nxt, klt=None):
    """psn_t2d_chain_step_device for chain step `step` (1..3). klt: the
    LocalSearchKLT to use (default: the oracle's)."""
    klt = ORC.local_search_klt if klt is None else klt
    for k in range(state.ndet):
        n = int(state.cnt[k])
        if n == 0:
            continue
        box, inl = klt(ORC.Rect(*state.boxes[k]), cur[k, :n], nxt[k, :n])
        ninl = len(inl)
        if ninl < ORC.MIN_FEATURES:
            state.cnt[k] = 0
            continue
        state.out_boxes[k, step] = (box.x, box.y, state.boxes[k, 2], state.boxes[k, 3])
        ended = state.last_step is not None and step >= state.last_step[k]
        state.cnt[k] = 0 if ended else ninl
        state.nsteps[k] = step
        state.set_cnt[k, step] = ninl
        state.next_in[k, :ninl] = nxt[k, inl]
        state.sets[k, step, :ninl] = nxt[k, inl]
        if step == 1:
            state.set_cnt[k, 0] = ninl
            state.sets[k, 0, :ninl] = cur[k, inl]


def trace(box_w, pre, cur):
    """What LocalSearchKLT meets on one input, for the coverage assertions of the
    tests (never for a comparison): n, the moving count M, whether the half-moving
    test stops it, whether either mode search has tied maxima at distinct sorted
    positions, the inlier count and the lanes of the moving vectors."""
    pre = np.asarray(pre, np.float32).reshape(-1, 2)
    cur = np.asarray(cur, np.float32).reshape(-1, 2)
    n = len(pre)
    d = (cur - pre).astype(np.float64)
    idx = np.nonzero(~(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) < 0.1 * ORC.SCALE))[0]
    m = len(idx)
    out = {"n": n, "M": m, "lanes": idx, "half_stop": float(m) < float(n) * 0.5, "tied": False, "tied_values": False,
           "max_count": 0}
    if out["half_stop"]:
        out["ninl"] = 0
        return out
    window = box_w * 0.2 * ORC.SCALE
    for a in (np.sort(d[idx, 0]), np.sort(d[idx, 1])):
        c = (np.abs(a[:, None] - a[None, :]) < window).sum(1)
        if m and c.max() > 0:
            at = np.nonzero(c == c.max())[0]
            out["tied"] = out["tied"] or len(at) > 1
            out["tied_values"] = out["tied_values"] or len(np.unique(a[at])) > 1
            out["max_count"] = max(out["max_count"], int(c.max()))
    _, inl = ORC.local_search_klt(ORC.Rect(0.0, 0.0, box_w, 1.0), pre, cur)
    out["ninl"] = len(inl)
    return out


# ---------------------------------------------------------------------------
# Seeded LocalSearchKLT inputs (pre = the LK prevPts, cur = its nextPts)
# ---------------------------------------------------------------------------

KLT_KINDS = ("static", "cluster", "ties", "uniform")


def klt_case(rng, n, kind):
    pre = rng.uniform(0, 100, (n, 2)).astype(np.float32)
    if kind == "static":
        d = rng.normal(0, 0.03, (n, 2))
    elif kind == "cluster":
        d = np.array([rng.uniform(-5, 5), rng.uniform(-5, 5)]) + rng.normal(0, 0.3, (n, 2))
        out = rng.random(n) < 0.3
        d[out] = rng.uniform(-20, 20, (out.sum(), 2))
    elif kind == "ties":
        d = rng.integers(-3, 4, (n, 2)).astype(np.float64)
    else:
        d = rng.uniform(-8, 8, (n, 2))
    cur = (pre + d).astype(np.float32)
    return pre, cur


def klt_box(rng):
    """The box of a klt_case trial (integer width and height)."""
    return (rng.uniform(0, 200), rng.uniform(0, 200), float(rng.integers(8, 80)), float(rng.integers(20, 200)))


EDGE_WIDTHS = (0.0, -5.0, 5.0, 10.0, 15.0, 20.0, 25.0, 7.5, 12.5)


def window_edge_case(rng, n=None):
    """Neighbour counts at the window's edge: integer and half-integer moves,
    box widths that make 0.2 * w an integer, empty windows (w <= 0), long runs
    of equal moves. n: the point count (drawn from 1..100 when None). -> (box, pre, cur)."""
    if n is None:
        n = int(rng.integers(1, 101))
    pre = rng.uniform(0, 100, (n, 2)).astype(np.float32)
    d = rng.integers(-4, 5, (n, 2)).astype(np.float64) * rng.choice([0.5, 1.0, 2.0])
    cur = (pre + d).astype(np.float32)
    w = float(rng.choice(list(EDGE_WIDTHS)))
    box = (rng.uniform(0, 200), rng.uniform(0, 200), w, 40.0)
    return box, pre, cur
