"""The reference's Tracker2D steps (host/tracker2d_steps.cpp: the backward chain's
bookkeeping, LocalSearchKLT, the forward matching cost and its majority gate)
against oracle/tracker2d_oracle.py, bit for bit, on a machine without a GPU.

tests/cpp/flow_steps_check.cpp is compiled with tracker2d_steps.cpp and
tracker2d_match.cpp only, under AddressSanitizer + UndefinedBehaviorSanitizer,
into a program of its own (nothing is loaded into this process). No LK runs on
either side: the oracle's _lk is replaced by a generator of seeded point sets,
which are recorded and handed to the program in its case file, so both sides see
the same "LK outputs" (displacement mixes as _klt_case of test_tracker2d.py:
static, cluster with outliers, integer ties).

The cases are laid out so that the oracle alone takes every branch of the list
in BRANCHES; that is asserted from the oracle's own results (boxes, sets, flags,
costs), so a case set that misses one fails instead of passing quietly.
tracker2d_oracle.SCALE is a module global read at call time, so the scale path
(0.5) runs through the same oracle with it set.
"""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ORC = pytest.importorskip("tracker2d_oracle")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "mcmtt_opticalflow_amd", "host")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fsanitize=float-cast-overflow",
       "-static-libasan", "-static-libubsan"]
RING = [3, 0, 1, 2]  # LK slot ids, oldest first
W, H = 60.0, 90.0    # the grid detections' box
BRANCHES = {"det_dropped", "det_capped", "stop_step1", "stop_step2", "all_steps", "one_past_frame", "set0_is_features",
            "overlap_set", "overlap_clear", "tracker_skipped", "gate_overlap", "gate_distance", "gate_area",
            "gate_center", "duration_past_boxes", "majority_clears", "majority_keeps"}
# (seed, scale, past frames in the ring)
CASES = [(1, 1.0, 3), (2, 1.0, 1), (3, 1.0, 2), (4, 0.5, 3), (5, 0.5, 1)]


class Slot:  # a ring entry: the oracle only hands it to _lk
    def __init__(self, slot):
        self.slot = slot


def _move(rng, pts, kind, shift=(0.0, 0.0)):
    """pts displaced as _klt_case of test_tracker2d.py displaces them, around `shift`."""
    n = len(pts)
    if kind == "static":
        d = rng.normal(0, 0.03, (n, 2))
    elif kind == "cluster":
        d = np.asarray(shift, np.float64) + rng.normal(0, 0.3, (n, 2))
        out = rng.random(n) < 0.3
        d[out] = rng.uniform(-20, 20, (int(out.sum()), 2))
    else:  # ties
        d = rng.integers(-3, 4, (n, 2)).astype(np.float64)
    return (pts + d).astype(np.float32)


def _pts_in(rng, box, n, scale):
    x, y, w, h = box
    return (np.stack([rng.uniform(x + 1, x + w - 1, n), rng.uniform(y + 1, y + h - 1, n)], 1) * scale).astype(np.float32)


def _build(seed, scale, npast):
    """Detections on a grid (no two cells overlap), a few placed on purpose, and
    trackers placed against them; every placement names the branch it is for."""
    rng = np.random.default_rng(seed)
    cell = lambda j, r: (20.0 + 100.0 * j, 20.0 + 110.0 * r, W, H)  # noqa: E731
    dets, nfeat, kinds = [], [], []
    for r in range(4):
        for j in range(6):
            dets.append(cell(j, r))
            nfeat.append(int(rng.integers(10, 101)))
            kinds.append([str(rng.choice(["cluster", "ties"])) for _ in range(3)])
    nfeat[0], nfeat[1] = 3, 0            # det_dropped
    nfeat[2], nfeat[3] = 120, 4          # det_capped, the minimum
    kinds[4] = ["static"] * 3            # stop_step1, set0_is_features
    kinds[5] = ["cluster", "static", "cluster"]  # stop_step2
    kinds[6] = ["cluster", "ties", "cluster"]    # all_steps
    for i in range(7, 16):
        kinds[i][0] = "cluster"          # the trackers placed below need a chain with a first step
    dets.append((20.0 + 100.0 * 5 + 20.0, 20.0 + 110.0 * 3 + 20.0, W, H))  # overlap_set: over the last grid cell
    nfeat.append(30)
    kinds.append(["cluster"] * 3)
    shifts = [[(float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3))) for _ in range(3)] for _ in dets]
    feats = [_pts_in(rng, b, n, scale) for b, n in zip(dets, nfeat)]

    def history(i, nb, first=(0.0, 0.0)):
        """a tracker's boxes t-nb .. t-1 along detection i's backward chain (+ `first` on the box at t-1)"""
        x, y, w, h = dets[i]
        out, cx, cy = [], 0.0, 0.0
        for b in range(1, nb + 1):
            cx, cy = cx + shifts[i][b - 1][0] / scale, cy + shifts[i][b - 1][1] / scale
            jx, jy = rng.uniform(-1, 1, 2)
            out.append((x + cx + jx + (first[0] if b == 1 else 0.0), y + cy + jy + (first[1] if b == 1 else 0.0), w, h))
        return out[::-1]

    trackers = []  # dict(boxes, duration, n, status_ones, shift)

    def tracker(i, nb=3, first=(0.0, 0.0), jump=False, box=None, n=None, duration=None, ones=None):
        boxes = history(i, nb, first)
        if box is not None:
            boxes[-1] = box
        # its points move back along the chain's first step (and, with jump, all the way from `first`)
        back = (-shifts[i][0][0] - first[0] * scale * jump, -shifts[i][0][1] - first[1] * scale * jump)
        trackers.append(dict(boxes=boxes, duration=duration, n=int(rng.integers(12, 60)) if n is None else n,
                             ones=ones, shift=back))

    x7, y7 = dets[7][:2]
    tracker(6)                                        # a plain match over a full chain
    tracker(7, box=(x7 - 70.0, y7, 200.0, H))         # gate_distance: same centre line, 140 px wider
    tracker(8, first=(48.0, 0.0), nb=1)               # gate_area: a fifth of the box shared
    tracker(9, first=(0.0, 50.0), nb=1)               # gate_center: 50 px below, 4/9 shared
    tracker(10, first=(100.0, 0.0), nb=2, jump=True)  # gate_overlap at t-1: it jumps 100 px onto the detection
    tracker(11, duration=9)                           # duration_past_boxes
    tracker(12, ones=3)                               # tracker_skipped
    tracker(13, n=20)                                 # majority_clears: two trackers on one detection,
    tracker(13, n=30)                                 # the second with more points in its box
    tracker(14, nb=1)                                 # majority_keeps: the only tracker on its detection
    for i in range(15, len(dets)):
        tracker(i, nb=int(rng.integers(1, 4)))
    for tr in trackers:
        tr["feat"] = _pts_in(rng, tr["boxes"][-1], tr["n"], scale)
    return rng, dets, feats, kinds, shifts, trackers


def _run_oracle(monkeypatch, seed, scale, npast):
    """The oracle over the case, its _lk replaced; -> (case file text, expected lines, branches taken)."""
    rng, dets, feats, kinds, shifts, trackers = _build(seed, scale, npast)
    ring = [None] * (3 - npast) + [Slot(s) for s in RING[3 - npast:]]
    valid = [i for i, f in enumerate(feats) if len(f) >= ORC.MIN_FEATURES]
    state = {"k": -1, "fwd": None}
    bsets, fsets, jobs = {}, {}, []

    def lk(prev_img, next_img, pts, win):
        pts = np.asarray(pts, np.float32).reshape(-1, 2)
        st = (rng.random(len(pts)) < 0.9).astype(np.uint8)
        if state["fwd"] is not None:  # forward_tracking: tracker state["fwd"], frame t-1 -> t
            t = state["fwd"]
            state["fwd"] = t + 1
            tr = trackers[t]
            if tr["ones"] is not None:
                st[:] = 0
                st[:tr["ones"]] = 1
            nxt = _move(rng, pts, "cluster", tr["shift"])
            fsets[t] = (nxt, st)
            jobs.append(["job", "fwd", t, prev_img.slot, next_img.slot, win[0], win[1]])
            return nxt.copy(), st.copy()
        step = RING[::-1].index(next_img.slot)  # backward_tracking: frame t-step+1 -> t-step
        if step == 1:
            state["k"] += 1
        det = valid[state["k"]]
        nxt = _move(rng, pts, kinds[det][step - 1], shifts[det][step - 1])
        bsets[(det, step)] = (nxt, st)
        jobs.append(["job", "bwd", det, step, prev_img.slot, next_img.slot, win[0], win[1]])
        return nxt.copy(), st.copy()

    monkeypatch.setattr(ORC, "_lk", lk)
    monkeypatch.setattr(ORC, "SCALE", scale)
    objs = ORC.backward_tracking(ring, [ORC.Rect(*b) for b in dets], feats)
    trs = [ORC.Tracker(t["boxes"], t["feat"], duration=t["duration"]) for t in trackers]
    state["fwd"] = 0
    cost = ORC.forward_tracking(ring, trs, objs)

    pt = lambda a: " ".join(f"{float(x).hex()} {float(y).hex()}" for x, y in a)  # noqa: E731
    rc = lambda b: " ".join(float(v).hex() for v in b)  # noqa: E731
    by = lambda s: " ".join(str(int(v)) for v in s)  # noqa: E731
    text = [f"scale {float(scale).hex()} npast {npast} ring {by(RING)}", f"dets {len(dets)}"]
    text += [f"{rc(b)} {len(f)} {pt(f)}" for b, f in zip(dets, feats)]
    text.append(f"bsets {len(bsets)}")
    text += [f"{d} {s} {len(p)} {pt(p)} {by(st)}" for (d, s), (p, st) in bsets.items()]
    text.append(f"trackers {len(trackers)}")
    for t, tr in enumerate(trackers):
        duration = len(tr["boxes"]) if tr["duration"] is None else tr["duration"]
        text.append(f"{duration} {len(tr['boxes'])} {' '.join(rc(b) for b in tr['boxes'])} {len(tr['feat'])} "
                    f"{pt(tr['feat'])} {pt(fsets[t][0])} {by(fsets[t][1])}")

    fl = lambda a: [float(v) for v in np.asarray(a, np.float64).reshape(-1)]  # noqa: E731
    lines = []
    for o in objs:
        lines.append(["obj", o.id, "overlap", int(o.overlap_other), "nboxes", len(o.boxes), "nsets", len(o.sets)])
        lines += [["box", *b.tuple()] for b in o.boxes]
        lines += [["set", len(s), *fl(s)] for s in o.sets]
    for t, tr in enumerate(trs):
        lines.append(["trk", t, "nboxes", len(tr.boxes), "nheads", len(tr.heads)])
        lines += [["box", *b.tuple()] for b in tr.boxes] + [["head", *b.tuple()] for b in tr.heads]
        lines += [["feat", len(tr.features), *fl(tr.features)], ["tracked", len(tr.tracked), *fl(tr.tracked)]]
    lines.append(["cost", len(objs), len(trs)])
    lines += [["row", *fl(row)] for row in cost]
    return "\n".join(text) + "\n", jobs, lines, _branches(npast, feats, objs, trs, fsets, cost)


def _gate(det, tr):
    """The gate of forward_tracking's box loop (:948-970) that rejects the pair first, from the oracle's
    boxes after the run and with its Rect arithmetic; 'ok' when none does."""
    tb = tr.duration
    for b in range(min(ORC.INTERVAL, len(tr.boxes), len(det.boxes))):
        if not 0 <= tb < len(tr.boxes):
            return "duration_past_boxes"
        db, tbx = det.boxes[b], tr.boxes[tb]
        if not db.overlap(tbx):
            return "gate_overlap"
        if 1.0 < db.distance(tbx):
            return "gate_distance"
        if 0.3 > db.overlapped_area(tbx) / min(db.area(), tbx.area()):
            return "gate_area"
        if 0.5 * max(db.w, tbx.w) < math.hypot(db.center()[0] - tbx.center()[0], db.center()[1] - tbx.center()[1]):
            return "gate_center"
        tb -= 1
    return "ok"


def _branches(npast, feats, objs, trs, fsets, cost):
    took = set()
    ids = {o.id for o in objs}
    for i, f in enumerate(feats):
        if len(f) < ORC.MIN_FEATURES and i not in ids:
            took.add("det_dropped")
    for o in objs:
        kept = len(o.boxes) - 1  # chain steps kept
        if len(feats[o.id]) > ORC.MAX_FEATURES and max(len(s) for s in o.sets) <= ORC.MAX_FEATURES:
            took.add("det_capped")
        if kept == 0 and npast >= 1:
            took.add("stop_step1")
            if len(o.sets) == 1 and np.array_equal(o.sets[0], feats[o.id][:ORC.MAX_FEATURES]):
                took.add("set0_is_features")
        if kept == 1 and npast >= 2:
            took.add("stop_step2")
        if kept == 3:
            took.add("all_steps")
        if kept == 1 and npast == 1:
            took.add("one_past_frame")
        took.add("overlap_set" if o.overlap_other else "overlap_clear")
    for t, tr in enumerate(trs):
        if not tr.updated:
            assert int(fsets[t][1].sum()) < ORC.MIN_FEATURES and np.all(np.isinf(cost[:, t]))
            took.add("tracker_skipped")
    for d, o in enumerate(objs):
        open_pairs, hits = [], 0
        for t, tr in enumerate(trs):
            if not tr.updated or not tr.boxes[-1].overlap(o.box):
                continue
            hits += sum(o.box.contain(p[0], p[1]) for p in fsets[t][0])  # the raw LK output (:914-918)
            g = _gate(o, tr)
            if g == "ok":
                open_pairs.append(t)
            else:
                assert np.isinf(cost[d, t]), (d, t, g)
                took.add(g)
        if open_pairs and np.all(np.isinf(cost[d])):
            took.add("majority_clears")
        if hits and any(np.isfinite(cost[d, t]) for t in open_pairs):
            took.add("majority_keeps")
    return took


def _parse(text):
    lines = []
    for ln in text.splitlines():
        row = []
        for tok in ln.split():
            try:
                row.append(int(tok))
            except ValueError:
                try:
                    row.append(float.fromhex(tok))
                except ValueError:
                    row.append(tok)
        lines.append(row)
    return lines


def _bits(row):  # floats by their bits (-0.0 is not 0.0), everything else as it is
    return [struct.pack("<d", v) if isinstance(v, float) else v for v in row]


@pytest.fixture(scope="module")
def steps_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("flow_steps")
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no host C++ compiler")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *SAN, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = tmp / "flow_steps_check"
    srcs = [os.path.join(ROOT, "tests", "cpp", "flow_steps_check.cpp"), os.path.join(HOST, "tracker2d_steps.cpp"),
            os.path.join(HOST, "tracker2d_match.cpp")]
    objs = [str(tmp / (os.path.basename(s) + ".o")) for s in srcs]
    # no ROCm include path: the steps are plain host C++. The three units compile side by side
    # (instrumented code is most of the test's time); -O0 leaves every load and store to the sanitizers.
    # _GLIBCXX_ASSERTIONS: an index past a deque's end stays inside its block, where ASan cannot see it
    jobs = [subprocess.Popen([cxx, "-O0", "-g", "-std=c++17", "-Wall", "-Wextra", "-D_GLIBCXX_ASSERTIONS", *SAN,
                              "-I", os.path.join(ROOT, "include"),
                              "-I", HOST, "-c", s, "-o", o]) for s, o in zip(srcs, objs)]
    assert [j.wait() for j in jobs] == [0, 0, 0]
    subprocess.run([cxx, *SAN, *objs, "-o", str(exe)], check=True)
    return exe


def test_flow_steps_match_oracle_sanitized(steps_exe, tmp_path, monkeypatch):
    took_at_1 = set()
    for seed, scale, npast in CASES:
        text, jobs, want, took = _run_oracle(monkeypatch, seed, scale, npast)
        assert took <= BRANCHES
        if scale == 1.0:
            took_at_1 |= took
        case = tmp_path / f"case_{seed}.txt"
        case.write_text(text)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([str(steps_exe), str(case)], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "flow steps check: ok" in r.stdout
        got = _parse(r.stdout)[:-1]
        # the oracle runs a detection's chain to its end before the next one's, the host a step of every chain
        got_jobs = sorted(_bits(g) for g in got if g[0] == "job")
        assert got_jobs == sorted(_bits(j) for j in jobs), (seed, scale, npast)
        got = [g for g in got if g[0] != "job"]
        assert len(got) == len(want), (seed, scale, npast)
        for n, (g, w) in enumerate(zip(got, want)):
            assert _bits(g) == _bits(w), (seed, scale, npast, n, g[:6], w[:6])
    # at scale 1.0 alone, so that the scale path is an addition to the list, not a part of its cover
    assert took_at_1 == BRANCHES, sorted(BRANCHES - took_at_1)
