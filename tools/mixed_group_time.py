#!/usr/bin/env python3
"""What one group of cameras with different frame sizes buys.

Workload: the PETS2009 S2.L1 views {1, 5, 7} -- 768x576 + 2 x 720x576 -- with
PETS-like box sizes (synth.pets_box_sizes), GridFAST features, frames uploaded two
ahead and pipelined with complete_next as bench.py drives a group. Three drivers
of the same cameras, run in turn `--rounds` times in one process on one GPU:

  mixed      one Group.with_sizes: two frame classes in one LK context, the cameras'
             launches split per (kernel, frame class)
  per_size   one Group per frame size (768x576: 1 camera, 720x576: 2 cameras), what
             the library could do before frame classes; per step every group's
             launch, then every group's uploads, then every group's complete_next,
             so that the groups' device work overlaps
  equal      three 768x576 cameras in one Group: one frame class, no split launches
             (more pixels than the mixed workload: the cost of the split shows as
             mixed being slower than equal by more than the pixel difference)

Per run: wall seconds of `--steps` steps after `--warmup`, ending in the last
frame's complete (it waits for the device), as camera-frames per second. The JSON
holds every run, the median per driver and the spread (max - min) / median.
A missing GPU is an error: nothing here falls back.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIEWS = [(768, 576), (720, 576), (720, 576)]


def feed_args(w, h, a):
    return argparse.Namespace(width=w, height=h, points=a.points, boxes=a.boxes, box_dist="pets", period=a.period,
                              features="gridfast", ingest="host")


class Driver:
    """Groups and the cameras each one takes: [(group, [feed, ...]), ...]."""

    def __init__(self, name, parts):
        self.name, self.parts = name, parts

    def close(self):
        for g, _ in self.parts:
            g.close()

    def run(self, t2d, steps, warmup):
        ahead, total = 2, warmup + steps
        for f in range(ahead):
            for g, feeds in self.parts:
                for k, fd in enumerate(feeds):
                    fd.push(g, k, f)
        dets = {t: [[fd.detections(t2d, t) for fd in feeds] for _, feeds in self.parts] for t in range(total + 1)}
        recs = {t: [g.records(d) for (g, _), d in zip(self.parts, dets[t])] for t in range(total + 1)}
        t0 = None
        for t in range(total):
            if t == warmup:
                t0 = time.perf_counter()
            for i, (g, _) in enumerate(self.parts):
                g.launch(t, recs[t][i], gridfast=True, seed=t)
            for g, feeds in self.parts:
                for k, fd in enumerate(feeds):
                    fd.push(g, k, t + ahead)
            for i, (g, _) in enumerate(self.parts):
                if t + 1 < total:
                    g.complete_next(t + 1, recs[t + 1][i], gridfast=True, seed=t + 1, raw=True)
                else:
                    g.complete_raw()
        dt = time.perf_counter() - t0
        objects = sum(g.result_struct(k).num_objects for g, feeds in self.parts for k in range(len(feeds)))
        return dt, objects


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--boxes", type=int, default=10)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--period", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_sizes.json"))
    a = ap.parse_args()

    import bench
    from mcmtt_opticalflow_amd import hip
    from mcmtt_opticalflow_amd import tracker2d as t2d

    hip.set_device(0)
    pinned = bench.pinned_allocator("hip")
    # camera ids 0..2: the same scenes (seeded by the id and the size) in every driver that shows that size
    mixed_feeds = [bench.CameraFeed(c, feed_args(w, h, a), pinned) for c, (w, h) in enumerate(VIEWS)]
    equal_feeds = [mixed_feeds[0]] + [bench.CameraFeed(c, feed_args(*VIEWS[0], a), pinned) for c in (1, 2)]
    max_obj = 2 * a.boxes

    def make(name):
        if name == "mixed":
            return Driver(name, [(t2d.Group.with_sizes(VIEWS, [0, 1, 2], max_objects=max_obj), mixed_feeds)])
        if name == "per_size":
            return Driver(name, [(t2d.Group(*VIEWS[0], [0], max_objects=max_obj), mixed_feeds[:1]),
                                 (t2d.Group(*VIEWS[1], [1, 2], max_objects=max_obj), mixed_feeds[1:])])
        return Driver(name, [(t2d.Group(*VIEWS[0], [0, 1, 2], max_objects=max_obj), equal_feeds)])

    names = ["mixed", "per_size", "equal"]
    runs = {n: [] for n in names}
    objects = {}
    for r in range(a.rounds):
        for n in names:  # alternating: a drift of the machine falls on every driver alike
            d = make(n)
            try:
                dt, nobj = d.run(t2d, a.steps, a.warmup)
            finally:
                d.close()
            runs[n].append(round(3 * a.steps / dt, 1))
            objects[n] = nobj
            print(f"round {r} {n}: {runs[n][-1]} camera-frames/s ({nobj} objects in the last frame)", flush=True)
    out = {"workload": {"views": VIEWS, "equal_views": [VIEWS[0]] * 3, "boxes_per_camera": a.boxes, "box_dist": "pets",
                        "features": "gridfast", "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
                        "frames_ahead": 2, "unit": "camera-frames/s (3 cameras x steps / wall seconds)"},
           "runs": runs, "last_frame_objects": objects,
           "median": {n: statistics.median(v) for n, v in runs.items()},
           "spread": {n: round((max(v) - min(v)) / statistics.median(v), 4) for n, v in runs.items()}}
    m = out["median"]
    out["mixed_over_per_size"] = round(m["mixed"] / m["per_size"], 4)
    out["mixed_over_equal"] = round(m["mixed"] / m["equal"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("median", "spread", "mixed_over_per_size", "mixed_over_equal")}))


if __name__ == "__main__":
    main()
