"""Device time of a frame-set's JPEG decode: n single psn_jpeg_decode_device calls
against one psn_jpeg_decode_batch_device of n, and a 4-camera Group's ingest
pushed per camera against push_frames_jpeg. tools/jpeg_time.py's protocol: seeded
1080p synth frames (a different frame per item), q90 4:2:0, no restart markers;
every output compared bit for bit with PIL at the timed size first; fresh
processes, --rounds rounds alternating the builds, median of the rounds'
medians, spread = max - min over the rounds; device time from HIP events around
the enqueue.

  (a) single  n psn_jpeg_decode_device calls on one decoder (both builds)
  (b) batch   one psn_jpeg_decode_batch_device of n (this tree's build)
  (c) group   n = 4: a 4-camera Group, wall time from the first host call to the
              ingest stream idle (psn_lk_sync), per-camera pushes against
              push_frames_jpeg (this tree's build)
for n = 1, 2, 4, 8. Per-kernel times: run one child under
`rocprofv3 --kernel-trace --stats` on its own (--only batch --n 4).

Build A runs (a) alone unless --a-only names more (an A that has the batch call).

usage: python tools/jpeg_batch_time.py --ab A_DIR B_DIR [--rounds 3] [--a-only single batch group] [--out profiles/jpeg_batch.json]
       python tools/jpeg_batch_time.py [--lib-dir DIR] [--only single batch group] [--n 1 2 4 8]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import jpeg_time as jt  # noqa: E402  (Timer, the frame size and quality)

NS = (1, 2, 4, 8)
CAMS = 4


def make_files(n):
    """n (restart-less file, PIL's decode as BGR), a different frame each."""
    import io

    from PIL import Image

    from mcmtt_opticalflow_amd import synth

    sc = synth.make_scene(jt.SEED, jt.W, jt.H, 64)
    out = []
    for t in range(n):
        rgb = synth.to_bgr(sc.frame(t))[..., ::-1].copy()
        rgb[..., 0] = np.clip(rgb[..., 0].astype(np.int32) + ((np.arange(jt.W) * 7) % 61 - 30)[None, :], 0, 255)
        b = io.BytesIO()
        Image.fromarray(rgb.astype(np.uint8)).save(b, "JPEG", quality=jt.QUALITY, subsampling=2)
        data = b.getvalue()
        out.append((data, np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])))
    return out


def med(xs):
    return round(1e3 * sorted(xs)[len(xs) // 2], 2)


def decoder_times(L, hip, timer, stream, files, n, batch, reps):
    from mcmtt_opticalflow_amd import _lib

    h = ctypes.c_void_p()
    assert L.psn_jpeg_create(0, ctypes.byref(h)) == 0
    try:
        assert L.psn_jpeg_set_stream(h, stream.ptr) == 0
        frame = jt.W * jt.H * 3
        d_out = hip.DeviceBuffer(n * frame)
        if batch:
            items = (_lib.JpegItem * n)()
            keep = [ctypes.create_string_buffer(f, len(f)) for f, _ in files[:n]]
            for i in range(n):
                items[i] = _lib.JpegItem(ctypes.addressof(keep[i]), len(files[i][0]), d_out.addr + i * frame, 3 * jt.W)

            def call():
                rc = L.psn_jpeg_decode_batch_device(h, items, n)
                assert rc == 0, L.psn_jpeg_last_error(h).decode()
        else:
            def call():
                for i in range(n):
                    rc = L.psn_jpeg_decode_device(h, files[i][0], len(files[i][0]), d_out.addr + i * frame, 3 * jt.W)
                    assert rc == 0, L.psn_jpeg_last_error(h).decode()

        call()
        stream.synchronize()
        got = d_out.to_array((n, jt.H, jt.W, 3), np.uint8)
        for i in range(n):  # results first: a wrong kernel's time is no time
            assert np.array_equal(got[i], files[i][1]), f"item {i} differs from PIL"
        for _ in range(5):
            call()
        stream.synchronize()
        out = {"bytes_equal_pil": True, "reps": reps, "median_us": med([timer.ms(stream, call) for _ in range(reps)])}
        d_out.free()
        return out
    finally:
        L.psn_jpeg_destroy(h)


def group_times(files, batch, reps):
    """Wall time of one frame-set's ingest of a CAMS-camera Group, host call to ingest stream idle."""
    from mcmtt_opticalflow_amd import _lib
    from mcmtt_opticalflow_amd import tracker2d as t2d

    L = _lib.load()
    fs = [f for f, _ in files[:CAMS]]
    ts = []
    with t2d.Group(jt.W, jt.H, list(range(CAMS)), max_objects=8) as g:
        lkh = g.lk_handle()
        for t in range(reps + 5):
            a = time.perf_counter()
            if batch:
                g.push_frames_jpeg(fs)
            else:
                for c in range(CAMS):
                    g.push_frame_jpeg(c, fs[c])
            assert L.psn_lk_sync(lkh) == 0
            b = time.perf_counter()
            g.run(t, [[] for _ in range(CAMS)])  # adopts the staged frames (untimed)
            if t >= 5:
                ts.append(b - a)
    return {"reps": reps, "median_us": med([1e3 * x for x in ts])}


def child(args):
    from mcmtt_opticalflow_amd import _lib

    if args.lib_dir:
        _lib.LIB_PATH = os.path.abspath(os.path.join(args.lib_dir, "libpsn_lk.so"))
    from mcmtt_opticalflow_amd import hip

    L = _lib.load()
    hip.set_device(0)
    timer, stream = jt.Timer(hip), hip.Stream()
    files = make_files(max(args.n + [CAMS]))
    res = {"lib": _lib.LIB_PATH, "file_bytes": [len(f) for f, _ in files]}
    for n in args.n:
        if "single" in args.only:
            res[f"single_n{n}"] = decoder_times(L, hip, timer, stream, files, n, False, args.reps)
        if "batch" in args.only:
            res[f"batch_n{n}"] = decoder_times(L, hip, timer, stream, files, n, True, args.reps)
    if "group" in args.only:
        res["group_per_camera"] = group_times(files, False, args.reps)
        res["group_batch"] = group_times(files, True, args.reps)
    stream.destroy()
    print(json.dumps(res))


def ab(args):
    a_dir, b_dir = args.ab
    rounds = {"A": [], "B": []}
    for r in range(args.rounds):
        for v, d, only in (("A", a_dir, args.a_only), ("B", b_dir, ["single", "batch", "group"])):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib-dir", d, "--reps", str(args.reps), "--only",
                                *only, "--n", *map(str, args.n)], capture_output=True, text=True, timeout=args.child_timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"round {r} build {v} failed ({p.returncode})")
            rounds[v].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(v, r, {k: x["median_us"] for k, x in rounds[v][-1].items() if isinstance(x, dict)}, flush=True)

    def summary(v, key):
        xs = [x[key]["median_us"] for x in rounds[v]]
        return {"runs_us": xs, "median_us": sorted(xs)[len(xs) // 2], "spread_us": round(max(xs) - min(xs), 2)}

    out = {"what": "HIP events around the enqueue (group: host wall time to ingest stream idle); A = the parent commit's "
                   "library, B = this tree's; builds alternated in one call, fresh processes",
           "frame": f"{jt.W}x{jt.H} q{jt.QUALITY} 4:2:0, no restart markers, a different frame per item",
           "rounds": args.rounds, "file_bytes": rounds["B"][0]["file_bytes"]}
    for v in "AB":
        out[v] = {k: summary(v, k) for k, x in rounds[v][0].items() if isinstance(x, dict)}
    m = lambda v, k: out[v][k]["median_us"]  # noqa: E731
    s = lambda v, k: out[v][k]["spread_us"]  # noqa: E731
    out["single_image_control"] = {"A_us": m("A", "single_n1"), "B_us": m("B", "single_n1"),
                                   "within_spreads": abs(m("A", "single_n1") - m("B", "single_n1"))
                                   <= s("A", "single_n1") + s("B", "single_n1")}
    out["ratios"] = {f"A_single_n{n}_over_B_batch_n{n}": round(m("A", f"single_n{n}") / m("B", f"batch_n{n}"), 3)
                     for n in args.n}
    if 4 in args.n:
        out["batch_of_4_faster_by_more_than_spreads"] = bool(
            m("A", "single_n4") - m("B", "batch_n4") > s("A", "single_n4") + s("B", "batch_n4"))
    out["ratios"]["group_per_camera_over_batch"] = round(m("B", "group_per_camera") / m("B", "group_batch"), 3)
    out["group_batch_faster_by_more_than_spreads"] = bool(
        m("B", "group_per_camera") - m("B", "group_batch") > s("B", "group_per_camera") + s("B", "group_batch"))
    print(json.dumps({k: out[k] for k in out if k not in "AB"}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--lib-dir", default=None)
    ap.add_argument("--only", nargs="+", default=["single", "batch", "group"])
    ap.add_argument("--n", nargs="+", type=int, default=list(NS))
    ap.add_argument("--ab", nargs=2, metavar=("A_DIR", "B_DIR"), default=None)
    ap.add_argument("--a-only", nargs="+", default=["single"], help="--ab: what build A runs (an A that has the batch call: all three)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240)
    args = ap.parse_args()
    return ab(args) if args.ab else child(args)


if __name__ == "__main__":
    main()
