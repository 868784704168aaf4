"""Device time of psn_jpeg_decode_device on one seeded 1080p synth frame (q90,
4:2:0) saved twice: without restart markers -- the parallel entropy path
(jpeg_sync / chain / emit / dc kernels) -- and with restart_marker_rows=1 -- the
serial path, one thread per restart segment (what bench.py --ingest jpeg times).

Per file and configuration the output is first compared bit for bit with PIL's
decode at the timed size, then HIP events time
  single   one psn_jpeg_decode_device call (H2D of the file, memset, kernels),
           median / min / p90 of event-bracketed calls after warm-up
  batch    the mean of a back-to-back batch
The new build also sweeps the subsequence size (64 / 128 / 256 bytes) and runs
the restart-less file on the serial kernel (debug entropy mode 1).

One process times one build. --ab A_DIR B_DIR starts fresh child processes that
alternate two builds (A: the older one, B: the tree's) for --rounds rounds in
one call, and writes the per-round figures, their spread and the ratios.
Per-kernel times: run a child under `rocprofv3 --kernel-trace --stats` on its own.

usage: python tools/jpeg_time.py [--lib-dir DIR] [--reps N] [--only KEY...] [--out FILE.json]
       python tools/jpeg_time.py --ab A_DIR B_DIR [--rounds R] [--only KEY...] [--out profiles/jpeg_entropy.json]
"""
import argparse
import ctypes
import io
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, SEED, QUALITY = 1920, 1080, 6, 90


def make_files():
    """(restart-less file, restart-per-row file, PIL's decode of each as BGR)."""
    from PIL import Image

    from mcmtt_opticalflow_amd import synth

    sc = synth.make_scene(SEED, W, H, 64)
    rgb = synth.to_bgr(sc.frame(1))[..., ::-1].copy()
    rgb[..., 0] = np.clip(rgb[..., 0].astype(np.int32) + ((np.arange(W) * 7) % 61 - 30)[None, :], 0, 255)
    rgb = rgb.astype(np.uint8)
    out = {}
    for name, opt in (("restartless", {}), ("restart_rows", {"restart_marker_rows": 1})):
        b = io.BytesIO()
        Image.fromarray(rgb).save(b, "JPEG", quality=QUALITY, subsampling=2, **opt)
        data = b.getvalue()
        ref = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])
        out[name] = (data, ref)
    return out


class Timer:
    def __init__(self, hip):
        self.hip, self.rt = hip, hip.rt()
        self.rt.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        self.rt.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        self.e = [ctypes.c_void_p(), ctypes.c_void_p()]
        for e in self.e:
            hip.check(self.rt.hipEventCreate(ctypes.byref(e)), "hipEventCreate")

    def ms(self, stream, fn, calls=1):
        """Device milliseconds of `calls` x fn() enqueued on `stream`."""
        self.hip.check(self.rt.hipEventRecord(self.e[0], stream.ptr), "record")
        for _ in range(calls):
            fn()
        self.hip.check(self.rt.hipEventRecord(self.e[1], stream.ptr), "record")
        self.hip.check(self.rt.hipEventSynchronize(self.e[1]), "sync")
        t = ctypes.c_float()
        self.hip.check(self.rt.hipEventElapsedTime(ctypes.byref(t), self.e[0], self.e[1]), "elapsed")
        return t.value / calls


def stats(xs):
    xs = sorted(xs)
    return {"median_us": round(1e3 * xs[len(xs) // 2], 2), "min_us": round(1e3 * xs[0], 2),
            "p90_us": round(1e3 * xs[int(0.9 * (len(xs) - 1))], 2)}


def measure(L, hip, timer, stream, data, ref, mode, sub, reps):
    from mcmtt_opticalflow_amd import _lib

    h = ctypes.c_void_p()
    assert L.psn_jpeg_create(0, ctypes.byref(h)) == 0
    try:
        assert L.psn_jpeg_set_stream(h, stream.ptr) == 0
        if mode or sub:
            assert L.psn_jpeg_debug_set_entropy(h, mode, sub) == 0
        d_out = hip.DeviceBuffer(W * H * 3)

        def call():
            rc = L.psn_jpeg_decode_device(h, data, len(data), d_out.ptr, 3 * W)
            assert rc == 0, L.psn_jpeg_last_error(h).decode()

        call()
        stream.synchronize()
        got = d_out.to_array((H, W, 3), np.uint8)
        assert np.array_equal(got, ref), "decode differs from PIL"  # results first: a wrong kernel's time is no time
        out = {"bytes_equal_pil": True}
        if hasattr(L, "psn_jpeg_last_stats"):
            s = _lib.JpegStats()
            assert L.psn_jpeg_last_stats(h, ctypes.byref(s)) == 0
            out["stats"] = _lib.struct_dict(s)
        t1 = timer.ms(stream, call)  # sizes the repetitions: the older build's restart-less decode is slow
        n = max(5, min(reps, int(2000.0 / max(t1, 1e-3))))
        for _ in range(min(5, n)):
            call()
        stream.synchronize()
        out["reps"] = n
        out["single"] = stats([timer.ms(stream, call) for _ in range(n)])
        out["batch_mean_us"] = round(1e3 * timer.ms(stream, call, calls=n), 2)
        d_out.free()
        return out
    finally:
        L.psn_jpeg_destroy(h)


def child(args):
    from mcmtt_opticalflow_amd import _lib

    if args.lib_dir:  # another build of the library (A/B)
        _lib.LIB_PATH = os.path.abspath(os.path.join(args.lib_dir, "libpsn_lk.so"))
    from mcmtt_opticalflow_amd import hip

    L = _lib.load()
    hip.set_device(0)
    timer, stream = Timer(hip), hip.Stream()
    files = make_files()
    new = hasattr(L, "psn_jpeg_debug_set_entropy")
    res = {"lib": _lib.LIB_PATH, "parallel_path": new, "frame": f"{W}x{H}", "quality": QUALITY, "subsampling": "4:2:0",
           "file_bytes": {k: len(v[0]) for k, v in files.items()}}
    runs = [("restart_rows", "restart_rows", 0, 0), ("restartless", "restartless", 0, 0)]
    if new:
        runs += [(f"restartless_sub{s}", "restartless", 2, s) for s in (64, 128, 256)]
        runs += [("restartless_serial_kernel", "restartless", 1, 0)]
    for key, f, mode, sub in runs:
        if args.only and key not in args.only:
            continue
        res[key] = measure(L, hip, timer, stream, files[f][0], files[f][1], mode, sub, args.reps)
    stream.destroy()
    print(json.dumps(res))
    return res


def ab(args):
    a_dir, b_dir = args.ab
    rounds = {"A": [], "B": []}
    for r in range(args.rounds):
        for v, d in (("A", a_dir), ("B", b_dir)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib-dir", d, "--reps", str(args.reps),
                                *(["--only", *args.only] if args.only else [])],
                               capture_output=True, text=True, timeout=args.child_timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"round {r} build {v} failed ({p.returncode})")
            rounds[v].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(v, r, {k: x["single"]["median_us"] for k, x in rounds[v][-1].items() if isinstance(x, dict) and "single" in x})

    def series(v, key, what):
        return [x[key]["single"]["median_us"] if what == "single" else x[key]["batch_mean_us"] for x in rounds[v] if key in x]

    def summary(xs):
        return {"runs_us": xs, "median_us": sorted(xs)[len(xs) // 2], "spread_us": round(max(xs) - min(xs), 2)}

    out = {"what": "psn_jpeg_decode_device, HIP events; A = older build, B = this tree; builds alternated in one call",
           "frame": f"{W}x{H} q{QUALITY} 4:2:0", "rounds": args.rounds, "file_bytes": rounds["B"][0]["file_bytes"],
           "stats": {k: x.get("stats") for k, x in rounds["B"][0].items() if isinstance(x, dict) and "stats" in x}}
    for v in "AB":
        out[v] = {key: {"single": summary(series(v, key, "single")), "batch": summary(series(v, key, "batch"))}
                  for key in rounds[v][0] if isinstance(rounds[v][0][key], dict) and "single" in rounds[v][0][key]}
    med = lambda v, key, w="single": out[v][key][w]["median_us"]  # noqa: E731
    out["ratios"] = {
        "restartless_A_over_B_single": round(med("A", "restartless") / med("B", "restartless"), 2),
        "restartless_A_over_B_batch": round(med("A", "restartless", "batch") / med("B", "restartless", "batch"), 2),
        "B_restartless_over_restart_rows_single": round(med("B", "restartless") / med("B", "restart_rows"), 3),
        "B_restartless_over_restart_rows_batch": round(med("B", "restartless", "batch") / med("B", "restart_rows", "batch"), 3),
        "restart_rows_A_over_B_single": round(med("A", "restart_rows") / med("B", "restart_rows"), 3),
    }
    print(json.dumps(out["ratios"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--lib-dir", default=None)
    ap.add_argument("--only", nargs="+", default=None, help="configurations to run (a kernel trace of one path)")
    ap.add_argument("--ab", nargs=2, metavar=("A_DIR", "B_DIR"), default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240)
    args = ap.parse_args()
    if args.ab:
        return ab(args)
    res = child(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
