"""Device time of the RGB box-histogram kernel (psn_rgbhist_device) next to the
alternative it replaces: copying the same colour frames back to pinned host
memory (a plain hipMemcpyAsync D2H; none of the histogram code).

Shapes: the headline frame-set (4 cameras x 8 boxes of 64 x 160 at 1080p), PETS-
like mixed boxes (synth.pets_box_sizes) on the same frames, one whole 4K frame.
Per shape: the counts are checked against numpy once, then HIP events time
  kernel      one psn_rgbhist_device call (memset + launch), median of single
              event-bracketed calls, and the mean of a back-to-back batch
  kernel+d2h  the same plus the 192-byte-per-box download of the counts
  frames d2h  hipMemcpyAsync of every frame of the shape to pinned memory
and a host clock times psn_lk_box_histograms end to end (descriptor upload,
launch, download, sync) on an LK context holding the frames.

usage: python tools/rgbhist_time.py [--out FILE.json] [--reps N]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mcmtt_opticalflow_amd import _lib, hip, lk, synth  # noqa: E402


def ref_counts(bgr, r):
    x, y, w, h = r
    p = bgr[y:y + h, x:x + w]
    return np.concatenate([np.bincount(p[..., c].ravel() >> 4, minlength=16) for c in (2, 1, 0)]).astype(np.uint32)


class Timer:
    def __init__(self):
        self.rt = hip.rt()
        self.rt.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        self.rt.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        self.e = [ctypes.c_void_p(), ctypes.c_void_p()]
        for e in self.e:
            hip.check(self.rt.hipEventCreate(ctypes.byref(e)), "hipEventCreate")

    def ms(self, stream, fn, calls=1):
        """Device milliseconds of `calls` x fn() enqueued on `stream`."""
        hip.check(self.rt.hipEventRecord(self.e[0], stream.ptr), "record")
        for _ in range(calls):
            fn()
        hip.check(self.rt.hipEventRecord(self.e[1], stream.ptr), "record")
        hip.check(self.rt.hipEventSynchronize(self.e[1]), "sync")
        t = ctypes.c_float()
        hip.check(self.rt.hipEventElapsedTime(ctypes.byref(t), self.e[0], self.e[1]), "elapsed")
        return t.value / calls


def stats(xs):
    xs = sorted(xs)
    return {"median_us": round(1e3 * xs[len(xs) // 2], 2), "min_us": round(1e3 * xs[0], 2),
            "p90_us": round(1e3 * xs[int(0.9 * (len(xs) - 1))], 2)}


def measure(name, frames, rects, reps, timer, stream, pinned):
    """frames: list of (H, W, 3) uint8; rects: list of (frame index, x, y, w, h)."""
    H, W = frames[0].shape[:2]
    d_frames = [hip.DeviceBuffer.from_array(f) for f in frames]
    n = len(rects)
    arr = (_lib.RgbHistRect * n)()
    for i, (f, x, y, w, h) in enumerate(rects):
        arr[i].frame, arr[i].stride = d_frames[f].addr, 3 * W
        arr[i].x, arr[i].y, arr[i].w, arr[i].h = x, y, w, h
    d_rects = hip.DeviceBuffer.from_array(np.frombuffer(bytes(arr), np.uint8))
    d_counts = hip.DeviceBuffer(n * 192)
    h_counts = pinned((n, 48 * 4))
    h_frames = [pinned(f.shape) for f in frames]

    def kernel():
        lk.rgbhist_device(d_rects.addr, n, d_counts.addr, stream.handle)

    def kernel_d2h():
        kernel()
        hip.memcpy_async(h_counts.ctypes.data, d_counts.addr, n * 192, hip.D2H, stream)

    def frames_d2h():
        for hf, df in zip(h_frames, d_frames):
            hip.memcpy_async(hf.ctypes.data, df.addr, hf.nbytes, hip.D2H, stream)

    kernel_d2h()
    stream.synchronize()
    got = h_counts.view(np.uint32).reshape(n, 48)
    for i, (f, x, y, w, h) in enumerate(rects):  # results first: a wrong kernel's time is no time
        assert np.array_equal(got[i], ref_counts(frames[f], (x, y, w, h))), (name, i)
    for fn in (kernel, kernel_d2h, frames_d2h):  # warm every path
        for _ in range(5):
            fn()
    stream.synchronize()
    out = {"rects": n, "frames": len(frames), "frame": f"{W}x{H}",
           "rect_pixels": int(sum(w * h for _, _, _, w, h in rects)),
           "frame_bytes": int(sum(f.nbytes for f in frames)), "counts_bytes": n * 192, "counts_checked": True}
    out["kernel"] = stats([timer.ms(stream, kernel) for _ in range(reps)])
    out["kernel"]["batch_mean_us"] = round(1e3 * timer.ms(stream, kernel, calls=reps), 2)
    out["kernel_plus_counts_d2h"] = stats([timer.ms(stream, kernel_d2h) for _ in range(reps)])
    out["frames_d2h"] = stats([timer.ms(stream, frames_d2h) for _ in range(max(reps // 4, 10))])
    out["frames_d2h"]["GBps"] = round(out["frame_bytes"] / (out["frames_d2h"]["median_us"] * 1e-6) / 1e9, 1)
    for b in d_frames + [d_rects, d_counts]:
        b.free()
    return out


def measure_abi(frames, rect_sets, reps):
    """Host wall time of psn_lk_box_histograms (synchronous) with the frames in an LK context's slots."""
    H, W = frames[0].shape[:2]
    with lk.LKContext(W, H, ring_slots=len(frames), max_level_cap=3) as ctx:
        for s, f in enumerate(frames):
            ctx.push_frame_async(s, f)
        ctx.sync()
        sets = [(s, np.asarray(r, np.int32)) for s, r in enumerate(rect_sets)]
        got = ctx.box_histograms(sets)
        for s, r in enumerate(rect_sets):
            for i, q in enumerate(r):
                assert np.array_equal(got[s][i], ref_counts(frames[s], q))
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ctx.box_histograms(sets)
            ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    hip.set_device(0)
    timer, stream, pinned = Timer(), hip.Stream(), hip.PinnedAllocator()
    W, H, C, B = 1920, 1080, 4, 8
    scenes = [synth.make_scene(c, W, H, 64, nboxes=B, box_w=64, box_h=160) for c in range(C)]
    frames = [synth.to_bgr(sc.frame(0)) for sc in scenes]
    head_sets = [[(min(max(int(x), 0), W - 64), min(max(int(y), 0), H - 160), 64, 160) for x, y in sc.box_at(0)]
                 for sc in scenes]
    rng = np.random.default_rng(5)
    pets_sets = []
    for c in range(C):
        ws, hs = synth.pets_box_sizes(c, B, H)
        pets_sets.append([(int(rng.integers(0, W - int(w))), int(rng.integers(0, H - int(h))), int(w), int(h))
                          for w, h in zip(ws, hs)])
    flat = lambda sets: [(c, *r) for c, rs in enumerate(sets) for r in rs]  # noqa: E731
    res = {}
    res["headline_4x8_64x160_1080p"] = measure("headline", frames, flat(head_sets), args.reps, timer, stream, pinned)
    res["pets_4x8_1080p"] = measure("pets", frames, flat(pets_sets), args.reps, timer, stream, pinned)
    big = np.random.default_rng(6).integers(0, 256, (2160, 3840, 3), dtype=np.uint8)
    res["whole_frame_4k"] = measure("4k", [big], [(0, 0, 0, 3840, 2160)], args.reps, timer, stream, pinned)
    res["headline_4x8_64x160_1080p"]["psn_lk_box_histograms_host_wall"] = measure_abi(frames, head_sets, args.reps)
    res["pets_4x8_1080p"]["psn_lk_box_histograms_host_wall"] = measure_abi(frames, pets_sets, args.reps)
    pinned.close()
    stream.destroy()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
