#!/usr/bin/env python3
"""How the two box kernels of the Tracker2D pass fit on the CUs while they run
TOGETHER: one 64x160 forward launch (lk_kernel_fw<10, true>) on a lowest-priority
stream beside three dependent 64x64 launches (lk_kernel_bx<8, true, 128>: a
backward chain, each step from the last one's points) on a highest-priority
stream -- Tracker2DFlow's stream priorities (host/tracker2d_pass.cpp) -- enqueued
together. One LK context, the synthetic 1080p scene, 2048 points, maxLevel 3, the
reference's criteria (30, 0.01). Prints one JSON line.

  python tools/bx_pack.py --reps 40                      # the median span of the set (HIP events) + checksums
  python tools/bx_pack.py --variants bx_pack=1           # the planned LDS requests, not the CU slots
  python tools/bx_pack.py --order forward-first          # the forward launch enqueued before the chain
  python tools/bx_pack.py --lib mcmtt_opticalflow_amd/lib/libpsn_lk_stamps.so --sets 10
      # the diagnostic build: residency from stamps 16-18 of both kernels (start /
      # end on the 100 MHz clock, HW_ID, XCC_ID), per set and per CU over time

Residency (stamps build). A CU holds 12 waves of these builds (3 per SIMD at 136-168
VGPRs) and 160 KB of LDS; a forward workgroup is 4 waves (one per SIMD), a two-wave
workgroup 2. Over the set's span, per CU: the resident workgroups of each kind, the
wave slots and LDS bytes in use, and the PACKING LOSS: the share of CU-time in which
the CU had 4 free wave slots (a free one on every SIMD when they are spread evenly:
the stamps hold thread 0's SIMD only) and at least 27 KB of free LDS while
workgroups were still undispatched (before the last workgroup start of the set).
A dependent chain launch cannot start before its predecessor ends, so the loss
includes the chain's own launch boundaries: compare builds, not against zero.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mcmtt_opticalflow_amd import _lib, hip, lk, synth  # noqa: E402

CU_LDS = 160 * 1024
CU_WAVES = 12            # 3 waves per SIMD at 136-168 VGPRs
PLANNED = {"bx": 25920, "fw": 52416}  # the launches' LDS: BxLayout(64, 64, 8, 1, 16).total, BxLayout(64, 160, 10).total
SLOT, SLOTS = 26 * 1024, {"bx": 1, "fw": 2}  # kBxLdsSlot, bx_lds_slots (psn_lk_kernels.h)
WAVES = {"bx": 2, "fw": 4}


class Rt:
    """The few HIP calls this tool adds to mcmtt_opticalflow_amd.hip: priority streams, timed events."""

    def __init__(self):
        h = hip.rt()
        vp, ip = ctypes.c_void_p, ctypes.c_int
        h.hipDeviceGetStreamPriorityRange.argtypes = [ctypes.POINTER(ip), ctypes.POINTER(ip)]
        h.hipStreamCreateWithPriority.argtypes = [ctypes.POINTER(vp), ctypes.c_uint, ip]
        h.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
        h.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
        h.hipStreamWaitEvent.argtypes = [vp, vp, ctypes.c_uint]
        self.h = h
        least, greatest = ip(), ip()
        hip.check(h.hipDeviceGetStreamPriorityRange(ctypes.byref(least), ctypes.byref(greatest)), "priority range")
        self.least, self.greatest = least.value, greatest.value

    def stream(self, priority):
        s = ctypes.c_void_p()
        hip.check(self.h.hipStreamCreateWithPriority(ctypes.byref(s), hip.STREAM_NON_BLOCKING, priority), "stream")
        return s

    def event(self):
        e = ctypes.c_void_p()
        hip.check(self.h.hipEventCreate(ctypes.byref(e)), "hipEventCreate")
        return e

    def record(self, e, s):
        hip.check(self.h.hipEventRecord(e, s), "hipEventRecord")

    def wait(self, s, e):
        hip.check(self.h.hipStreamWaitEvent(s, e, 0), "hipStreamWaitEvent")

    def elapsed_ms(self, e0, e1):
        hip.check(self.h.hipEventSynchronize(e1), "hipEventSynchronize")
        ms = ctypes.c_float()
        hip.check(self.h.hipEventElapsedTime(ctypes.byref(ms), e0, e1), "hipEventElapsedTime")
        return float(ms.value)


def residency(stamps, requests):
    """stamps: [(kind, (npts, 64) int64)] of one set's launches. -> the set's residency record."""
    kind, r0, r1, cu = [], [], [], []
    for k, s in stamps:
        ok = s[:, 17] > 0
        hw = s[ok, 18]
        hwid, xcc = hw & 0xffffffff, hw >> 32
        cu.append((xcc << 16) | (((hwid >> 13) & 7) << 8) | (((hwid >> 12) & 1) << 4) | ((hwid >> 8) & 15))
        r0.append(s[ok, 16])
        r1.append(s[ok, 17])
        kind.append(np.full(int(ok.sum()), 0 if k == "bx" else 1))
    kind, r0, r1, cu = (np.concatenate(a) for a in (kind, r0, r1, cu))
    t0, t1, last_start = int(r0.min()), int(r1.max()), int(r0.max())
    span = t1 - t0
    cus = np.unique(cu)
    wv = np.array([WAVES["bx"], WAVES["fw"]])
    by = np.array([requests["bx"], requests["fw"]])
    loss = busy_w = busy_l = 0
    res_t = np.zeros(2)
    mx = np.zeros(2, int)
    first = {"bx": 0, "fw": 0}
    hist = {}
    for c in cus:
        m = cu == c
        ev = sorted([(int(a), 1, int(k)) for a, k in zip(r0[m], kind[m])] + [(int(b), -1, int(k)) for b, k in zip(r1[m], kind[m])],
                    key=lambda e: (e[0], e[1]))
        first["bx" if min(ev)[2] == 0 else "fw"] += 1
        n = np.zeros(2, int)
        last = t0
        for t, d, k in ev + [(t1, 0, 0)]:
            dt = t - last
            if dt > 0:
                waves, lds = int(n @ wv), int(n @ by)
                busy_w += waves * dt
                busy_l += lds * dt
                res_t += n * dt
                key = f"{n[1]}fw+{n[0]}bx"
                hist[key] = hist.get(key, 0) + dt
                if CU_WAVES - waves >= 4 and CU_LDS - lds >= 27 * 1024:
                    loss += max(0, min(t, last_start) - last)
            n[k] += d
            mx = np.maximum(mx, n)
            last = t
    cu_time = len(cus) * max(span, 1)
    top = sorted(hist.items(), key=lambda kv: -kv[1])[:8]
    return {"span_us": round(span / 100.0, 1), "cus": int(len(cus)),
            "packing_loss": round(loss / cu_time, 4),
            "wave_slots_in_use": round(busy_w / cu_time / CU_WAVES, 4), "lds_in_use": round(busy_l / cu_time / CU_LDS, 4),
            "resident_mean": {"bx": round(res_t[0] / cu_time, 3), "fw": round(res_t[1] / cu_time, 3)},
            "resident_max": {"bx": int(mx[0]), "fw": int(mx[1])},
            "first_on_cu": first, "last_start_us": round((last_start - t0) / 100.0, 1),
            "cu_time_by_mix": {k: round(v / cu_time, 4) for k, v in top}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--sets", type=int, default=10, help="stamps build: sets whose residency is read")
    ap.add_argument("--lib", default=None, help="a libpsn_lk.so build (default: the product library); a stamps build adds residency")
    ap.add_argument("--variants", default="", help="context variants, e.g. bx_pack=1")
    ap.add_argument("--lds", default="", help="residency: the LDS requests of an experimental build, e.g. bx=26624,fw=53248")
    ap.add_argument("--order", default="chains-first", choices=["chains-first", "forward-first"])
    ap.add_argument("--flags", type=lambda v: int(v, 0), default=0)
    args = ap.parse_args()
    variants = {k: int(v) for k, v in (kv.split("=") for kv in args.variants.split(",") if kv)}
    n = args.points
    sc = synth.make_scene(0, 1920, 1080, n, nboxes=8)
    f0, f1 = sc.frame(0), sc.frame(1)
    pts = np.ascontiguousarray(sc.points_at(1), np.float32)
    L = _lib.load(args.lib)
    rt = Rt()
    lo, hi = rt.stream(rt.least), rt.stream(rt.greatest)
    d_prev = hip.DeviceBuffer.from_array(pts)
    # the forward launch's outputs, then the chain's three steps (step k reads step k-1's points)
    d_next = [hip.DeviceBuffer(8 * n) for _ in range(4)]
    d_st = [hip.DeviceBuffer(n) for _ in range(4)]
    d_err = [hip.DeviceBuffer(4 * n) for _ in range(4)]
    out = {"points": n, "reps": args.reps, "variants": variants, "order": args.order, "flags": args.flags,
           "lib": os.path.relpath(args.lib, ROOT) if args.lib else "product"}
    with lk.LKContext(1920, 1080, ring_slots=2, max_level_cap=3) as ctx:
        for k, v in variants.items():
            ctx.set_variant(k, v)
        requests = {k: max(v, SLOTS[k] * SLOT) if variants.get("bx_pack", 0) == 0 else v for k, v in PLANNED.items()}
        if "bx_pack" not in variants:
            try:
                ctx.set_variant("bx_pack", 0)
            except _lib.PsnLkError:  # a build from before the slots: the planned requests
                requests = dict(PLANNED)
        requests.update({k: int(v) for k, v in (kv.split("=") for kv in args.lds.split(",") if kv)})
        out["lds_requests"] = requests
        ctx.push_frame(0, f0)
        ctx.push_frame(1, f1)
        ctx.sync()
        stamped = L.psn_lk_debug_set_stamps(ctx.handle, None) == 0
        d_stamps = [hip.DeviceBuffer(n * 64 * 8) for _ in range(4)] if stamped else None
        p_fw, p_bx = lk.make_params((64, 160), 3, flags=args.flags), lk.make_params((64, 64), 3, flags=args.flags)
        q_fw = lk.query_array([lk.make_query(1, 0, 0, n, p_fw)])
        q_bx = [lk.query_array([lk.make_query(1 - (k & 1), k & 1, 0, n, p_bx)]) for k in range(3)]
        e0, e1, el = rt.event(), rt.event(), rt.event()

        def forward():
            ctx.set_stream(lo.value)
            if stamped:
                L.psn_lk_debug_set_stamps(ctx.handle, d_stamps[0].addr)
            ctx.track_device(q_fw, d_prev.addr, d_next[0].addr, d_st[0].addr, d_err[0].addr)

        def chain():
            ctx.set_stream(hi.value)
            for k in range(3):
                if stamped:
                    L.psn_lk_debug_set_stamps(ctx.handle, d_stamps[1 + k].addr)
                src = d_prev if k == 0 else d_next[k]
                ctx.track_device(q_bx[k], src.addr, d_next[1 + k].addr, d_st[1 + k].addr, d_err[1 + k].addr)

        def one_set():
            rt.record(e0, hi)
            rt.wait(lo, e0)
            for part in ((chain, forward) if args.order == "chains-first" else (forward, chain)):
                part()
            rt.record(el, lo)
            rt.wait(hi, el)
            rt.record(e1, hi)
            return rt.elapsed_ms(e0, e1)

        for _ in range(3):
            one_set()
        if stamped:
            sets = []
            for _ in range(args.sets):
                for b in d_stamps:
                    b.zero()
                ms = one_set()
                hip.synchronize()
                st = [("fw" if i == 0 else "bx", b.to_array((n, 64), np.uint64).astype(np.int64)) for i, b in enumerate(d_stamps)]
                sets.append(residency(st, requests) | {"event_span_us": round(1e3 * ms, 1)})
            out["sets"] = sets
            loss = np.array([s["packing_loss"] for s in sets])
            out["packing_loss"] = {"median": round(float(np.median(loss)), 4), "min": round(float(loss.min()), 4),
                                   "max": round(float(loss.max()), 4), "sorted": sorted(round(float(v), 4) for v in loss)}
            out["span_us_median"] = round(float(np.median([s["span_us"] for s in sets])), 1)
        else:
            ms = np.array([one_set() for _ in range(args.reps)])
            out["span_us"] = {"median": round(1e3 * float(np.median(ms)), 1), "mean": round(1e3 * float(ms.mean()), 1),
                              "min": round(1e3 * float(ms.min()), 1), "max": round(1e3 * float(ms.max()), 1)}
        hip.synchronize()
        res = []
        for i in range(4):
            res += [d_next[i].to_array((n, 2), np.float32), d_st[i].to_array((n,), np.uint8)]
        out["next_status_sha"] = hashlib.sha1(b"".join(a.tobytes() for a in res)).hexdigest()[:16]
        out["tracked"] = [int(res[2 * i + 1].sum()) for i in range(4)]
        ctx.set_stream(None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
