"""The reduced optical-flow scale (PSN_2D_OPTICALFLOW_SCALE) on the device:
the ingest resize (resize_gray_kernel, psn_lk_create_scaled) against
tests/resize_ref.py bit for bit through every push variant and overlap mode; LK,
GridFAST and the Tracker2D Run at a scale against the oracle with its SCALE set,
fed with frames resized by resize_ref; the appearance histograms still taken on
the full-size colour frame; scale 1.0 through the new entry points; errors."""
import ctypes
import os

import numpy as np
import pytest

import resize_ref
import rgbhist_ref
from mcmtt_opticalflow_amd import _lib, hip, lk, synth
from mcmtt_opticalflow_amd import tracker2d as t2d

ORC = pytest.importorskip("tracker2d_oracle")

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_WINSIZE = -1, -2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_fixtures.npz")


# ---------------------------------------------------------------------------
# 1. resize parity
# ---------------------------------------------------------------------------

def _padded_source(w, h, ch, lead, seed):
    """A random frame inside a random buffer: `lead` bytes before pixel (0, 0), a row
    stride that is no multiple of 4. -> (buffer, stride, the frame as (h, w[, 3]))."""
    stride = w * ch + 5
    if stride % 4 == 0:
        stride += 1
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, lead + h * stride + 8, dtype=np.uint8)
    rows = buf[lead:lead + h * stride].reshape(h, stride)[:, :w * ch]
    frame = np.ascontiguousarray(rows.reshape((h, w, 3) if ch == 3 else (h, w)))
    return buf, stride, frame


def _expected_levels(oracle_mod, frame, scale, nlev):
    gray = oracle_mod.bgr2gray(frame) if frame.ndim == 3 else frame
    l0 = resize_ref.resize(gray, scale)  # BGR2GRAY before the resize (:257, then :262)
    return oracle_mod.build_pyramid(l0, nlev)


def _check_levels(ctx, slot, want, what):
    for lvl, ref in enumerate(want):
        np.testing.assert_array_equal(ctx.read_level(slot, lvl), ref, err_msg=f"{what} level {lvl}")


# (200, 134, 0.3) skips source pixels; (700, 300, 0.1): a BGR tile's source columns
# do not fit the kernel's LDS rows (the direct-read path), a gray tile's do
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("w,h,scale", [(64, 48, 0.5), (645, 483, 0.5), (322, 242, 0.75), (200, 134, 0.3),
                                       (700, 300, 0.1)])
def test_resize_parity_every_push(oracle_mod, w, h, scale, ch):
    """read_level(slot, 0) = resize_ref, levels >= 1 = the oracle pyramid of that image,
    for host, async and device pushes in the OFF, STREAM and FUSED modes; the device
    frame starts 1 byte into its allocation with an odd row stride, the host frames
    have padded rows as well."""
    lw, lh = resize_ref.scaled_size(w, h, scale)
    nlev = 4 if min(lw, lh) >= 40 else 3
    pin = hip.PinnedAllocator()
    bufs = []
    try:
        with lk.LKContext(w, h, ring_slots=4, max_level_cap=nlev - 1, scale=scale) as ctx:
            assert (ctx.lk_width, ctx.lk_height) == (lw, lh) and ctx.source_size() == (w, h)
            assert ctx.get_scale() == scale
            for l in range(nlev):
                assert ctx.level_size(l) == ((lw + (1 << l) - 1) >> l, (lh + (1 << l) - 1) >> l)
            L, hnd = ctx._L, ctx.handle
            seed = 0
            for mode in (lk._lib.OVERLAP_OFF, lk._lib.OVERLAP_STREAM, lk._lib.OVERLAP_FUSED):
                ctx.set_ingest_overlap(mode)
                for push in ("host", "async", "device"):
                    seed += 1
                    lead = 1 if push == "device" else 0
                    buf, stride, frame = _padded_source(w, h, ch, lead, 1000 * ch + seed)
                    want = _expected_levels(oracle_mod, frame, scale, nlev)
                    slot = seed % 4
                    what = f"mode {mode} push {push}"
                    if push == "host":
                        ctx._check(L.psn_lk_push_frame(hnd, slot, buf.ctypes.data, stride, ch), what)
                    elif push == "async":
                        pbuf = pin(buf.shape)
                        pbuf[:] = buf
                        ctx._check(L.psn_lk_push_frame_async(hnd, slot, pbuf.ctypes.data, stride, ch), what)
                    else:
                        bufs.append(hip.DeviceBuffer.from_array(buf))
                        ctx.push_frame_device(slot, bufs[-1].addr + lead, stride, ch)
                    _check_levels(ctx, slot, want, what)
            ctx.sync()
    finally:
        for b in bufs:
            b.free()
        pin.close()


def test_resize_parity_1080p_fused_tail(oracle_mod):
    """1920 x 1080 BGR at 0.5, pushed from the device in FUSED mode: the resize runs at
    the push, the pyramid build inside the next LK launch's tail (LDS poisoned)."""
    W, H, s = 1920, 1080, 0.5
    sc = synth.make_scene(3, W, H, 64)
    frames = [synth.to_bgr(sc.frame(t)) for t in range(3)]
    for f in frames:  # colour that matters to BGR2GRAY
        f[..., 0] = np.clip(f[..., 0].astype(np.int32) + ((np.arange(W) * 7) % 61 - 30)[None, :], 0, 255)
    want = [_expected_levels(oracle_mod, f, s, 4) for f in frames]
    dev = [hip.DeviceBuffer.from_array(f) for f in frames]
    pts = (sc.points_at(0) * s).astype(np.float32)
    try:
        with lk.LKContext(W, H, ring_slots=3, max_level_cap=3, scale=s, variants={"poison_lds": 1}) as ctx:
            ctx.set_ingest_overlap(lk._lib.OVERLAP_FUSED)
            for slot in range(3):
                ctx.push_frame_device(slot, dev[slot].addr, 3 * W, 3)  # slot 2's build stays deferred
            q = [lk.make_query(0, 1, 0, len(pts), lk.make_params((21, 21), 3))]
            nxt, st, er = ctx.track(q, pts)  # builds slot 2 in its tail
            r_next, r_st, r_err = oracle_mod.calc_optical_flow_pyr_lk(want[0][0], want[1][0], pts, (21, 21), 3)
            np.testing.assert_array_equal(nxt, r_next)
            np.testing.assert_array_equal(st, r_st)
            np.testing.assert_array_equal(er, r_err)
            for slot in (2, 0, 1):
                _check_levels(ctx, slot, want[slot], f"slot {slot}")
    finally:
        for d in dev:
            d.free()


def test_resize_parity_jpeg(oracle_mod):
    z = np.load(GOLDEN)
    data, bgr = z["420_q85_rstrow_jpeg"].tobytes(), z["420_q85_rstrow_bgr"]
    H, W = bgr.shape[:2]
    for s in (0.5, 0.75):
        want = _expected_levels(oracle_mod, np.ascontiguousarray(bgr), s, 3)
        with lk.LKContext(W, H, ring_slots=2, max_level_cap=2, scale=s) as ctx:
            ctx.push_frame_jpeg(1, data)
            ctx.sync()
            _check_levels(ctx, 1, want, f"jpeg at {s}")
            # the colour source is the decoded full-size frame
            rects = np.array([(0, 0, W, H), (W // 2 + 10, 5, W, 40)], np.int32)  # (right of the LK width)
            got = ctx.box_histograms([(1, rects)])[0]
            for g, r in zip(got, rects):
                np.testing.assert_array_equal(g, rgbhist_ref.hist_counts(bgr, rgbhist_ref.clip_rect(r, W, H)))


# ---------------------------------------------------------------------------
# 2. LK on a scaled context
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("win", [(21, 21), (32, 80)])
def test_lk_on_scaled_context(oracle_mod, win):
    W, H, s = 640, 480, 0.5
    sc = synth.make_scene(11, W, H, 96)
    f0, f1 = sc.frame(0), sc.frame(1)
    r0, r1 = resize_ref.resize(f0, s), resize_ref.resize(f1, s)
    pts = (sc.points_at(0) * s).astype(np.float32)
    r_next, r_st, r_err = oracle_mod.calc_optical_flow_pyr_lk(r0, r1, pts, win, 3)
    with lk.LKContext(W, H, ring_slots=2, max_level_cap=3, scale=s, variants={"poison_lds": 1}) as ctx:
        ctx.push_frame(0, f0)
        ctx.push_frame(1, f1)
        nxt, st, er = ctx.track([lk.make_query(0, 1, 0, len(pts), lk.make_params(win, 3))], pts)
        np.testing.assert_array_equal(nxt, r_next)
        np.testing.assert_array_equal(st, r_st)
        np.testing.assert_array_equal(er, r_err)
        assert int(st.sum()) > len(pts) // 2
        # the one-shot call is calcOpticalFlowPyrLK itself: LK-size images, not resized
        nxt, st, er = ctx.calc_optical_flow_pyr_lk(r0, r1, pts, win, 3)
        np.testing.assert_array_equal(nxt, r_next)
        np.testing.assert_array_equal(st, r_st)
        np.testing.assert_array_equal(er, r_err)


# ---------------------------------------------------------------------------
# 3. Group Run at a scale vs the oracle
# ---------------------------------------------------------------------------

def _bgr(gray, seed):
    rng = np.random.default_rng(seed)
    d = rng.integers(-6, 7, gray.shape + (3,))
    return np.clip(gray[..., None].astype(np.int32) + d, 0, 255).astype(np.uint8)


def _camera_dets(sc, t, rng, s, tiny=False):
    """Detections at frame t in source coordinates (integer boxes, head boxes, a 3D
    estimate) and stand-in GridFAST points inside the SCALED boxes (the points live in
    the resized frame); optionally a 4-px-wide detection with 3 points: its scaled
    window is <= 2 px, and it is dropped before its LK call (:744)."""
    boxes, extra, feats = [], [], []
    for bx, by in sc.box_at(t):
        box = (float(np.floor(bx)), float(np.floor(by)), float(sc.box_w), float(sc.box_h))
        head = (box[0] + box[2] / 4, box[1], box[2] / 2, box[3] / 8)
        loc = (box[0] * 10.0, box[1] * 10.0, 0.0)
        n = int(rng.integers(20, 101))
        sb = [v * s for v in box]
        feats.append(np.stack([rng.uniform(sb[0] + 1, sb[0] + sb[2] - 1, n),
                               rng.uniform(sb[1] + 1, sb[1] + sb[3] - 1, n)], 1).astype(np.float32))
        boxes.append(box)
        extra.append((head, loc, 1700.0))
    if tiny:
        boxes.append((5.0, 5.0, 4.0, 30.0))
        extra.append(((5.0, 5.0, 4.0, 4.0), (0.0, 0.0, 0.0), 1700.0))
        feats.append(np.float32([[3, 5], [3.5, 7], [3.2, 11]]))
    return boxes, extra, feats


def _scaled_rois(boxes, s, lw, lh):
    """box.scale(s).cropWithSize(lw, lh).cv() (PSNWhere_Tracker2D.cpp:735-736)."""
    out = []
    for b in boxes:
        b = [v * s for v in b]
        x, y = max(0.0, b[0]), max(0.0, b[1])
        out.append((int(x), int(y), int(min(lw - x - 1, b[2])), int(min(lh - y - 1, b[3]))))
    return out


def _check_result(g_res, r_res, what):
    assert (g_res["cam_id"], g_res["frame_idx"]) == (r_res["cam_id"], r_res["frame_idx"]), what
    assert len(g_res["objects"]) == len(r_res["objects"]), what
    for go, ro in zip(g_res["objects"], r_res["objects"]):
        assert (go["id"], go["box"], go["head"], go["score"]) == (ro["id"], ro["box"], ro["head"], ro["score"]), what
        np.testing.assert_array_equal(go["prev"], ro["prev"], err_msg=what)
        np.testing.assert_array_equal(go["curr"], ro["curr"], err_msg=what)
    assert g_res["detection_rects"] == [] and g_res["tracker_rects"] == []


@pytest.mark.parametrize("ahead", [False, "two"])
@pytest.mark.parametrize("gridfast", [False, True])
@pytest.mark.parametrize("W,H,bw,bh,s", [(960, 540, 64, 160, 0.5), (640, 480, 32, 80, 0.75), (645, 483, 32, 80, 0.5)])
def test_group_run_at_scale_matches_oracle(oracle_mod, monkeypatch, gridfast, W, H, bw, bh, s, ahead):
    """test_tracker2d_group.test_group_run_matches_oracle at a scale: the oracle runs with
    SCALE = s on frames resized by resize_ref; detections, boxes, point sets, results and
    surviving trackers are compared exactly."""
    monkeypatch.setattr(ORC, "SCALE", s)
    C, T = 3, 7
    lw, lh = resize_ref.scaled_size(W, H, s)
    scenes = [synth.make_scene(40 + c, W, H, 120, nboxes=3, box_w=bw, box_h=bh, max_speed=3.0) for c in range(C)]
    refs = [ORC.CameraTracker(cam_id=10 + c) for c in range(C)]
    rngs = [np.random.default_rng(500 + c) for c in range(C)]
    grays = [[sc.frame(t) for t in range(T)] for sc in scenes]
    bgrs = [[_bgr(grays[c][t], 100 * c + t) for t in range(T)] for c in range(C)]
    per_frame = [[_camera_dets(scenes[c], t, rngs[c], s, tiny=(c == 0)) for c in range(C)] for t in range(T)]
    g_frames = [[[t2d.make_detection(b, np.zeros((0, 2), np.float32) if gridfast else f, head=e[0],
                                     location=e[1], height=e[2]) for b, e, f in zip(*per_frame[t][c])]
                 for c in range(C)] for t in range(T)]
    n_obj = n_matched = 0
    stage = 2 if ahead == "two" else 1
    with t2d.Group(W, H, [10 + c for c in range(C)], scale=s) as g:
        for f in range(stage):
            for c in range(C):  # camera 1 ingests BGR, the others gray
                g.push_frame(c, bgrs[c][f] if c == 1 else grays[c][f])
        for t in range(T):
            g.launch(t, g_frames[t], gridfast=gridfast, seed=t)
            if t + stage < T:
                for c in range(C):
                    g.push_frame(c, bgrs[c][t + stage] if c == 1 else grays[c][t + stage])
            if ahead and t + 1 < T:
                out = g.complete_next(t + 1, g_frames[t + 1], gridfast=gridfast, seed=t + 1)
            else:
                out = g.complete()
            for c in range(C):
                gray = resize_ref.resize(oracle_mod.bgr2gray(bgrs[c][t]) if c == 1 else grays[c][t], s)
                boxes, extra, feats = per_frame[t][c]
                if gridfast:
                    feats, _ = oracle_mod.gridfast_detect(gray, _scaled_rois(boxes, s, lw, lh), seed=t)
                objs, _, r_res = refs[c].run(gray, [ORC.Rect(*b) for b in boxes], feats, t,
                                             [(ORC.Rect(*e[0]), e[1], e[2]) for e in extra])
                what = f"frame {t} camera {c}"
                g_out, g_res = out[c]
                for d, f in zip(g_out, feats):
                    np.testing.assert_array_equal(t2d.points(d.features, d.num_features), f, err_msg=what)
                valid = [d for d in g_out if d.valid]
                assert len(valid) == len(objs), what
                for d, o in zip(valid, objs):
                    assert [d.boxes[i].tuple() for i in range(d.num_boxes)] == [b.tuple() for b in o.boxes], what
                    assert d.num_sets == len(o.sets), what
                    for k in range(d.num_sets):
                        np.testing.assert_array_equal(t2d.points(d.sets[k], d.set_count[k]), o.sets[k], err_msg=what)
                _check_result(g_res, r_res, what)
                g_trk = g.trackers(c)
                assert [(x.id, x.duration, x.num_boxes) for x in g_trk] == \
                       [(x.id, x.duration, len(x.boxes)) for x in refs[c].active], what
                n_obj += len(g_res["objects"])
                n_matched += sum(1 for x in refs[c].active if x.duration > 1)
    assert n_obj > 20 and n_matched >= 6  # the sequence creates and continues trackers


# ---------------------------------------------------------------------------
# 4. single camera
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("device_chain", [False, True])
def test_flow_tracker_at_scale_matches_oracle(oracle_mod, monkeypatch, device_chain):
    """FlowTracker(scale=0.5): backward and forward against ORC.backward_tracking /
    ORC.forward_tracking on the resized frames, host chain and device chain."""
    W, H, T, s = 640, 480, 3, 0.5
    monkeypatch.setattr(ORC, "SCALE", s)
    sc = synth.make_scene(21, W, H, 120, nboxes=3, box_w=32, box_h=80, max_speed=3.0)
    rng = np.random.default_rng(78)
    ring, trackers = [None] * 4, []
    n_steps = n_updated = 0
    with t2d.FlowTracker(W, H, scale=s) as ft:
        ft.set_device_chain(device_chain)
        for t in range(T):
            img = sc.frame(t)
            ft.push_frame(img)
            ring[-1] = resize_ref.resize(img, s)
            boxes, _, feats = _camera_dets(sc, t, rng, s, tiny=True)
            r_objs = ORC.backward_tracking(ring, [ORC.Rect(*b) for b in boxes], feats)
            g_trk_in = [t2d.make_tracker([b.tuple() for b in tr.boxes], tr.features, tr.duration) for tr in trackers]
            r_cost = ORC.forward_tracking(ring, trackers, r_objs) if trackers else np.zeros((len(r_objs), 0), np.float32)
            g_dets = ft.backward([t2d.make_detection(b, f) for b, f in zip(boxes, feats)])
            g_trk, g_cost = ft.forward(g_trk_in, g_dets) if g_trk_in else ([], np.zeros((len(r_objs), 0), np.float32))
            what = f"frame {t}"
            valid = [d for d in g_dets if d.valid]
            assert len(valid) == len(r_objs), what
            for d, o in zip(valid, r_objs):
                assert d.overlap_other == int(o.overlap_other), what
                assert [d.boxes[i].tuple() for i in range(d.num_boxes)] == [b.tuple() for b in o.boxes], what
                assert d.num_sets == len(o.sets), what
                for k in range(d.num_sets):
                    np.testing.assert_array_equal(t2d.points(d.sets[k], d.set_count[k]), o.sets[k], err_msg=what)
            for gt, rt in zip(g_trk, trackers):
                assert gt.updated == int(rt.updated), what
                assert [gt.boxes[i].tuple() for i in range(gt.num_boxes)] == [b.tuple() for b in rt.boxes], what
                np.testing.assert_array_equal(t2d.points(gt.features, gt.num_features), rt.features, err_msg=what)
                np.testing.assert_array_equal(t2d.points(gt.tracked, gt.num_tracked), rt.tracked, err_msg=what)
                n_updated += int(rt.updated)
            np.testing.assert_array_equal(g_cost.reshape(r_cost.shape), r_cost, err_msg=what)
            n_steps += sum(len(o.boxes) - 1 for o in r_objs)
            trackers = [ORC.Tracker([o.box], o.sets[0]) for o in r_objs]  # every detection starts a tracker
            ft.rotate()
            ring = ring[1:] + ring[:1]
    assert n_steps >= 6 and n_updated >= 4


# ---------------------------------------------------------------------------
# 5. appearance at a scale
# ---------------------------------------------------------------------------

def test_group_appearance_at_scale():
    """Group(scale=0.5).appearance counts on the full-size BGR frame: a box right of the
    LK width, and one reaching past the source frame's right edge, count what
    rgbhist_ref counts there (clipping to the LK size would lose them)."""
    W, H, s = 645, 483, 0.5
    lw, lh = resize_ref.scaled_size(W, H, s)
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    boxes = [(40.0, 30.0, 64.0, 160.0), (float(lw + 20), 100.0, 64.0, 160.0), (W - 40.0, float(lh + 10), 64.0, 160.0),
             (10.0, float(lh + 30), 50.0, 120.0)]
    dets = []
    for b in boxes:
        sb = [v * s for v in b]
        x1 = min(sb[0] + sb[2], lw - 1.0)
        f = np.stack([rng.uniform(sb[0] + 1, x1 - 1, 30), rng.uniform(sb[1] + 1, sb[1] + sb[3] - 1, 30)], 1)
        dets.append(t2d.make_detection(b, f.astype(np.float32)))
    with t2d.Group(W, H, [3], scale=s) as g:
        g.push_frame(0, frame)
        (_, res), = g.run(0, [dets])
        app, = g.appearance(0)
    assert len(res["objects"]) == len(boxes) == len(app)
    for o, rec in zip(res["objects"], app):
        rect = rgbhist_ref.appearance_rect(o["box"], W, H)
        want = rgbhist_ref.hist_counts(frame, rect)
        assert (rec["id"], rec["rect"], rec["n_pixels"]) == (o["id"], rect, rect[2] * rect[3])
        assert rec["n_pixels"] > 0
        np.testing.assert_array_equal(rec["counts"], want)
    assert [o["box"] for o in res["objects"]] == boxes  # result boxes are in source coordinates


# ---------------------------------------------------------------------------
# 6. scale 1.0 through the new entry points
# ---------------------------------------------------------------------------

def test_scale_one_is_the_unscaled_group():
    """Group(scale=1.0) (psn_t2d_group_create_scaled) and Group() (psn_t2d_group_create):
    byte-identical packed result slots over 4 frames."""
    W, H, C, T = 640, 480, 2, 4
    scenes = [synth.make_scene(60 + c, W, H, 128, nboxes=4, box_w=32, box_h=80) for c in range(C)]
    frames = [[synth.to_bgr(sc.frame(t)) if c else sc.frame(t) for t in range(T)] for c, sc in enumerate(scenes)]
    dets = [[[t2d.make_detection((float(int(x)), float(int(y)), 32.0, 80.0), sc.points_at(t)[sc.pt_box == k])
              for k, (x, y) in enumerate(sc.box_at(t))] for sc in scenes] for t in range(T)]

    def run(**kw):
        slots = []
        with t2d.Group(W, H, [7, 9], max_objects=16, **kw) as g:
            for t in range(T):
                for c in range(C):
                    g.push_frame(c, frames[c][t])
                for _, r in g.run(t, dets[t]):
                    slot = np.zeros(t2d.result_slot_bytes(16, 1), np.uint8)
                    t2d.pack_result(r, slot)
                    slots.append(slot.tobytes())
                    assert len(r["objects"]) == 4
        return slots

    assert run(scale=1.0) == run()


def test_scale_one_adds_no_launch():
    """A FUSED-mode device push of a scale-1.0 context defers its only kernel (the build
    runs inside the next LK launch): no timed push. At 0.5 the resize runs at the push."""
    W, H = 320, 240
    img = synth.texture(W, H, 9)
    d = hip.DeviceBuffer.from_array(img)
    try:
        for scale, n_fused in ((None, 0), (1.0, 0), (0.5, 3)):
            with lk.LKContext(W, H, ring_slots=2, max_level_cap=3, scale=scale) as ctx:
                ctx.enable_timing(16, 1)
                for _ in range(3):
                    ctx.push_frame_device(0, d.addr, W, 1)
                ctx.sync()
                assert ctx.timing_stats()["n_push"] == 3  # one timed push each: the resize is inside it
                ctx.set_ingest_overlap(lk._lib.OVERLAP_FUSED)
                ctx.push_frame_device(0, d.addr, W, 1)
                ctx.push_frame_device(1, d.addr, W, 1)   # flushes slot 0's build: a push launch
                ctx.track([lk.make_query(0, 0, 0, 1, lk.make_params((21, 21), 3))], np.float32([[50, 50]]))
                ctx.sync()
                # slot 0's build was flushed by the second push (1 timed push), slot 1's ran in
                # the LK launch; the scaled context adds its two resize launches
                assert ctx.timing_stats()["n_push"] == 1 + (2 if n_fused else 0), scale
    finally:
        d.free()


# ---------------------------------------------------------------------------
# 7. errors
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [float("nan"), 0.0, -0.5, 1.5])
def test_bad_scale_at_every_constructor(bad):
    with pytest.raises(lk.PsnLkError) as e:
        lk.LKContext(320, 240, scale=bad)
    assert e.value.code == ERR_ARG
    with pytest.raises(t2d.T2dError) as e:
        t2d.FlowTracker(320, 240, scale=bad)
    assert e.value.code == ERR_ARG
    with pytest.raises(t2d.T2dError) as e:
        t2d.Group(320, 240, [0, 1], scale=bad)
    assert e.value.code == ERR_ARG


def test_scaled_frame_below_one_pixel():
    with pytest.raises(lk.PsnLkError) as e:
        lk.LKContext(3, 240, scale=0.3)
    assert e.value.code == ERR_ARG


def test_jpeg_of_the_lk_size_is_refused():
    """A scaled context takes source-size JPEGs: one of the LK size fails as a
    wrong-size JPEG does on any context."""
    z = np.load(GOLDEN)
    data, bgr = z["420_q75_jpeg"].tobytes(), z["420_q75_bgr"]
    h, w = bgr.shape[:2]
    with lk.LKContext(2 * w, 2 * h, ring_slots=1, max_level_cap=1, scale=0.5) as ctx:
        assert (ctx.lk_width, ctx.lk_height) == (w, h)
        with pytest.raises(lk.PsnLkError) as e:
            ctx.push_frame_jpeg(0, data)
        assert e.value.code == ERR_ARG
    with lk.LKContext(2 * w, 2 * h, ring_slots=1, max_level_cap=1) as ctx:  # today's wrong-size failure
        with pytest.raises(lk.PsnLkError) as e2:
            ctx.push_frame_jpeg(0, data)
        assert e2.value.code == e.value.code


def test_scaled_window_too_small(monkeypatch):
    """A 4-px-wide detection has a 4 x 4 backward window at full size and a 2 x 2 one at
    0.5 (CV_Assert(winSize > 2)): with 3 features it is dropped (:744) and the frame runs;
    with 4 it fails the frame, as the oracle's LK call does."""
    W, H, s = 320, 240, 0.5
    monkeypatch.setattr(ORC, "SCALE", s)
    img = synth.texture(W, H, 3)
    small = resize_ref.resize(img, s)
    good = t2d.make_detection((20, 20, 60, 120), np.float32([[20, 20], [25, 30], [30, 40], [22, 50]]))
    few_pts, four_pts = np.float32([[3, 5], [3.5, 7], [3.2, 11]]), np.float32([[3, 5], [3.5, 7], [3.2, 11], [3.1, 9]])
    with t2d.Group(W, H, [0], scale=s) as g:
        for t in range(2):
            g.push_frame(0, img)
            (dets, res), = g.run(t, [[good, t2d.make_detection((5, 5, 4, 30), few_pts)]])
            assert [d.valid for d in dets] == [1, 0] and len(res["objects"]) == 1
        r_objs = ORC.backward_tracking([None, None, small, small], [ORC.Rect(5, 5, 4, 30)], [few_pts])
        assert r_objs == []  # the oracle drops it too
        g.push_frame(0, img)
        with pytest.raises(t2d.T2dError) as e:
            g.run(2, [[good, t2d.make_detection((5, 5, 4, 30), four_pts)]])
        assert e.value.code == ERR_WINSIZE
        with pytest.raises(Exception):
            ORC.backward_tracking([None, None, small, small], [ORC.Rect(5, 5, 4, 30)], [four_pts])
        g.push_frame(0, img)
        (dets, res), = g.run(3, [[good]])  # the group runs on
        assert dets[0].valid == 1
    with t2d.Group(W, H, [0]) as g:  # at full size the same detection has a 4 x 4 window
        g.push_frame(0, img)
        g.push_frame(0, img)
        g.run(0, [[good]])
        (dets, _), = g.run(1, [[t2d.make_detection((5, 5, 4, 30), four_pts * 2)]])
        assert dets[0].valid == 1
