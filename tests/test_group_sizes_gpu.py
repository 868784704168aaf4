"""A Tracker2D group whose cameras have their own frame sizes
(psn_t2d_group_create_sizes, include/psn_tracker2d.h; Group.with_sizes) against
oracle/tracker2d_oracle.py's CameraTracker, one per camera on that camera's own
frames -- the reference sizes every CPSNWhere_Tracker2D from its own camera.

The method is tests/test_tracker2d_group.py::test_group_run_matches_oracle's with a
W, H per camera: detections (features), boxes, point sets, result objects and the
surviving trackers, bit for bit, through the given-features and the GridFAST
path, plain and pipelined (frames staged two ahead, complete_next). The cameras
share their box size, so consecutive queries of cameras in different frame
classes have the same plan: a merge of counted sub-queries across classes, or a
launch with the other class's ring geometry (pitch 512 against 256, a 32x80
window's max level 1 against 0), would show in the bits.
"""
import ctypes

import numpy as np
import pytest

import resize_ref
import rgbhist_ref
from mcmtt_opticalflow_amd import _lib, synth
from mcmtt_opticalflow_amd import tracker2d as t2d

ORC = pytest.importorskip("tracker2d_oracle")

pytestmark = pytest.mark.gpu

ERR_ARG = -1


def _bgr(gray, seed):
    rng = np.random.default_rng(seed)
    d = rng.integers(-6, 7, gray.shape + (3,))
    return np.clip(gray[..., None].astype(np.int32) + d, 0, 255).astype(np.uint8)


def _camera_dets(sc, t, rng, s):
    """Detections at frame t in source coordinates and stand-in GridFAST points inside
    the boxes scaled by s (the points live in the LK frame)."""
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
    return boxes, extra, feats


def _scaled_rois(boxes, s, lw, lh):
    """box.scale(s).cropWithSize(lw, lh).cv() (PSNWhere_Tracker2D.cpp:735-736), the camera's own lw x lh."""
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


def _run_against_oracle(oracle_mod, sizes, bw, bh, s, gridfast, ahead, T=6):
    """-> per camera (result objects over the sequence, trackers continued past their first frame)."""
    C = len(sizes)
    lks = [resize_ref.scaled_size(w, h, s) for w, h in sizes]
    scenes = [synth.make_scene(40 + c, w, h, 120, nboxes=3, box_w=bw, box_h=bh, max_speed=3.0)
              for c, (w, h) in enumerate(sizes)]
    refs = [ORC.CameraTracker(cam_id=10 + c) for c in range(C)]
    rngs = [np.random.default_rng(500 + c) for c in range(C)]
    grays = [[sc.frame(t) for t in range(T)] for sc in scenes]
    bgrs = [[_bgr(grays[c][t], 100 * c + t) for t in range(T)] for c in range(C)]
    per_frame = [[_camera_dets(scenes[c], t, rngs[c], s) for c in range(C)] for t in range(T)]
    g_frames = [[[t2d.make_detection(b, np.zeros((0, 2), np.float32) if gridfast else f, head=e[0],
                                     location=e[1], height=e[2]) for b, e, f in zip(*per_frame[t][c])]
                 for c in range(C)] for t in range(T)]
    n_obj, n_cont = [0] * C, [0] * C
    stage = 2 if ahead == "two" else 1
    with t2d.Group.with_sizes(sizes, [10 + c for c in range(C)], scale=None if s == 1.0 else s) as g:
        assert [g.camera_size(c) for c in range(C)] == [sz + lk_ for sz, lk_ in zip(sizes, lks)]
        for f in range(stage):
            for c in range(C):  # camera 1 ingests BGR, the others gray
                g.push_frame(c, bgrs[c][f] if c == 1 else grays[c][f])
        for t in range(T):
            g.launch(t, g_frames[t], gridfast=gridfast, seed=t)
            if t + stage < T:  # frame t+stage is uploaded while frame t runs
                for c in range(C):
                    g.push_frame(c, bgrs[c][t + stage] if c == 1 else grays[c][t + stage])
            if ahead and t + 1 < T:
                out = g.complete_next(t + 1, g_frames[t + 1], gridfast=gridfast, seed=t + 1)
            else:
                out = g.complete()
            for c in range(C):
                gray = oracle_mod.bgr2gray(bgrs[c][t]) if c == 1 else grays[c][t]
                if s != 1.0:
                    gray = resize_ref.resize(gray, s)
                assert gray.shape == lks[c][::-1]
                boxes, extra, feats = per_frame[t][c]
                if gridfast:
                    feats, _ = oracle_mod.gridfast_detect(gray, _scaled_rois(boxes, s, *lks[c]), seed=t)
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
                n_obj[c] += len(g_res["objects"])
                n_cont[c] = max(n_cont[c], sum(1 for x in refs[c].active if x.duration > 1))
    return n_obj, n_cont


@pytest.mark.parametrize("ahead", [False, "two"])
@pytest.mark.parametrize("gridfast", [False, True])
def test_mixed_sizes_match_oracle(oracle_mod, gridfast, ahead):
    """Sizes 320x240 + 2 x 200x150 (two frame classes, the second with two cameras),
    boxes 32x80 in every camera: forward windows 32x80 (box kernel), backward 32x32
    (single-tile kernel), both in both classes, on the device chain (counted,
    merged sub-queries: camera 0's and camera 1's queries have equal plans)."""
    n_obj, n_cont = _run_against_oracle(oracle_mod, [(320, 240), (200, 150), (200, 150)], 32, 80, 1.0, gridfast, ahead)
    assert min(n_obj) >= 12 and min(n_cont) >= 1, (n_obj, n_cont)


@pytest.mark.parametrize("gridfast,ahead", [(False, False), (True, "two")])
def test_pets_halves_at_scale_match_oracle(oracle_mod, monkeypatch, gridfast, ahead):
    """384x288 + 2 x 360x288 at scale 0.5 (the halves of PETS2009's 768x576 and 720x576
    views): LK sizes 192x144 and 180x144, boxes 48x112 -> windows 24x56 and 24x24."""
    monkeypatch.setattr(ORC, "SCALE", 0.5)
    n_obj, n_cont = _run_against_oracle(oracle_mod, [(384, 288), (360, 288), (360, 288)], 48, 112, 0.5, gridfast, ahead)
    assert min(n_obj) >= 12 and min(n_cont) >= 1, (n_obj, n_cont)


def test_appearance_crops_per_camera():
    """The same box in a 320x240 and a 200x150 camera, past the narrow one's right edge
    and inside the wide one's: each appearance rect is cropped with its camera's size."""
    sizes = [(320, 240), (200, 150)]
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
    boxes = [(170.0, 30.0, 60.0, 100.0), (20.0, 90.0, 50.0, 100.0)]  # past x = 200; past y = 150
    dets = []
    for w, h in sizes:
        cam = []
        for b in boxes:
            x1, y1 = min(b[0] + b[2], w - 1.0), min(b[1] + b[3], h - 1.0)
            f = np.stack([rng.uniform(b[0] + 1, x1 - 1, 30), rng.uniform(b[1] + 1, y1 - 1, 30)], 1)
            cam.append(t2d.make_detection(b, f.astype(np.float32)))
        dets.append(cam)
    with t2d.Group.with_sizes(sizes, [3, 4]) as g:
        for c in range(2):
            g.push_frame(c, frames[c])
        out = g.run(0, dets)
        app = g.appearance(0)
    rects = []
    for c, (w, h) in enumerate(sizes):
        res = out[c][1]
        assert len(res["objects"]) == len(boxes) == len(app[c])
        for o, rec in zip(res["objects"], app[c]):
            rect = rgbhist_ref.appearance_rect(o["box"], w, h)
            assert (rec["id"], rec["rect"], rec["n_pixels"]) == (o["id"], rect, rect[2] * rect[3])
            assert rec["n_pixels"] > 0
            np.testing.assert_array_equal(rec["counts"], rgbhist_ref.hist_counts(frames[c], rect))
            rects.append(rect)
    assert rects[0][2] > rects[2][2] and rects[1][3] > rects[3][3]  # the narrow camera's crops are the smaller ones


def test_equal_sizes_are_the_plain_group():
    """Group.with_sizes with all cameras equal and Group(W, H, ...): byte-identical
    packed result slots, and the same timed pushes and LK calls with the same kernels."""
    W, H, C, T = 320, 240, 2, 4
    scenes = [synth.make_scene(60 + c, W, H, 128, nboxes=3, box_w=32, box_h=80) for c in range(C)]
    frames = [[synth.to_bgr(sc.frame(t)) if c else sc.frame(t) for t in range(T)] for c, sc in enumerate(scenes)]
    dets = [[[t2d.make_detection((float(int(x)), float(int(y)), 32.0, 80.0), sc.points_at(t)[sc.pt_box == k])
              for k, (x, y) in enumerate(sc.box_at(t))] for sc in scenes] for t in range(T)]
    L = _lib.load()

    def run(make):
        slots = []
        with make() as g:
            assert L.psn_lk_num_classes(g.lk_handle()) == 1
            assert L.psn_lk_enable_timing(g.lk_handle(), 256, 1) == 0
            for t in range(T):
                for c in range(C):
                    g.push_frame(c, frames[c][t])
                for _, r in g.run(t, dets[t]):
                    slot = np.zeros(t2d.result_slot_bytes(16, 1), np.uint8)
                    t2d.pack_result(r, slot)
                    slots.append(slot.tobytes())
                    assert len(r["objects"]) >= 1
            tags = [tag for _, tag in _lib.timing_launches(L, g.lk_handle(), 256)]
            entries = _lib.timing_entries(L, g.lk_handle(), 256)
            n_push, n_track = ctypes.c_int(), ctypes.c_int()
            pm, tm = ctypes.c_double(), ctypes.c_double()
            assert L.psn_lk_timing_stats(g.lk_handle(), ctypes.byref(n_push), ctypes.byref(pm), ctypes.byref(n_track),
                                         ctypes.byref(tm)) == 0
        return slots, tags, entries, n_push.value, n_track.value

    plain = run(lambda: t2d.Group(W, H, [7, 9], max_objects=16))
    sized = run(lambda: t2d.Group.with_sizes([(W, H)] * C, [7, 9], max_objects=16))
    assert plain[0] == sized[0]
    assert plain[1:] == sized[1:] and plain[3] == C * T and plain[4] > 0


def test_wrong_size_push_and_too_many_sizes():
    sizes = [(320, 240), (200, 150)]
    wide, narrow = synth.texture(320, 240, 1), synth.texture(200, 150, 2)
    d = [[t2d.make_detection((10, 10, 30, 60), np.float32([[20, 20], [25, 30], [30, 40], [22, 50]]))]] * 2
    with t2d.Group.with_sizes(sizes, [0, 1]) as g:
        assert g.camera_size(0) == (320, 240, 320, 240) and g.camera_size(1) == (200, 150, 200, 150)
        with pytest.raises(t2d.T2dError) as e:
            g.camera_size(2)
        assert e.value.code == ERR_ARG
        with pytest.raises(t2d.T2dError) as e:
            g.push_frame(1, wide)
        assert e.value.code == ERR_ARG
        with pytest.raises(t2d.T2dError) as e:
            g.push_frame(0, narrow)
        assert e.value.code == ERR_ARG
        # at the C ABI: a row of the narrow camera's length into the wide camera
        assert g._L.psn_t2d_group_push_frame(g._h, 0, narrow.ctypes.data, 200, 1) == ERR_ARG
        # nothing was staged by the refused pushes: the group runs
        g.push_frame(0, wide)
        g.push_frame(1, narrow)
        out = g.run(0, d)
        assert [len(r["objects"]) for _, r in out] == [1, 1]
    with pytest.raises(t2d.T2dError) as e:
        t2d.Group.with_sizes([(320 + 8 * i, 240) for i in range(9)], list(range(9)))
    assert e.value.code == ERR_ARG
    with t2d.Group.with_sizes([(160 + 8 * i, 120) for i in range(8)], list(range(8))) as g:  # eight sizes fit
        assert _lib.load().psn_lk_num_classes(g.lk_handle()) == 8
        assert g.camera_size(7) == (216, 120, 216, 120)
