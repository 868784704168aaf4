"""An LK context with frame classes (psn_lk_create_classes, include/psn_lk.h) on the
device: classes 320x240 (slots 0-3) and 200x150 (slots 4-7), scratch slots 8-9.

The level pitches differ (512 and 256 bytes) and so does the level truncation of a
32x80 window (max level 1 and 0): a launch that took the other class's geometry
would read the wrong rows. Every check is bit for bit: pyramid levels against
tests/pyr_ref.py, LK against one-class contexts and the CPU oracle, GridFAST
against per-set calls and the oracle, histograms against tests/rgbhist_ref.py, the
scaled ingest against tests/resize_ref.py, JPEG pushes against single pushes.
Which launches a call is planned into (one per kernel and frame class) is checked
on the CPU, tests/test_lk_plan_classes.py; psn_lk_timing_launches shows here that a
call on two classes is a split call.
"""
import os

import numpy as np
import pytest

import pyr_ref
import resize_ref
import rgbhist_ref
from mcmtt_opticalflow_amd import _lib, hip, lk, synth

pytestmark = pytest.mark.gpu

ERR_ARG = -1
CLASSES = [(320, 240, 4), (200, 150, 4)]
WINS = [(21, 21), (32, 32), (32, 80)]   # single-tile, single-tile at its 1,024-px edge, box kernel
BIG = (70, 201)                         # the large class only: taller than the small frame
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_fixtures.npz")


@pytest.fixture(scope="module")
def scenes():
    """Per class: two consecutive frames of a moving scene and its points at the first."""
    out = []
    for k, (w, h, _) in enumerate(CLASSES):
        sc = synth.make_scene(70 + k, w, h, 90, nboxes=3, box_w=32, box_h=80, max_speed=3.0)
        out.append((sc.frame(0), sc.frame(1), sc.points_at(0)))
    return out


def _queries(scenes, first_slots):
    """One query per (class, window) on (first_slot, first_slot + 1), the classes
    interleaved, and the 70x201 window on class 0; every query tracks its class's points.
    -> (queries, points, [(class, window, first point, count)])."""
    qs, pts, index, n0 = [], [], [], 0
    for win in WINS + [BIG]:
        for k, (_, _, p) in enumerate(scenes):
            if win == BIG and k == 1:
                continue
            qs.append(lk.make_query(first_slots[k], first_slots[k] + 1, n0, len(p), lk.make_params(win, 3)))
            index.append((k, win, n0, len(p)))
            pts.append(p)
            n0 += len(p)
    return qs, np.concatenate(pts), index


def _push_pairs(ctx, scenes, first_slots):
    for k, (f0, f1, _) in enumerate(scenes):
        ctx.push_frame(first_slots[k], f0)
        ctx.push_frame(first_slots[k] + 1, f1)


@pytest.fixture(scope="module")
def reference(oracle_mod, scenes):
    """The oracle's outputs per (class, window): computed once, read by several tests."""
    ref = {}
    for k, (f0, f1, p) in enumerate(scenes):
        for win in WINS + ([BIG] if k == 0 else []):
            ref[(k, win)] = oracle_mod.calc_optical_flow_pyr_lk(f0, f1, p, win, 3)
    return ref


def _check_against(ref, index, nxt, st, er, what):
    for k, win, a, n in index:
        r_next, r_st, r_err = ref[(k, win)]
        np.testing.assert_array_equal(nxt[a:a + n], r_next, err_msg=f"{what}: class {k} window {win}")
        np.testing.assert_array_equal(st[a:a + n], r_st, err_msg=f"{what}: class {k} window {win}")
        if er is not None:
            np.testing.assert_array_equal(er[a:a + n], r_err, err_msg=f"{what}: class {k} window {win}")


def test_geometry_pitch_and_truncation():
    with lk.LKContext.with_classes(CLASSES) as ctx:
        assert ctx.classes == CLASSES and ctx.ring_slots == 8
        assert [ctx.class_slots(k) for k in range(2)] == [(0, 4), (4, 4)]
        assert [ctx.slot_class(s) for s in range(10)] == [0] * 4 + [1] * 4 + [0, 0]  # the scratch slots: class 0
        assert ctx.level_size(0) == (320, 240) == ctx.source_size() and ctx.get_scale() == 1.0
        for k, (w, h, _) in enumerate(CLASSES):
            assert ctx.class_source_size(k) == (w, h)
            for lv in range(4):
                assert ctx.class_level_size(k, lv) == (w, h)
                w, h = (w + 1) // 2, (h + 1) // 2
        # rows padded to 256 B: the two classes' level-0 pitches differ
        assert [(ctx.class_level_size(k, 0)[0] + 255) & ~255 for k in range(2)] == [512, 256]
        # the 32x80 window truncates to max level 1 in the first class and 0 in the second
        assert [lk.effective_max_level(*ctx.class_level_size(k, 0), 32, 80, 3) for k in range(2)] == [1, 0]
        L, i = _lib.load(), lk.ctypes.c_int()
        for bad in (-1, 2):
            assert L.psn_lk_class_slots(ctx.handle, bad, None, None) == ERR_ARG
            assert L.psn_lk_class_level_size(ctx.handle, bad, 0, None, None) == ERR_ARG
        assert L.psn_lk_class_level_size(ctx.handle, 1, 4, None, None) == ERR_ARG
        assert L.psn_lk_slot_class(ctx.handle, 10, lk.ctypes.byref(i)) == ERR_ARG


def test_levels_of_every_slot():
    """Different textures into all eight slots (gray and BGR), every level of every
    slot read back; a push of the other class's size is refused."""
    with lk.LKContext.with_classes(CLASSES) as ctx:
        frames = []
        for s in range(8):
            w, h = ctx.class_source_size(ctx.slot_class(s))
            g = synth.texture(w, h, 20 + s)
            frames.append(synth.to_bgr(g) if s % 2 else g)
        for s in (5, 0, 7, 2, 4, 1, 6, 3):  # not in slot order
            ctx.push_frame(s, frames[s])
        for s in range(8):
            for lv, ref in enumerate(pyr_ref.pyramid(frames[s], 3)):
                np.testing.assert_array_equal(ctx.read_level(s, lv), ref, err_msg=f"slot {s} level {lv}")
        with pytest.raises(lk.PsnLkError) as e:
            ctx.push_frame(4, frames[0])  # a 320x240 frame into the 200x150 class
        assert e.value.code == ERR_ARG
        with pytest.raises(lk.PsnLkError) as e:
            ctx.push_frame(0, frames[4])
        assert e.value.code == ERR_ARG
        # at the C ABI a row shorter than the class's is refused (the size itself is not an argument)
        small = np.ascontiguousarray(frames[4])
        assert ctx._L.psn_lk_push_frame(ctx.handle, 0, small.ctypes.data, 200, 1) == ERR_ARG
        np.testing.assert_array_equal(ctx.read_level(0, 0), pyr_ref.pyramid(frames[0], 0)[0])
    # the larger class second: its slots do not fit between class 0's user and scratch
    # slots and lie behind them
    with lk.LKContext.with_classes(CLASSES[::-1]) as ctx:
        assert [ctx.class_slots(k) for k in range(2)] == [(0, 4), (4, 4)] and ctx.level_size(0) == (200, 150)
        for s in range(8):
            ctx.push_frame(s, frames[(s + 4) % 8])
        for s in range(8):
            for lv, ref in enumerate(pyr_ref.pyramid(frames[(s + 4) % 8], 3)):
                np.testing.assert_array_equal(ctx.read_level(s, lv), ref, err_msg=f"reversed: slot {s} level {lv}")
        g = synth.texture(200, 150, 31)
        nxt, st, _ = ctx.calc_optical_flow_pyr_lk(g, g, np.float32([[50, 50], [150, 100]]), (21, 21), 3)  # the scratch slots
        np.testing.assert_array_equal(nxt, np.float32([[50, 50], [150, 100]]))
        assert st.tolist() == [1, 1]
        for s in range(8):  # ... which lie between the two classes' slots: nothing of either was overwritten
            np.testing.assert_array_equal(ctx.read_level(s, 3), pyr_ref.pyramid(frames[(s + 4) % 8], 3)[3])


def test_mixed_call(scenes, reference):
    """One psn_lk_track call with queries on both classes: the bits of two one-class
    contexts and of the oracle."""
    with lk.LKContext.with_classes(CLASSES, variants={"poison_lds": 1}) as ctx:
        _push_pairs(ctx, scenes, (0, 4))
        ctx.enable_timing(8, 1)
        qs, pts, index = _queries(scenes, (0, 4))
        nxt, st, er = ctx.track(qs, pts)
        _check_against(reference, index, nxt, st, er, "mixed call")
        assert int(st.sum()) > len(pts) // 2
        # the same queries class by class: single-class calls of the same context
        for k in range(2):
            sub = [q for q, ix in zip(qs, index) if ix[0] == k]
            n2, s2, e2 = ctx.track(sub, pts)
            for (kk, win, a, n) in index:
                if kk == k:
                    np.testing.assert_array_equal(n2[a:a + n], nxt[a:a + n])
                    np.testing.assert_array_equal(s2[a:a + n], st[a:a + n])
                    np.testing.assert_array_equal(e2[a:a + n], er[a:a + n])
        tags = [t for _, t in _lib.timing_launches(ctx._L, ctx.handle, 8)]
        assert len(tags) == 3 and all(t >= 1000 for t in tags)  # every call here is split over several launches
        # the one-shot call runs on the scratch slots: class 0's geometry
        f0, f1, p = scenes[0]
        n3, s3, e3 = ctx.calc_optical_flow_pyr_lk(f0, f1, p, (32, 80), 3)
        r = reference[(0, (32, 80))]
        np.testing.assert_array_equal(n3, r[0])
        np.testing.assert_array_equal(s3, r[1])
        np.testing.assert_array_equal(e3, r[2])
    # two one-class contexts
    for k, (w, h, n) in enumerate(CLASSES):
        with lk.LKContext(w, h, ring_slots=n, max_level_cap=3) as one:
            one.push_frame(0, scenes[k][0])
            one.push_frame(1, scenes[k][1])
            sub = [(q, ix) for q, ix in zip(qs, index) if ix[0] == k]
            for q, _ in sub:
                q.prev_slot, q.next_slot = 0, 1
            n1, s1, e1 = one.track([q for q, _ in sub], pts)
            for _, (kk, win, a, m) in sub:
                np.testing.assert_array_equal(n1[a:a + m], nxt[a:a + m], err_msg=f"class {k} {win}")
                np.testing.assert_array_equal(s1[a:a + m], st[a:a + m], err_msg=f"class {k} {win}")
                np.testing.assert_array_equal(e1[a:a + m], er[a:a + m], err_msg=f"class {k} {win}")


def test_cross_class_query_is_refused(scenes, reference):
    with lk.LKContext.with_classes(CLASSES) as ctx:
        _push_pairs(ctx, scenes, (0, 4))
        qs, pts, index = _queries(scenes, (0, 4))
        ctx.enable_timing(8, 1)
        bad = lk.make_query(1, 4, 0, 10, lk.make_params((21, 21), 3))
        with pytest.raises(lk.PsnLkError) as e:
            ctx.track(qs[:2] + [bad] + qs[2:], pts)
        assert e.value.code == ERR_ARG and "slots 1 and 4" in str(e.value), str(e.value)
        assert _lib.timing_launches(ctx._L, ctx.handle, 8) == []  # the call failed before anything was launched
        nxt, st, er = ctx.track(qs, pts)  # and the next call succeeds
        _check_against(reference, index, nxt, st, er, "after a refused call")


def test_overlap_modes_with_a_deferred_push_across_classes(scenes, reference):
    """A class-1 device push, deferred in FUSED mode, across a class-0 track (its
    build rides in that launch's tail with its own level table): the same bits in
    OFF, STREAM and FUSED."""
    bufs = [[hip.DeviceBuffer.from_array(f) for f in (f0, f1)] for f0, f1, _ in scenes]
    try:
        for mode in (_lib.OVERLAP_OFF, _lib.OVERLAP_STREAM, _lib.OVERLAP_FUSED):
            with lk.LKContext.with_classes(CLASSES, variants={"poison_lds": 1, "fused_helpers": 4}) as ctx:
                ctx.set_ingest_overlap(mode)
                ctx.enable_timing(16, 1)
                qs, pts, index = _queries(scenes, (0, 4))
                d_prev = hip.DeviceBuffer.from_array(pts)
                d_next, d_st, d_err = (hip.DeviceBuffer(len(pts) * 8), hip.DeviceBuffer(len(pts)),
                                       hip.DeviceBuffer(len(pts) * 4))
                try:
                    ctx.push_frame_device(0, bufs[0][0].addr, CLASSES[0][0], 1)
                    ctx.push_frame_device(1, bufs[0][1].addr, CLASSES[0][0], 1)
                    ctx.push_frame_device(4, bufs[1][0].addr, CLASSES[1][0], 1)
                    ctx.push_frame_device(5, bufs[1][1].addr, CLASSES[1][0], 1)  # FUSED: deferred
                    c0 = [q for q, ix in zip(qs, index) if ix[0] == 0]
                    c1 = [q for q, ix in zip(qs, index) if ix[0] == 1]
                    ctx.track_device(c0, d_prev.addr, d_next.addr, d_st.addr, d_err.addr)  # does not read slot 5
                    ctx.track_device(c1, d_prev.addr, d_next.addr, d_st.addr, d_err.addr)
                    ctx.sync()
                    hip.synchronize()
                    # FUSED: each push ran its predecessor's build as a launch of its own, and the
                    # last one (slot 5, class 1) rode in the class-0 call's single-tile launch
                    assert ctx.timing_stats()["n_push"] == (3 if mode == _lib.OVERLAP_FUSED else 4)
                    nxt = d_next.to_array((len(pts), 2), np.float32)
                    st = d_st.to_array(len(pts), np.uint8)
                    er = d_err.to_array(len(pts), np.float32)
                    _check_against(reference, index, nxt, st, er, f"overlap mode {mode}")
                    for lv, ref in enumerate(pyr_ref.pyramid(scenes[1][1], 3)):
                        np.testing.assert_array_equal(ctx.read_level(5, lv), ref, err_msg=f"mode {mode} level {lv}")
                finally:
                    for b in (d_prev, d_next, d_st, d_err):
                        b.free()
    finally:
        for pair in bufs:
            for b in pair:
                b.free()


def test_gridfast_sets_over_both_classes(oracle_mod, scenes):
    """Sets on slots of both classes, the classes alternating (every set starts a new
    launch): keypoints, order and counts of per-set calls and of the oracle; a roi
    past the small frame's edges is clamped to the small frame."""
    rois = {0: [(10, 10, 120, 150), (200, 60, 200, 300), (0, 0, 320, 240)],
            1: [(10, 10, 120, 130), (150, 100, 100, 100), (0, 0, 320, 240)]}

    def clip(r, w, h):
        x0, y0 = max(r[0], 0), max(r[1], 0)
        return (x0, y0, max(min(r[0] + r[2], w) - x0, 0), max(min(r[1] + r[3], h) - y0, 0))

    with lk.LKContext.with_classes(CLASSES) as ctx:
        _push_pairs(ctx, scenes, (0, 4))
        slots = [0, 4, 1, 5, 4]
        sets = [rois[ctx.slot_class(s)] for s in slots]
        got = ctx.gridfast_detect_sets(slots, sets, seed=11)
        n_kp = 0
        for s, rs, (g_pts, g_tot) in zip(slots, sets, got):
            k = ctx.slot_class(s)
            w, h, _ = CLASSES[k]
            o_pts, o_tot = ctx.gridfast_detect(s, rs, seed=11)
            img = scenes[k][s - (0, 4)[k]]
            r_pts, r_tot = oracle_mod.gridfast_detect(img, [clip(r, w, h) for r in rs], seed=11)
            np.testing.assert_array_equal(g_tot, o_tot, err_msg=f"slot {s}")
            np.testing.assert_array_equal(g_tot, r_tot, err_msg=f"slot {s} against the oracle")
            for a, b, c in zip(g_pts, o_pts, r_pts):
                np.testing.assert_array_equal(a, b, err_msg=f"slot {s}")
                np.testing.assert_array_equal(a, c, err_msg=f"slot {s} against the oracle")
                n_kp += len(a)
                assert len(a) == 0 or (a[:, 0].max() < w and a[:, 1].max() < h)
        assert n_kp > 200


def test_histograms_clip_per_class():
    """A rect that overhangs x = 200: clipped at 200 on the small class, whole on the large one."""
    rng = np.random.default_rng(3)
    big = rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)
    small = rng.integers(0, 256, (150, 200, 3), dtype=np.uint8)
    rects = np.array([(170, 20, 60, 100), (10, 100, 80, 80), (-5, -5, 50, 50)], np.int32)
    with lk.LKContext.with_classes(CLASSES) as ctx:
        ctx.push_frame_async(1, big)
        ctx.push_frame_async(6, small)
        ctx.sync()
        g_big, g_small = ctx.box_histograms([(1, rects), (6, rects)])
        for frame, got in ((big, g_big), (small, g_small)):
            h, w = frame.shape[:2]
            for g, r in zip(got, rects):
                np.testing.assert_array_equal(g, rgbhist_ref.hist_counts(frame, rgbhist_ref.clip_rect(r, w, h)))
        assert int(g_big[0].sum()) == 3 * 60 * 100 and int(g_small[0].sum()) == 3 * 30 * 100
        assert int(g_small[1].sum()) == 3 * 80 * 50  # and the bottom edge at y = 150


def test_scaled_classes(oracle_mod):
    """Classes 384x288 and 361x287 at 0.5: LK sizes 192x144 and 180x143 (each class its
    own truncation of the product), level 0 = resize_ref of the class's own source, and
    the histograms still on the full-size colour frames."""
    cls = [(384, 288, 2), (361, 287, 2)]
    with lk.LKContext.with_classes(cls, scale=0.5) as ctx:
        assert [ctx.class_level_size(k, 0) for k in range(2)] == [(192, 144), (180, 143)]
        assert [ctx.class_level_size(k, 0) for k in range(2)] == [lk.scaled_size(w, h, 0.5) for w, h, _ in cls]
        assert [ctx.class_source_size(k) for k in range(2)] == [(384, 288), (361, 287)]
        assert ctx.level_size(0) == (192, 144) and ctx.source_size() == (384, 288) and ctx.get_scale() == 0.5
        frames = {}
        for s in range(4):
            w, h = ctx.class_source_size(ctx.slot_class(s))
            g = synth.texture(w, h, 50 + s)
            frames[s] = synth.to_bgr(g) if s in (1, 2) else g
        for s in (3, 0, 2, 1):
            ctx.push_frame(s, frames[s])
        for s in range(4):
            gray = oracle_mod.bgr2gray(frames[s]) if frames[s].ndim == 3 else frames[s]
            want = oracle_mod.build_pyramid(resize_ref.resize(gray, 0.5), 4)
            for lv, ref in enumerate(want):
                np.testing.assert_array_equal(ctx.read_level(s, lv), ref, err_msg=f"slot {s} level {lv}")


def test_jpeg_batch_over_both_classes():
    """One psn_lk_push_frames_jpeg with a file per class (320x240 and 131x97): the bytes
    of the single pushes, one batch of two items; a file of the other class's size is
    refused with its item index before any slot is touched."""
    z = np.load(GOLDEN)
    big, small = z["420_q85_rstrow_jpeg"].tobytes(), z["422_q60_rst5_jpeg"].tobytes()
    cls = [(320, 240, 2), (131, 97, 2)]
    rects = np.array([(100, 50, 120, 100), (0, 0, 400, 400)], np.int32)

    def read(ctx, a, b):
        lv = [ctx.read_level(s, l) for s in (a, b) for l in range(3)]
        return lv, ctx.box_histograms([(a, rects), (b, rects)])

    with lk.LKContext.with_classes(cls, max_level_cap=2) as ctx:
        ctx.push_frame_jpeg(1, big)
        ctx.push_frame_jpeg(2, small)
        ctx.sync()
        ref_lv, ref_hist = read(ctx, 1, 2)
        np.testing.assert_array_equal(ref_lv[0], pyr_ref.gray(z["420_q85_rstrow_bgr"]))
        assert ref_lv[3].shape == (97, 131)
    with lk.LKContext.with_classes(cls, max_level_cap=2) as ctx:
        ctx.push_frames_jpeg([3, 0], [small, big])
        ctx.sync()
        got_lv, got_hist = read(ctx, 0, 3)
        for a, b in zip(got_lv, ref_lv):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(got_hist, ref_hist):
            np.testing.assert_array_equal(a, b)
        # one batch of two items
        assert ctx.jpeg_batch_stats(1) == ctx.jpeg_stats() and ctx.jpeg_batch_stats(0)["blocks"] > 0
        with pytest.raises(lk.PsnLkError):
            ctx.jpeg_batch_stats(2)
        with pytest.raises(lk.PsnLkError) as e:  # the small file into a slot of the large class
            ctx.push_frames_jpeg([1, 2], [big, big])
        assert e.value.code == ERR_ARG and "item 1" in str(e.value)
        with pytest.raises(lk.PsnLkError) as e:
            ctx.push_frames_jpeg([1, 2], [small, small])
        assert e.value.code == ERR_ARG and "item 0" in str(e.value)
        with pytest.raises(lk.PsnLkError) as e:
            ctx.push_frame_jpeg(2, big)
        assert e.value.code == ERR_ARG
        got_lv, _ = read(ctx, 0, 3)  # nothing was touched
        for a, b in zip(got_lv, ref_lv):
            np.testing.assert_array_equal(a, b)
