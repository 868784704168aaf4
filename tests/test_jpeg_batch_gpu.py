"""A frame-set's JPEG files decoded in one batched device pass
(psn_jpeg_decode_batch_device, psn_lk_push_frames_jpeg,
psn_t2d_group_push_frames_jpeg) against the single-image calls.

The reference of every item is never another batch: the single-image
psn_jpeg_decode on a fresh decoder (the same device code as a batch of one: an
item decodes the same alone and among neighbours), the CPU oracle (independent
of the library: every item of every batch), PIL's decodes of the golden
fixtures, and for synthesised streams the coefficient arrays they were written
from. The cases are the smallest that reach each way a batch entry can go wrong:
unequal extents (early-exit workgroups), per-item round counters, both entropy
paths in one batch, an item's bytes beside a neighbour's, and the all-or-nothing
refusal."""
import ctypes
import functools
import io

import numpy as np
import pytest

import jpeg_synth as js
import jpeg_variants as jv
from mcmtt_opticalflow_amd import _lib, lk, synth

pytestmark = pytest.mark.gpu

FIXTURES = sorted(jv.PLAIN) + list(jv.RESTART)


@functools.lru_cache(maxsize=None)
def _single(data, entropy=0, sub=0):
    """(pixels, stats) of the single-image decode on a fresh decoder (computed once per file and mode)."""
    with lk.JpegDecoder(entropy=entropy, sub_bytes=sub) as dec:
        out = dec.decode(data)
        out.setflags(write=False)
        return out, dec.stats()


@functools.lru_cache(maxsize=None)
def _oracle(oracle_mod, data):
    """The CPU oracle's pixels (it feeds zeros past a truncated stream, as the device readers do)."""
    out = oracle_mod.jpeg_decode_bgr(data)
    out.setflags(write=False)
    return out


def _check_batch(oracle_mod, dec, files, entropy=0, sub=0, stats=True):
    outs = dec.decode_batch(files)
    assert len(outs) == len(files)
    for i, (f, got) in enumerate(zip(files, outs)):
        ref, st = _single(f, entropy, sub)
        np.testing.assert_array_equal(got, ref, err_msg=f"item {i}")
        np.testing.assert_array_equal(got, _oracle(oracle_mod, f), err_msg=f"item {i} against the oracle")
        if stats:
            assert dec.batch_stats(i) == st, f"item {i}"
    return outs


def _cut40(data):
    """The file's entropy data cut at 40 % (not after an FF), closed with EOI."""
    e0, e1 = jv.entropy_range(data)
    cut = e0 + (e1 - e0) * 4 // 10
    while data[cut - 1] == 0xFF:
        cut -= 1
    return data[:cut] + jv.EOI


def test_mixed_geometry_and_path_in_one_batch(oracle_mod):
    """Every golden fixture together, planner at its default: three samplings, a
    one-component file, odd sizes, restart files (serial list) beside restart-less
    ones (parallel list)."""
    files = [jv.fixture(n)[0] for n in FIXTURES]
    with lk.JpegDecoder() as dec:
        outs = _check_batch(oracle_mod, dec, files)
        paths = {dec.batch_stats(i)["path"] for i in range(len(files))}
        assert dec.stats() == dec.batch_stats(len(files) - 1)  # the last item's
    assert paths == {_lib.JPEG_PATH_SERIAL, _lib.JPEG_PATH_PARALLEL}
    assert len({o.shape for o in outs}) > 2
    for n, f, got in zip(FIXTURES, files, outs):
        np.testing.assert_array_equal(got, jv.fixture(n)[1], err_msg=n)  # PIL's decode
        np.testing.assert_array_equal(got, oracle_mod.jpeg_decode_bgr(f), err_msg=n)


def test_unequal_extents_at_sub4(oracle_mod):
    """S = 4: one sequence (gray_q80: 137 subsequences, under 256) beside 444_q95
    (8 sequences) and ambiguous444 (both round caps): early-exit workgroups and
    per-item round counters."""
    amb = js.case("ambiguous444")
    files = [jv.fixture("gray_q80")[0], jv.fixture("444_q95")[0], amb.data]
    with lk.JpegDecoder(entropy=2, sub_bytes=4) as dec:
        outs = _check_batch(oracle_mod, dec, files, 2, 4)
        st = [dec.batch_stats(i) for i in range(3)]
        assert st[0]["sequences"] == 1 and st[0]["subsequences"] < 256 and st[1]["sequences"] == 8
        assert st[2]["sync_rounds"] == 256 and st[2]["chain_rounds"] == st[2]["sequences"] >= 4
        assert st[0]["sync_rounds"] < 256
        np.testing.assert_array_equal(dec.batch_coefficients(2), amb.coefs)
        for i in (0, 1):  # the files' coefficients: the CPU model's serial decode
            np.testing.assert_array_equal(dec.batch_coefficients(i), lk.JpegDecoder.model(files[i], 1, 0)[0])
        np.testing.assert_array_equal(dec.coefficients(), amb.coefs)  # the last item's
    for f, got in zip(files, outs):
        np.testing.assert_array_equal(got, oracle_mod.jpeg_decode_bgr(f))


def test_more_than_1024_sequences_in_one_item():
    """multipass at S = 4: two chain passes in one item, beside a small file."""
    mp = js.case("multipass")
    small = jv.fixture("420_tiny")[0]
    with lk.JpegDecoder(entropy=2, sub_bytes=4) as dec:
        outs = dec.decode_batch([small, mp.data])
        st = dec.batch_stats(1)
        assert st["sequences"] > 1024 and st["blocks"] == mp.coefs.shape[0]
        np.testing.assert_array_equal(dec.batch_coefficients(1), mp.coefs)
        np.testing.assert_array_equal(outs[0], _single(small, 2, 4)[0])
        assert dec.batch_stats(0) == _single(small, 2, 4)[1]


@pytest.mark.parametrize("sub", [4, 64])
def test_a_neighbours_bytes(oracle_mod, sub):
    """A file cut at 40 % before and after intact files, ladder_ff (a third of its
    bytes FF) first and last in the blob: the emit kernel's last thread decodes
    past a truncated item's end and must read zeros there, not the next item's
    bytes. The reversed batch gives the same per-item output."""
    lad = js.case("ladder_ff").data
    cut = _cut40(jv.fixture("422_q90")[0])
    files = [lad, cut, jv.fixture("420_q75")[0], cut, jv.fixture("444_q95")[0], _cut40(jv.fixture("gray_q80")[0]), lad]
    with lk.JpegDecoder(entropy=2, sub_bytes=sub) as dec:
        fwd = _check_batch(oracle_mod, dec, files, 2, sub)
        rev = _check_batch(oracle_mod, dec, files[::-1], 2, sub)
    for a, b in zip(fwd, rev[::-1]):
        np.testing.assert_array_equal(a, b)


def test_sizes(oracle_mod):
    name, f = "420_tiny", jv.fixture("420_tiny")[0]
    big = jv.fixture("444_q95")[0]
    with lk.JpegDecoder() as dec:
        _check_batch(oracle_mod, dec, [big])                       # n = 1
        outs = _check_batch(oracle_mod, dec, [big] * 8)            # the same file into 8 outputs
        assert all(np.array_equal(o, outs[0]) for o in outs)
        _check_batch(oracle_mod, dec, [f] * _lib.JPEG_MAX_BATCH)   # the largest batch
        with pytest.raises(lk.PsnLkError):
            dec.batch_stats(_lib.JPEG_MAX_BATCH)
        with pytest.raises(lk.PsnLkError) as e:
            dec.decode_batch([f] * (_lib.JPEG_MAX_BATCH + 1))
        assert e.value.code == -1


def test_all_or_nothing(oracle_mod):
    good = [jv.fixture(n)[0] for n in ("420_q75", "gray_q80", "420_q85_rstrow", "444_q95")]
    bad = list(good)
    bad[2] = bad[2][:2] + b"\x00\x00" + bad[2][4:]  # no marker after SOI
    with lk.JpegDecoder() as dec:
        _check_batch(oracle_mod, dec, good[:2])
        before = dec.stats()
        with pytest.raises(lk.PsnLkError) as e:
            dec.decode_batch(bad)
        assert e.value.code == -1 and "item 2" in str(e.value)
        assert dec.stats() == before and dec.batch_stats(1) == before  # the context is as it was
        _check_batch(oracle_mod, dec, good)
        ref, st = _single(good[0])
        np.testing.assert_array_equal(dec.decode(good[0]), ref)
        assert dec.stats() == st
        with pytest.raises(lk.PsnLkError):  # the last decode is no batch any more
            dec.batch_stats(0)


@pytest.mark.parametrize("entropy,sub", [(1, 0), (2, 4), (2, 64), (2, 256)])
def test_modes_and_sizes(oracle_mod, entropy, sub):
    """Debug modes 1 and 2, S in {4, 64, 256} (256: bytes unstaged)."""
    files = [jv.fixture("422_q90")[0], jv.fixture("420_q30_rst3")[0], jv.fixture("444_q95")[0]]
    with lk.JpegDecoder(entropy=entropy, sub_bytes=sub) as dec:
        _check_batch(oracle_mod, dec, files, entropy, sub)
        want = _lib.JPEG_PATH_SERIAL if entropy == 1 else _lib.JPEG_PATH_PARALLEL
        assert [dec.batch_stats(i)["path"] for i in range(3)] == [want, _lib.JPEG_PATH_SERIAL, want]


# ------------------------------------------------------------------ LKContext, Group

def _pil_jpeg(img, **opt):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", **opt)
    return b.getvalue()


def _color_frame(sc, t):
    rgb = synth.to_bgr(sc.frame(t))[..., ::-1].copy()
    rgb[..., 0] = np.clip(rgb[..., 0].astype(np.int32) + ((np.arange(sc.width) * 7) % 61 - 30)[None, :], 0, 255)
    return rgb.astype(np.uint8)


def test_lk_push_frames_jpeg():
    pytest.importorskip("PIL")
    W, H = 320, 240
    sc = synth.make_scene(9, W, H, 32)
    files = [_pil_jpeg(_color_frame(sc, 0), quality=88, subsampling=2),
             _pil_jpeg(_color_frame(sc, 1), quality=88, subsampling=2, restart_marker_rows=1)]
    rects = [(1, [(10, 20, 64, 80), (300, 200, 40, 60)]), (2, [(100, 50, 33, 41)])]

    def read(ctx):
        ctx.sync()
        return ([ctx.read_level(s, lvl) for s in (1, 2) for lvl in range(4)], np.concatenate(ctx.box_histograms(rects)))

    with lk.LKContext(W, H, ring_slots=3, max_level_cap=3) as ctx:
        ctx.push_frame_jpeg(1, files[0])
        ctx.push_frame_jpeg(2, files[1])
        ref_lv, ref_hist = read(ctx)
    with lk.LKContext(W, H, ring_slots=3, max_level_cap=3) as ctx:
        ctx.push_frames_jpeg([1, 2], files)
        got_lv, got_hist = read(ctx)
        for a, b in zip(got_lv, ref_lv):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(got_hist, ref_hist)
        # one batch of two frames: one upload and one launch per kernel, whatever the count
        assert ctx.jpeg_batch_stats(1) == ctx.jpeg_stats()
        assert ctx.jpeg_batch_stats(0)["path"] == _lib.JPEG_PATH_PARALLEL
        assert ctx.jpeg_batch_stats(1)["path"] == _lib.JPEG_PATH_SERIAL
        with pytest.raises(lk.PsnLkError):
            ctx.jpeg_batch_stats(2)
        with pytest.raises(lk.PsnLkError) as e:  # a repeated slot
            ctx.push_frames_jpeg([0, 1, 0], [files[0], files[1], files[0]])
        assert e.value.code == -5 and "item 2" in str(e.value)
        other = _pil_jpeg(np.zeros((64, 64, 3), np.uint8) + 77, quality=80)
        with pytest.raises(lk.PsnLkError) as e:  # a frame of another size
            ctx.push_frames_jpeg([0, 1], [files[0], other])
        assert e.value.code == -1 and "item 1" in str(e.value)
        got_lv, got_hist = read(ctx)  # nothing was touched
        for a, b in zip(got_lv, ref_lv):
            np.testing.assert_array_equal(a, b)
        ctx.push_frames_jpeg([2, 1], files)  # and the context still works
        ctx.sync()
        np.testing.assert_array_equal(ctx.read_level(2, 0), ref_lv[0])
        np.testing.assert_array_equal(ctx.read_level(1, 1), ref_lv[5])


@pytest.mark.parametrize("opt", [{}, {"restart_marker_rows": 1}], ids=["restartless", "restart_rows"])
def test_group_push_frames_jpeg(opt):
    """A 2-camera 320x240 group, a few frames: per-camera pushes against batch
    pushes, packed result slots byte-identical every frame."""
    from mcmtt_opticalflow_amd import tracker2d as t2d

    pytest.importorskip("PIL")
    W, H, C, T = 320, 240, 2, 4
    scenes = [synth.make_scene(80 + c, W, H, 64, nboxes=2, box_w=32, box_h=80) for c in range(C)]
    files = [[_pil_jpeg(_color_frame(sc, t), quality=90, subsampling=2, **opt) for t in range(T)] for sc in scenes]

    def run(batch):
        out = []
        with t2d.Group(W, H, list(range(C)), max_objects=8) as g:
            for t in range(T):
                if batch:
                    g.push_frames_jpeg([files[c][t] for c in range(C)])
                else:
                    for c in range(C):
                        g.push_frame_jpeg(c, files[c][t])
                dets = []
                for sc in scenes:
                    pts = sc.points_at(t)
                    dets.append([t2d.make_detection((float(int(x)), float(int(y)), 32.0, 80.0), pts[sc.pt_box == k])
                                 for k, (x, y) in enumerate(sc.box_at(t))])
                packed = []
                for _, r in g.run(t, dets):
                    slot = np.zeros(t2d.result_slot_bytes(8, 1), np.uint8)
                    t2d.pack_result(r, slot)
                    packed.append((slot.tobytes(), len(r["objects"])))
                out.append(packed)
            if batch:  # one batch of C frames per push: the decoder's last decode has items 0..C-1
                L, s = _lib.load(), _lib.JpegStats()
                assert L.psn_lk_jpeg_batch_stats(g.lk_handle(), C - 1, ctypes.byref(s)) == 0
                assert L.psn_lk_jpeg_batch_stats(g.lk_handle(), C, ctypes.byref(s)) == -1
        return out

    a, b = run(False), run(True)
    assert a == b
    assert sum(n for f in a for _, n in f) > 4
