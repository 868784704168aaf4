"""The single-image JPEG decode is a batch of one (psn_jpeg_decode_device over
the decode psn_jpeg_decode_batch_device runs): what the single-image calls showed
before the two paths were merged, pinned.

Single images and batches alternate on one decoder, with buffers that grow and
buffers that do not; a single image's coefficients and round counters at the
smallest shapes where the parallel kernels can go wrong; the single-image calls'
error texts, which name no item; a refusal leaves the records of the last decode
alone."""
import functools
import io

import numpy as np
import pytest

import jpeg_synth as js
import jpeg_variants as jv
from mcmtt_opticalflow_amd import _lib, hip, lk

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("path", "sub_bytes", "subsequences", "sequences", "sync_rounds", "chain_rounds", "blocks")


@functools.lru_cache(maxsize=None)
def _fresh_stats(name):
    """stats() of a fixture decoded alone on a fresh decoder."""
    with lk.JpegDecoder() as dec:
        dec.decode(jv.fixture(name)[0])
        return dec.stats()


def test_single_batch_single_on_one_decoder():
    """420_tiny alone, a batch, a restart file alone (serial route), 444_q95 alone
    (parallel route, its scratch after a serial item's 16 bytes), 420_tiny again."""
    def single(dec, name):
        data, pil = jv.fixture(name)
        np.testing.assert_array_equal(dec.decode(data), pil, err_msg=name)
        assert dec.stats() == _fresh_stats(name), name
        with pytest.raises(lk.PsnLkError) as e:
            dec.batch_stats(0)
        assert e.value.code == -1 and "the last decode was not a batch" in str(e.value)
        with pytest.raises(lk.PsnLkError) as e:
            dec.batch_coefficients(0)
        assert e.value.code == -1 and "the last decode was not a batch" in str(e.value)

    batch = ["444_q95", "420_q85_rstrow", "gray_q80"]
    with lk.JpegDecoder() as dec:
        single(dec, "420_tiny")
        outs = dec.decode_batch([jv.fixture(n)[0] for n in batch])
        for i, (n, got) in enumerate(zip(batch, outs)):
            np.testing.assert_array_equal(got, jv.fixture(n)[1], err_msg=n)
            assert dec.batch_stats(i) == _fresh_stats(n), n
        assert dec.stats() == dec.batch_stats(2)
        single(dec, "420_q85_rstrow")
        assert dec.stats()["path"] == _lib.JPEG_PATH_SERIAL
        single(dec, "444_q95")
        assert dec.stats()["path"] == _lib.JPEG_PATH_PARALLEL
        single(dec, "420_tiny")


@pytest.mark.parametrize("name", ["gray_q80", "ambiguous444", "multipass"])
def test_single_image_coefficients_and_counters_at_sub4(name):
    """Debug entropy mode 2, S = 4, each file alone: gray_q80 is one sequence of
    fewer than 256 subsequences, ambiguous444 reaches both round caps, multipass
    has more than 1,024 sequences (two chain passes)."""
    if name == "gray_q80":
        data = jv.fixture(name)[0]
        coefs = lk.JpegDecoder.model(data, 1, 0)[0]  # the CPU model's serial decode
    else:
        data, coefs = js.case(name).data, js.case(name).coefs
    with lk.JpegDecoder(entropy=2, sub_bytes=4) as dec:
        dec.decode(data)
        st = dec.stats()
        np.testing.assert_array_equal(dec.coefficients(), coefs)
    want = lk.JpegDecoder.model(data, 2, 4)[1]
    assert {k: st[k] for k in STAT_FIELDS} == {k: want[k] for k in STAT_FIELDS}
    assert st["path"] == _lib.JPEG_PATH_PARALLEL and st["sub_bytes"] == 4 and st["blocks"] == coefs.shape[0]
    if name == "gray_q80":  # what batch_stats reported for these files as items of a batch
        assert st["sequences"] == 1 and st["subsequences"] < 256 and st["sync_rounds"] < 256
    elif name == "ambiguous444":
        assert st["sync_rounds"] == 256 and st["chain_rounds"] == st["sequences"] >= 4
    else:
        assert st["sequences"] > 1024


def test_single_image_error_texts():
    """The texts psn_jpeg_decode_device gave before it became a batch of one, and the
    batch call's, which names the item. A refusal leaves stats() as it was."""
    good = jv.fixture("420_q75")[0]
    w, h, _ = lk.JpegDecoder.info(good)
    no_marker = good[:2] + b"\x00\x00" + good[4:]  # no marker after SOI
    buf = hip.DeviceBuffer(2 * 3 * w * h)
    with lk.JpegDecoder() as dec:
        try:
            L, ctx = dec._L, dec._h
            dec.decode(good)
            before = dec.stats()

            def single(data, stride):
                rc = L.psn_jpeg_decode_device(ctx, data, len(data), buf.ptr, stride)
                return rc, L.psn_jpeg_last_error(ctx).decode()

            assert single(no_marker, 3 * w) == (-1, "marker expected")
            assert dec.stats() == before
            assert single(good, 3 * w - 1) == (-1, f"stride {3 * w - 1} < 3 * width {w}")
            assert dec.stats() == before

            def batch_of_two(data, stride):
                items, keep = dec._items([good, data], [buf.addr, buf.addr + 3 * w * h], [3 * w, stride])
                rc = L.psn_jpeg_decode_batch_device(ctx, items, 2)
                return rc, L.psn_jpeg_last_error(ctx).decode()

            assert batch_of_two(no_marker, 3 * w) == (-1, "item 1: marker expected")
            assert dec.stats() == before
            assert batch_of_two(good, 3 * w - 1) == (-1, f"item 1: stride {3 * w - 1} < 3 * width {w}")
            assert dec.stats() == before
            with pytest.raises(lk.PsnLkError):  # the last decode is still the single image
                dec.batch_stats(0)
            np.testing.assert_array_equal(dec.decode(good), jv.fixture("420_q75")[1])
        finally:
            dec.close()  # waits for the decoder's stream before the buffer goes
            buf.free()


def test_push_frame_jpeg_errors_stay_unprefixed():
    """A 64x64 file on a 320x240 context: code -1, both sizes, no item; nothing is touched."""
    Image = pytest.importorskip("PIL.Image")
    data = jv.fixture("420_q85_rstrow")[0]  # 320x240
    b = io.BytesIO()
    Image.fromarray(np.zeros((64, 64, 3), np.uint8) + 77).save(b, "JPEG", quality=80)
    with lk.LKContext(320, 240, ring_slots=2, max_level_cap=2) as ctx:
        ctx.push_frame_jpeg(0, data)
        ctx.sync()
        before = [ctx.read_level(0, lvl) for lvl in range(3)]
        with pytest.raises(lk.PsnLkError) as e:
            ctx.push_frame_jpeg(0, b.getvalue())
        assert e.value.code == -1
        assert "JPEG 64x64, context 320x240" in str(e.value) and "item" not in str(e.value)
        with pytest.raises(lk.PsnLkError):  # a single-frame push is no batch
            ctx.jpeg_batch_stats(0)
        ctx.sync()
        for a, lv in zip(before, (ctx.read_level(0, lvl) for lvl in range(3))):
            np.testing.assert_array_equal(lv, a)
