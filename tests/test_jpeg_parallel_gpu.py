"""The parallel entropy path on the device (jpeg_sync_kernel, jpeg_chain_kernel,
jpeg_emit_kernel, jpeg_dc_kernel): byte for byte the serial path's output, which
for intact files is PIL's and the oracle's."""
import numpy as np
import pytest

import jpeg_variants as jv
from mcmtt_opticalflow_amd import _lib, lk, synth
from test_jpeg import _color_frame, _pil_jpeg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frame_640():
    """One 640x480 synth frame, q90 4:2:0, no restart options: (file, PIL's decode)."""
    pytest.importorskip("PIL")
    return _pil_jpeg(_color_frame(synth.make_scene(7, 640, 480, 32), 0), quality=90, subsampling=2)


@pytest.mark.parametrize("s", [4, 16, 128])
def test_restartless_fixtures(oracle_mod, s):
    with lk.JpegDecoder(entropy=2, sub_bytes=s) as dec:
        for name in sorted(jv.PLAIN):
            data, bgr = jv.fixture(name)
            got = dec.decode(data)
            np.testing.assert_array_equal(got, bgr, err_msg=name)
            np.testing.assert_array_equal(got, oracle_mod.jpeg_decode_bgr(data), err_msg=name)
            st = dec.stats()
            nsub = -(-jv.PLAIN[name] // s)
            assert st["path"] == _lib.JPEG_PATH_PARALLEL and st["sub_bytes"] == s, (name, st)
            assert st["subsequences"] == nsub and st["sequences"] == -(-nsub // 256), (name, st)
            assert st["blocks"] == jv.scan_blocks(data), (name, st)
            assert 1 <= st["sync_rounds"] <= 256 and 1 <= st["chain_rounds"] <= st["sequences"], (name, st)
            if name == "444_q95" and s == 4:
                assert st["sequences"] == 8


@pytest.mark.parametrize("damage", [jv.truncated, jv.corrupted])
@pytest.mark.parametrize("s", [4, 128])
def test_damaged_variants_equal_serial_path(damage, s):
    bad = damage(jv.fixture("444_q95")[0])
    with lk.JpegDecoder(entropy=1) as ser, lk.JpegDecoder(entropy=2, sub_bytes=s) as par:
        ref = ser.decode(bad)
        assert ser.stats()["path"] == _lib.JPEG_PATH_SERIAL
        got = par.decode(bad)
        st = par.stats()
    assert st["path"] == _lib.JPEG_PATH_PARALLEL and st["blocks"] == jv.scan_blocks(bad), st
    np.testing.assert_array_equal(got, ref)


def test_frame_640_default_decoder(oracle_mod, frame_640):
    data, ref = frame_640
    plan = lk.JpegDecoder.plan(data)
    with lk.JpegDecoder() as dec:
        got = dec.decode(data)
        st = dec.stats()
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(got, oracle_mod.jpeg_decode_bgr(data))
    print("640x480 q90 4:2:0:", st)
    assert st["path"] == _lib.JPEG_PATH_PARALLEL and st["sequences"] > 1
    assert (st["sub_bytes"], st["subsequences"], st["sequences"]) == (plan["sub_bytes"], plan["subsequences"],
                                                                      plan["sequences"])
    assert st["blocks"] == 40 * 30 * 6
    # the caps, not typical values: a sequence is 256 subsequences, the chain has one thread a sequence
    assert 1 <= st["sync_rounds"] <= 256 and 1 <= st["chain_rounds"] <= st["sequences"]


def test_context_push_frame_jpeg(oracle_mod, frame_640):
    data, _ = frame_640
    ref = oracle_mod.build_pyramid(oracle_mod.bgr2gray(oracle_mod.jpeg_decode_bgr(data)), 4)
    with lk.LKContext(640, 480, ring_slots=2, max_level_cap=3) as ctx:
        with pytest.raises(lk.PsnLkError):
            ctx.jpeg_stats()  # no JPEG pushed yet
        ctx.push_frame_jpeg(1, data)
        ctx.sync()
        for lvl in range(4):
            np.testing.assert_array_equal(ctx.read_level(1, lvl), ref[lvl], err_msg=f"level {lvl}")
        st = ctx.jpeg_stats()
    assert st["path"] == _lib.JPEG_PATH_PARALLEL and st["sequences"] > 1 and st["blocks"] == 40 * 30 * 6, st


def test_restart_file_keeps_serial_path():
    pytest.importorskip("PIL")
    data, ref = _pil_jpeg(_color_frame(synth.make_scene(7, 640, 480, 32), 0), quality=90, subsampling=2,
                          restart_marker_rows=1)
    with lk.JpegDecoder() as dec:
        got = dec.decode(data)
        st = dec.stats()
    np.testing.assert_array_equal(got, ref)
    assert st["path"] == _lib.JPEG_PATH_SERIAL and st["segments"] == 30, st
    assert (st["subsequences"], st["sequences"], st["sync_rounds"], st["chain_rounds"]) == (0, 0, 0, 0)
