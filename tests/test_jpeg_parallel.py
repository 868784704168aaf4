"""The parallel entropy path of the device JPEG decoder, on the CPU: the planner
(psn_jpeg_entropy_plan) and the CPU model (psn_jpeg_entropy_model), which runs
the kernels' symbol step (csrc/psn_jpeg_entropy.h) with their rounds emulated
one after the other. The output is defined by the serial decode: the parallel
coefficients equal it exactly for intact, truncated and corrupted plain streams
at every subsequence size, down to 4 bytes (symbols longer than a subsequence,
several sequences for jpeg_chain_kernel)."""
import numpy as np
import pytest

import jpeg_variants as jv
from mcmtt_opticalflow_amd import _lib, lk

SUBS = [4, 8, 16, 64, 128, 1024]


@pytest.mark.parametrize("name", sorted(jv.PLAIN))
def test_plan_parallel_for_restartless(name):
    data, _ = jv.fixture(name)
    p = lk.JpegDecoder.plan(data)
    e0, e1 = jv.entropy_range(data)
    assert p["entropy_bytes"] == e1 - e0 == jv.PLAIN[name]
    assert p["path"] == _lib.JPEG_PATH_PARALLEL and p["plain"] == 1 and p["segments"] == 1
    assert p["sub_bytes"] in (64, 128, 256)
    assert p["subsequences"] == -(-p["entropy_bytes"] // p["sub_bytes"])
    assert p["sequences"] == -(-p["subsequences"] // 256)


@pytest.mark.parametrize("name", jv.RESTART)
def test_plan_serial_for_restart_files(name):
    data, _ = jv.fixture(name)
    p = lk.JpegDecoder.plan(data)
    assert p["path"] == _lib.JPEG_PATH_SERIAL and p["segments"] > 1
    assert (p["sub_bytes"], p["subsequences"], p["sequences"]) == (0, 0, 0)


@pytest.mark.parametrize("variant", [jv.with_fill_byte, jv.ending_in_ff])
def test_plan_serial_for_non_plain_streams(variant):
    data, _ = jv.fixture("444_q95")
    assert lk.JpegDecoder.plan(data)["plain"] == 1
    p = lk.JpegDecoder.plan(variant(data))
    assert p["plain"] == 0 and p["path"] == _lib.JPEG_PATH_SERIAL and p["segments"] == 1
    with pytest.raises(lk.PsnLkError):  # the model reads plain streams only
        lk.JpegDecoder.model(variant(data), 2, 16)


def _serial(data):
    coef, st = lk.JpegDecoder.model(data, 1, 0)
    assert st["path"] == _lib.JPEG_PATH_SERIAL and st["blocks"] == jv.scan_blocks(data) == coef.shape[0]
    return coef


def _check_parallel(data, ref, s):
    coef, st = lk.JpegDecoder.model(data, 2, s)
    e0, e1 = jv.entropy_range(data)
    nsub = -(-(e1 - e0) // s)
    assert st["path"] == _lib.JPEG_PATH_PARALLEL and st["sub_bytes"] == s
    assert st["subsequences"] == nsub and st["sequences"] == -(-nsub // 256)
    assert st["blocks"] == jv.scan_blocks(data)
    assert 1 <= st["sync_rounds"] <= 256 and 1 <= st["chain_rounds"] <= st["sequences"]
    np.testing.assert_array_equal(coef, ref)
    return st


@pytest.mark.parametrize("name", sorted(jv.PLAIN))
def test_model_parallel_equals_serial(name):
    data, _ = jv.fixture(name)
    ref = _serial(data)
    assert np.abs(ref).sum() > 0
    for s in SUBS:
        _check_parallel(data, ref, s)


def test_model_chain_across_sequences():
    """444_q95 at 4-byte subsequences: 1,823 subsequences in 8 sequences."""
    data, _ = jv.fixture("444_q95")
    st = _check_parallel(data, _serial(data), 4)
    assert (st["subsequences"], st["sequences"]) == (1823, 8)


@pytest.mark.parametrize("damage", [jv.truncated, jv.corrupted])
def test_model_parallel_equals_serial_on_damaged_files(oracle_mod, damage):
    data, bgr = jv.fixture("444_q95")
    bad = damage(data)
    assert lk.JpegDecoder.plan(bad)["path"] == _lib.JPEG_PATH_PARALLEL  # still plain
    assert oracle_mod.jpeg_decode_bgr(bad).shape == bgr.shape  # decodes without error
    ref = _serial(bad)
    assert not np.array_equal(ref, _serial(data))
    for s in SUBS:
        _check_parallel(bad, ref, s)


def test_model_planner_default_and_bad_requests():
    data, _ = jv.fixture("422_q90")
    coef, st = lk.JpegDecoder.model(data)  # mode 0: the planner, default subsequence size
    p = lk.JpegDecoder.plan(data)
    assert (st["path"], st["sub_bytes"], st["subsequences"]) == (p["path"], p["sub_bytes"], p["subsequences"])
    np.testing.assert_array_equal(coef, _serial(data))
    for mode, s in ((3, 0), (2, 6), (2, 2), (2, 2048), (-1, 0)):
        with pytest.raises(lk.PsnLkError):
            lk.JpegDecoder.model(data, mode, s)
    with pytest.raises(lk.PsnLkError):  # restart intervals: the serial kernel's ground
        lk.JpegDecoder.model(jv.fixture(jv.RESTART[0])[0], 1, 0)
