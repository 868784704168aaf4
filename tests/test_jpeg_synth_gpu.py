"""The device entropy decode (jpeg_sync_kernel, jpeg_chain_kernel, jpeg_emit_kernel,
jpeg_dc_kernel, and the serial jpeg_entropy_kernel) on the synthesised streams of
tests/jpeg_synth.py, whose properties test_jpeg_synth.py asserts on the CPU.

Coefficients are read back (JpegDecoder.coefficients) and compared with the array
the stream was written from -- for an ill-formed stream, with the serial CPU
model. Pixels equal the oracle's. The kernels' counters equal the CPU model's
field for field: the model emulates the kernels' barrier-ordered rounds one for
one, so equality is the specification."""
import time

import numpy as np
import pytest

import jpeg_synth as js
from mcmtt_opticalflow_amd import lk

pytestmark = pytest.mark.gpu

SUBS = [4, 16, 128, 256, 1024]  # 256 and 1024: above the LDS staging limit, bytes read from global memory
DECODERS = [(2, s) for s in SUBS] + [(0, 0), (1, 0)]  # forced sizes, the planner's default, the serial kernel
STAT_FIELDS = ("path", "sub_bytes", "subsequences", "sequences", "sync_rounds", "chain_rounds", "blocks")

_model_cache = {}


def _model(name, mode, s):
    """The CPU model's (coefficients, stats) of a case, computed once."""
    key = (name, mode, s)
    if key not in _model_cache:
        _model_cache[key] = lk.JpegDecoder.model(js.case(name).data, mode, s)
    return _model_cache[key]


@pytest.fixture(scope="module")
def decoders():
    """One context per (mode, sub_bytes), shared by every case of the module: each
    decode also follows some other case's on the same context."""
    decs = {key: lk.JpegDecoder(entropy=key[0], sub_bytes=key[1]) for key in DECODERS}
    yield decs
    for d in decs.values():
        d.close()


@pytest.fixture(scope="module")
def oracle_pixels(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = oracle_mod.jpeg_decode_bgr(js.case(name).data)
        return cache[name]

    return get


def _check(dec, name, mode, s, oracle_pixels):
    c = js.case(name)
    tag = f"{name} entropy={mode} sub_bytes={s}"
    got = dec.decode(c.data)
    coef, st = dec.coefficients(), dec.stats()
    ref = c.coefs if c.intact else _model(name, 1, 0)[0]
    np.testing.assert_array_equal(coef, ref, err_msg=tag)
    np.testing.assert_array_equal(got, oracle_pixels(name), err_msg=tag)
    want = _model(name, mode, s)[1]
    assert {k: st[k] for k in STAT_FIELDS} == {k: want[k] for k in STAT_FIELDS}, tag
    return st


@pytest.mark.parametrize("name", js.SMALL_INTACT + js.ILL_FORMED_CASES)
def test_device_equals_input_oracle_and_model(decoders, oracle_pixels, name):
    for mode, s in DECODERS:
        _check(decoders[(mode, s)], name, mode, s, oracle_pixels)


def test_cold_start_behind_a_stuffed_zero(decoders, oracle_pixels):
    """stuffed_starts: every subsequence's cold state is its true state, half of
    them behind a stuffed zero, one of those the first of a workgroup (its look
    back leaves the staged window): round 0 is right, round 1 confirms it."""
    st = _check(decoders[(2, 4)], "stuffed_starts", 2, 4, oracle_pixels)
    assert (st["sequences"], st["sync_rounds"], st["chain_rounds"]) == (2, 2, 1), st


def test_multipass_two_chain_passes(decoders, oracle_pixels):
    """1.08 MiB of entropy bytes: 1,101 sequences at 4-byte subsequences, so
    jpeg_chain_kernel runs two passes with a carry between them. The serial
    kernel (one thread for 350,000 symbols) is left to the smaller cases."""
    js.case("multipass")
    t0 = time.perf_counter()
    for mode, s in ((2, 4), (2, 128), (0, 0)):
        t1 = time.perf_counter()
        st = _check(decoders[(mode, s)], "multipass", mode, s, oracle_pixels)
        print(f"multipass entropy={mode} sub_bytes={s}: {time.perf_counter() - t1:.3f} s {st}")
        if s == 4:
            assert st["sequences"] > 1024
    print(f"multipass on the device, three decoders with their checks: {time.perf_counter() - t0:.3f} s")


@pytest.mark.parametrize("mode,s", DECODERS)
def test_context_carries_nothing_over(oracle_pixels, mode, s):
    """A fresh context decodes a larger case, then a smaller one with other tables
    and geometry: states, block counts and the zeroed coefficient buffer of the
    first leave no trace in the second."""
    with lk.JpegDecoder(entropy=mode, sub_bytes=s) as dec:
        with pytest.raises(lk.PsnLkError):
            dec.coefficients()  # nothing decoded yet
        for name in ("ladder_ff", "ambiguous444", "truncated_ambiguous444", "zrl", "geometry_420_7x9"):
            _check(dec, name, mode, s, oracle_pixels)


def test_read_back_rejects_a_wrong_count():
    c = js.case("zrl")
    with lk.JpegDecoder() as dec:
        dec.decode(c.data)
        buf = np.empty(c.coefs.size + 64, np.int16)
        for count in (0, c.coefs.size - 64, c.coefs.size + 64):
            assert dec._L.psn_jpeg_debug_read_coefficients(dec._h, buf.ctypes.data, count) == -1
        assert dec._L.psn_jpeg_debug_read_coefficients(dec._h, None, c.coefs.size) == -1
        assert dec._L.psn_jpeg_debug_read_coefficients(dec._h, buf.ctypes.data, c.coefs.size) == 0
        np.testing.assert_array_equal(buf[:c.coefs.size].reshape(-1, 64), c.coefs)
