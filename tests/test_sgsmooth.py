"""Savitzky-Golay trajectory post-filter (BASELINE configs[4]
"SGSmooth post-filter"): the reference's online smoother CPSNWhere_SGSmooth
(psn_where/PSNWhere_SGSmooth.cpp) batched over many series on the GPU
(include/psn_sgsmooth.h, libpsn_lk.so).

Oracle: oracle/sgsmooth_oracle.py restates the reference; it is pinned
bit-for-bit against the reference's OWN code (oracle/_ref/libsgsmooth_ref.so,
compiled from psn_where/PSNWhere_SGSmooth.cpp by `make -C oracle ref`) when
that library is present. Bar: bit-exact doubles (same operations, same order).
"""
import ctypes
import os

import numpy as np
import pytest

import sgsmooth_oracle as sgo

CASES = [(9, 1), (7, 2), (4, 1), (1, 1), (15, 3), (2, 0)]
# the spans around the device's register path (windows <= 16) and its general
# loop (17 .. PSN_SG_MAX_SPAN = 63), even spans (window span - 1) included
LONG_CASES = [(span, degree) for span in (3, 16, 17, 18, 21, 32, 33, 62, 63) for degree in (0, 1, 3, 5)]
LONG_CASES.append((5, 7))  # degree >= span: every insert bypasses


def _ref_or_skip():
    L = sgo.ref_lib()
    if L is None:
        pytest.skip("oracle/_ref/libsgsmooth_ref.so not built (needs /root/reference)")
    return L


@pytest.mark.parametrize("w,degree", [(3, 1), (5, 1), (9, 1), (7, 2), (11, 3), (9, 0), (31, 2)] +
                         [(w, degree) for w in (17, 33, 63) for degree in range(6)])
def test_calculate_q_matches_reference(w, degree):
    L = _ref_or_skip()
    hf = (w - 1) // 2
    qb = (ctypes.c_double * max(hf * w, 1))()
    qm = (ctypes.c_double * w)()
    qe = (ctypes.c_double * max(hf * w, 1))()
    L.sgref_q(w, degree, qb, qm, qe)
    b, m, e = sgo.calculate_q(w, degree)
    assert list(qb)[:hf * w] == b and list(qm) == m and list(qe)[:hf * w] == e


@pytest.mark.parametrize("span,degree", CASES + LONG_CASES)
def test_restatement_matches_reference(span, degree):
    L = _ref_or_skip()
    rng = np.random.default_rng(span * 10 + degree)
    h = L.sgref_create(span, degree)
    try:
        s = sgo.SGSmooth(span, degree)
        # 2 * span + 12 inserts: the device's ring of `span` values has wrapped well past the span
        for k, v in enumerate((rng.normal(0, 50, max(40, 2 * span + 12)) + 300).astype(np.float32)):
            assert L.sgref_insert(h, float(v)) == s.insert(float(v))
            # the smoothed series always has one value per inserted value (the
            # reference's size() is stale after a bypass insert and starts
            # uninitialised, so the count is taken from the inserts)
            assert [L.sgref_result(h, i) for i in range(k + 1)] == s.smoothed
    finally:
        L.sgref_destroy(h)


def test_known_values():
    # degree 1, window 3: Qmid = 1/3 each; a linear ramp is reproduced exactly
    # at the ends (local line fit) and in the middle (moving average of a line)
    s = sgo.SGSmooth(3, 1)
    for v in (0.0, 3.0, 6.0, 9.0):
        s.insert(v)
    assert np.allclose(s.smoothed, [0.0, 3.0, 6.0, 9.0], atol=1e-12)
    s = sgo.SGSmooth(9, 1)
    assert s.insert(5.0) == 0 and s.insert(7.0) == 1  # bypass while the window <= degree
    assert s.smoothed == [5.0, 7.0]


@pytest.mark.gpu
@pytest.mark.parametrize("span,degree,dims", [(9, 1, 2), (7, 2, 3), (4, 1, 2), (15, 3, 1)])
def test_sg_gpu_matches_oracle(span, degree, dims):
    from mcmtt_opticalflow_amd import lk as glk

    n, T = 300, 24
    rng = np.random.default_rng(span + 100 * degree)
    sm = glk.SGSmoother(n, dims, span, degree)
    oracles = [[sgo.SGSmooth(span, degree) for _ in range(dims)] for _ in range(n)]
    try:
        for t in range(T):
            vals = (rng.normal(0, 30, (n, dims)) + 500).astype(np.float32)
            active = (rng.random(n) < 0.8).astype(np.uint8) if t % 3 == 2 else None
            ref, out = sm.insert(vals, active)
            for i in range(n):
                if active is not None and not active[i]:
                    assert ref[i] == -1
                    continue
                rs = [oracles[i][d].insert(float(vals[i, d])) for d in range(dims)]
                assert ref[i] == rs[0], (t, i)
                m = len(oracles[i][0].smoothed) - rs[0]
                for d in range(dims):
                    exp = oracles[i][d].smoothed[rs[0]:]
                    assert out[i, :m, d].tolist() == exp, (t, i, d)
        lens = sm.lengths()
        assert (lens == [len(o[0].data) for o in oracles]).all()
    finally:
        sm.close()


# (span, degree, dims): the last window of the register path, the first of the
# general loop, an even span, dims 1 / 4, degree 0, the longest span, always bypass
LONG_GPU = [(16, 1, 2), (17, 1, 2), (18, 2, 4), (21, 3, 1), (33, 0, 2), (63, 2, 2), (63, 5, 1), (5, 7, 2)]


def _kind(o, span, degree):
    """The path sg_insert_kernel takes for oracle series o's next insert."""
    w = min(span, len(o.data) + 1)
    w -= (w + 1) % 2
    if w <= degree:
        return "bypass"
    if o.qrows != w:
        return "entire"
    return "register" if w <= 16 else "general"


@pytest.mark.gpu
@pytest.mark.parametrize("span,degree,dims", LONG_GPU)
def test_sg_gpu_long_spans(monkeypatch, span, degree, dims):
    """Windows past the register path (w > 16: the general update loop and its
    ring wrap), dims 1 / 4, degree 0 and degree >= span, an `active` mask on
    every step so that series of five ages (bypass, entire, register and general
    updates) share each launch, psn_sg_reset after use. The values carry two
    unread columns, which psn_sg_insert repacks on the host: the kernel's own
    in_stride > dims is test_sg_insert_device_matches_insert's. One Python oracle per series and coordinate is the cost, so the longer
    spans run fewer series (a second workgroup up to span 33)."""
    import functools

    from mcmtt_opticalflow_amd import lk as glk

    monkeypatch.setattr(sgo, "calculate_q", functools.lru_cache(maxsize=None)(sgo.calculate_q))
    n = 300 if span <= 21 else 260 if span <= 33 else 96
    rng = np.random.default_rng(span + 100 * degree + 7)
    # five cohorts, the last one joining about 2 * span steps in, each staggered over four steps
    start = (np.arange(n) % 5) * (span // 2) + (np.arange(n) // 5) % 4
    steady = np.arange(n) % 3 == 0                # never paused: the oldest of them pass 2 * span + 8 inserts
    sm = glk.SGSmoother(n, dims, span, degree)
    mixed = 0
    try:
        for T in (min(span + 3, 14), 2 * span + 8):  # a short first use, psn_sg_reset, then past L = 2 * span
            oracles = [[sgo.SGSmooth(span, degree) for _ in range(dims)] for _ in range(n)]
            for t in range(T):
                vals = (rng.normal(0, 30, (n, dims + 2)) + 500).astype(np.float32)  # the host's in_stride = dims + 2
                active = ((t >= start) & (steady | (rng.random(n) < 0.85))).astype(np.uint8)
                kinds = {_kind(oracles[i][0], span, degree) for i in range(n) if active[i]}
                mixed += kinds >= {"bypass", "entire", "register", "general"}
                ref, out = sm.insert(vals, active)
                for i in range(n):
                    if not active[i]:
                        assert ref[i] == -1
                        continue
                    rs = [oracles[i][d].insert(float(vals[i, d])) for d in range(dims)]
                    assert ref[i] == rs[0], (t, i)
                    m = len(oracles[i][0].smoothed) - rs[0]
                    for d in range(dims):
                        assert out[i, :m, d].tolist() == oracles[i][d].smoothed[rs[0]:], (t, i, d)
            lens = sm.lengths()
            assert (lens == [len(o[0].data) for o in oracles]).all()
            assert sm._L.psn_sg_reset(sm._h) == 0
            assert (sm.lengths() == 0).all()
        assert lens.max() == 2 * span + 8 and (lens[start > 0] < lens.max()).all()
        if span > 16 and degree >= 1:  # (degree 0 never bypasses; span <= 16 has no general update)
            assert mixed > 0, "no launch held bypass, entire, register and general updates together"
    finally:
        sm.close()


@pytest.mark.gpu
def test_sg_insert_device_matches_insert(monkeypatch):
    """psn_sg_insert_device with the caller's buffers (values with in_stride =
    dims + 2 read by the kernel itself, mask, refresh, out) on a stream set by
    psn_sg_set_stream gives the oracle's values and what psn_sg_insert gives for
    the same input, through the general update path."""
    import functools

    import hiprt
    from mcmtt_opticalflow_amd import hip
    from mcmtt_opticalflow_amd import lk as glk

    n, dims, span, degree = 300, 2, 17, 1
    rng = np.random.default_rng(5)
    a, b = glk.SGSmoother(n, dims, span, degree), glk.SGSmoother(n, dims, span, degree)
    stream = hip.Stream()
    d_in, d_act = hiprt.DeviceBuffer(n * (dims + 2) * 4), hiprt.DeviceBuffer(n)
    d_ref, d_out = hiprt.DeviceBuffer(n * 4), hiprt.DeviceBuffer(n * span * dims * 8)
    length = np.zeros(n, np.int64)
    monkeypatch.setattr(sgo, "calculate_q", functools.lru_cache(maxsize=None)(sgo.calculate_q))
    oracles = [[sgo.SGSmooth(span, degree) for _ in range(dims)] for _ in range(n)]
    try:
        b.set_stream(stream.handle)
        for t in range(2 * span + 8):
            vals = (rng.normal(0, 30, (n, dims + 2)) + 500).astype(np.float32)
            active = ((t >= (np.arange(n) % 4) * 6) & ((np.arange(n) % 3 == 0) | (rng.random(n) < 0.85))).astype(np.uint8)
            ref, out = a.insert(vals, active)
            hip.memcpy_async(d_in.addr, vals.ctypes.data, vals.nbytes, hiprt.H2D, stream)
            hip.memcpy_async(d_act.addr, active.ctypes.data, active.nbytes, hiprt.H2D, stream)
            stream.synchronize()  # the pageable copies have left vals / active
            b.insert_device(d_in.addr, dims + 2, d_act.addr, d_ref.addr, d_out.addr)
            stream.synchronize()
            g_ref, g_out = d_ref.to_array((n,), np.int32), d_out.to_array((n, span, dims), np.float64)
            length += active
            np.testing.assert_array_equal(g_ref, ref)
            assert (ref[active == 0] == -1).all()
            for i in np.nonzero(active)[0]:
                m = length[i] - ref[i]
                assert 1 <= m <= span and g_out[i, :m].tolist() == out[i, :m].tolist(), (t, i)
                for d in range(dims):
                    assert oracles[i][d].insert(float(vals[i, d])) == g_ref[i], (t, i, d)
                    assert g_out[i, :m, d].tolist() == oracles[i][d].smoothed[g_ref[i]:], (t, i, d)
        assert (a.lengths() == length).all() and (b.lengths() == length).all() and length.max() == 2 * span + 8
        b.set_stream(None)
    finally:
        a.close()
        b.close()
        stream.destroy()
        for d in (d_in, d_act, d_ref, d_out):
            d.free()
