"""What a push leaves in a ring slot, bit for bit against tests/pyr_ref.py: pyr_tile
(psn_lk_pyr.h) behind pyramid_kernel and behind the fused build of lk_kernel_st
(pyr_tail), on frame sizes next to every top-level tile edge, on strips and 1..9-pixel
frames, from unscaled sources whose base or stride is off the dword grid (interior
tiles on the byte-gather fallback, gray and BGR), in every overlap mode, and slot by
slot (a build writes its own slot only; a second push replaces every tile)."""
import numpy as np
import pytest

import hiprt
import pyr_ref
from mcmtt_opticalflow_amd import _lib, hip, lk
from test_lk_gpu import assert_same, oracle_ref
from test_scale_gpu import _padded_source

pytestmark = pytest.mark.gpu

ERR_ARG = -1
MODES = (_lib.OVERLAP_OFF, _lib.OVERLAP_STREAM, _lib.OVERLAP_FUSED)


def _check_slot(ctx, slot, want, what):
    assert len(want) == ctx.max_level_cap + 1
    for lvl, ref in enumerate(want):
        assert ctx.level_size(lvl) == ref.shape[::-1], f"{what} level {lvl}"
        got = ctx.read_level(slot, lvl)
        assert got.shape == ref.shape, f"{what} level {lvl}"
        np.testing.assert_array_equal(got, ref, err_msg=f"{what} level {lvl}")


def _raw_source(w, h, ch, lead, pad, seed):
    """_padded_source's random buffer, the frame `lead` bytes in, read with the row stride of
    layout `pad` (pyr_ref.raw_stride) -> (buffer, stride, the frame as (h, w[, 3]))."""
    stride = pyr_ref.raw_stride(w, ch, pad)
    rows_needed = -(-h * stride // (w * ch + 5)) + 1  # its rows are w * ch + 5 bytes apart at least
    buf, _, _ = _padded_source(w, rows_needed, ch, lead, seed)
    assert lead + h * stride + 8 <= buf.size
    rows = buf[lead:lead + h * stride].reshape(h, stride)[:, :w * ch]
    return buf, stride, np.ascontiguousarray(rows.reshape((h, w, 3) if ch == 3 else (h, w)))


# ---------------------------------------------------------------------------
# 1. size sweep
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("cap", pyr_ref.CAPS)
def test_pyramid_size_sweep(cap):
    """Host pushes of random frames at every size of pyr_ref.sweep_sizes(cap): gray, and BGR
    for a third of them (cap 0: the 64 x 64-tile ingest-only kernel path)."""
    for i, (w, h) in enumerate(pyr_ref.sweep_sizes(cap)):
        rng = np.random.default_rng(100000 * cap + 300 * w + h)
        with lk.LKContext(w, h, ring_slots=2, max_level_cap=cap) as ctx:
            gray = rng.integers(0, 256, (h, w), dtype=np.uint8)
            ctx.push_frame(0, gray)
            _check_slot(ctx, 0, pyr_ref.pyramid(gray, cap), f"cap {cap} {w}x{h} gray")
            if pyr_ref.sweep_is_bgr(i):
                bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
                ctx.push_frame(1, bgr)
                _check_slot(ctx, 1, pyr_ref.pyramid(bgr, cap), f"cap {cap} {w}x{h} BGR")
                _check_slot(ctx, 0, pyr_ref.pyramid(gray, cap), f"cap {cap} {w}x{h} gray after the BGR push")


def test_cap_above_the_deepest_top_is_refused():
    with pytest.raises(lk.PsnLkError) as e:  # kPyrMaxTop = 5
        lk.LKContext(64, 64, ring_slots=1, max_level_cap=6)
    assert e.value.code == ERR_ARG


# ---------------------------------------------------------------------------
# 2. + 3. raw sources on the unscaled path, in every overlap mode
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("w,h,cap", pyr_ref.RAW_FRAMES)
def test_raw_sources_every_push_and_mode(w, h, cap, ch):
    """psn_lk_push_frame, psn_lk_push_frame_async and psn_lk_push_frame_device with an explicit
    stride: every layout of pyr_ref.RAW_LAYOUTS (random padding bytes), OFF, STREAM and FUSED.
    The device push reads the buffer as it lies: only lead 0 with a stride that is a multiple
    of 4 sends interior tiles through the dword loads, the rest through the byte gather."""
    pin = hip.PinnedAllocator()
    bufs = []
    try:
        with lk.LKContext(w, h, ring_slots=3, max_level_cap=cap) as ctx:
            L, hnd = ctx._L, ctx.handle
            seed = 0
            for mode in MODES:
                ctx.set_ingest_overlap(mode)
                for lead, pad in pyr_ref.RAW_LAYOUTS:
                    for push in ("host", "async", "device"):
                        seed += 1
                        buf, stride, frame = _raw_source(w, h, ch, lead, pad, 7000 * ch + 100 * cap + seed)
                        want = pyr_ref.pyramid(frame, cap)
                        slot = seed % 3
                        what = f"{w}x{h}x{ch} cap {cap} mode {mode} lead {lead} stride {stride} push {push}"
                        if push == "host":
                            ctx._check(L.psn_lk_push_frame(hnd, slot, buf.ctypes.data + lead, stride, ch), what)
                        elif push == "async":
                            pbuf = pin(buf.shape)
                            pbuf[:] = buf
                            ctx._check(L.psn_lk_push_frame_async(hnd, slot, pbuf.ctypes.data + lead, stride, ch), what)
                        else:
                            bufs.append(hiprt.DeviceBuffer.from_array(buf))
                            ctx.push_frame_device(slot, bufs[-1].addr + lead, stride, ch)
                        _check_slot(ctx, slot, want, what)
            ctx.sync()
    finally:
        for b in bufs:
            b.free()
        pin.close()


# ---------------------------------------------------------------------------
# 4. the build fused into an LK launch's tail
# ---------------------------------------------------------------------------

FUSED_SHAPES = [(261, 203, 1, 0, 0, 3), (131, 97, 3, 1, "odd", 2), (300, 270, 1, 0, 0, 5)]  # w, h, ch, lead, pad, cap


def _fused_setup(ctx, w, h, seed):
    """Slots 0 and 1 built from a texture pair; timing on; FUSED. -> (f0, f1, points)."""
    from mcmtt_opticalflow_amd import synth

    tex = synth.texture(w + 8, h + 8, seed)
    f0, f1 = np.ascontiguousarray(tex[4:4 + h, 4:4 + w]), np.ascontiguousarray(tex[3:3 + h, 2:2 + w])
    ctx.push_frame(0, f0)
    ctx.push_frame(1, f1)
    ctx.sync()
    ctx.enable_timing(16, 1)
    ctx.set_ingest_overlap(_lib.OVERLAP_FUSED)
    xs, ys = np.meshgrid(np.linspace(0, w - 1, 6), np.linspace(0, h - 1, 4))
    return f0, f1, (np.stack([xs.ravel(), ys.ravel()], 1) + 0.25).astype(np.float32)


@pytest.mark.parametrize("env", [{}, {"threads": 64}, {"threads": 128}, {"threads": 512}])
@pytest.mark.parametrize("w,h,ch,lead,pad,cap", FUSED_SHAPES)
def test_fused_build_in_the_lk_tail(oracle_mod, w, h, ch, lead, pad, cap, env):
    """A deferred device push whose build runs in the tail of a 21 x 21 lk_kernel_st launch on
    two other slots (TY = NT / 16 rows per pass at every workgroup size): the push adds no
    build launch, the launch's points are the oracle's, the slot holds pyr_ref's levels."""
    buf, stride, frame = _raw_source(w, h, ch, lead, pad, 40 + cap)
    d = hiprt.DeviceBuffer.from_array(buf)
    try:
        with lk.LKContext(w, h, ring_slots=3, max_level_cap=cap, variants=env) as ctx:
            f0, f1, pts = _fused_setup(ctx, w, h, 5)
            ctx.push_frame_device(2, d.addr + lead, stride, ch)  # deferred
            gpu = ctx.track([lk.make_query(0, 1, 0, len(pts), lk.make_params((21, 21), cap))], pts)
            ctx.sync()
            kernels = {_lib.kernel_of_tag(t) for _, t in _lib.timing_launches(ctx._L, ctx.handle, 16)}
            stats = ctx.timing_stats()
            assert kernels == {"lk_kernel_st"}
            assert (stats["n_push"], stats["n_track"]) == (0, 1), stats  # built by the LK launch, not flushed
            _check_slot(ctx, 2, pyr_ref.pyramid(frame, cap), f"fused {w}x{h}x{ch} cap {cap} {env}")
            assert ctx.timing_stats()["n_push"] == 0  # ... and nothing was left for the reads to flush
            assert_same(gpu, oracle_ref(oracle_mod, f0, f1, pts, (21, 21), cap), f"fused launch {env}")
            _check_slot(ctx, 0, pyr_ref.pyramid(f0, cap), "slot 0 after the fused build")
            _check_slot(ctx, 1, pyr_ref.pyramid(f1, cap), "slot 1 after the fused build")
    finally:
        d.free()


@pytest.mark.parametrize("w,h,ch,lead,pad,cap", FUSED_SHAPES)
def test_deferred_build_flushed_by_a_read(w, h, ch, lead, pad, cap):
    """read_level right after the deferred push: the build runs as its own launch (pend_args.tile)."""
    buf, stride, frame = _raw_source(w, h, ch, lead, pad, 60 + cap)
    d = hiprt.DeviceBuffer.from_array(buf)
    try:
        with lk.LKContext(w, h, ring_slots=3, max_level_cap=cap) as ctx:
            _fused_setup(ctx, w, h, 6)
            ctx.push_frame_device(2, d.addr + lead, stride, ch)
            assert ctx.timing_stats()["n_push"] == 0  # deferred
            _check_slot(ctx, 2, pyr_ref.pyramid(frame, cap), f"flushed {w}x{h}x{ch} cap {cap}")
            assert ctx.timing_stats()["n_push"] == 1  # one build launch, by the first read
    finally:
        d.free()


# ---------------------------------------------------------------------------
# 5. slots
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [_lib.OVERLAP_OFF, _lib.OVERLAP_FUSED])
def test_slot_isolation_and_replacement(mode):
    """A to slots 0 and 2, then B to slot 1: 0 and 2 still hold A. Then C to slot 1: every
    level is C's (in FUSED mode the device pushes are deferred and flushed by the next push
    or read)."""
    W, H, cap = 261, 203, 3
    rng = np.random.default_rng(77)
    A, B, C = (rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(3))
    pA, pB, pC = (pyr_ref.pyramid(f, cap) for f in (A, B, C))
    dev = [hiprt.DeviceBuffer.from_array(f) for f in (A, B, C)]
    try:
        with lk.LKContext(W, H, ring_slots=4, max_level_cap=cap) as ctx:
            ctx.set_ingest_overlap(mode)

            def push(slot, k):
                if mode == _lib.OVERLAP_FUSED:
                    ctx.push_frame_device(slot, dev[k].addr, W, 1)
                else:
                    ctx.push_frame(slot, (A, B, C)[k])

            push(0, 0)
            push(2, 0)
            push(1, 1)
            for slot, want in ((0, pA), (2, pA), (1, pB), (0, pA)):
                _check_slot(ctx, slot, want, f"mode {mode} slot {slot} after B")
            push(1, 2)
            for slot, want in ((1, pC), (0, pA), (2, pA)):
                _check_slot(ctx, slot, want, f"mode {mode} slot {slot} after C")
            ctx.sync()
    finally:
        for d in dev:
            d.free()
