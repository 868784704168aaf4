// Frame ingest of include/psn_lk.h (host side of libpsn_lk.so): the pushes of
// host, device and JPEG frames, the resize and pyramid build each one launches
// or defers, and the ordering of a slot's readers behind its build.
#include <hip/hip_runtime.h>

#include "psn_lk_ctx.h"
#include "psn_resize.h"

// The resize of a scaled context's source into its slot's gray plane (rz) and
// the standalone pyramid launch of `slot` that reads it (a), on stream s, timed
// as one push when timing is enabled; the slot's ready event is recorded after
// the build. a null: the resize alone, of a fused-mode push (the pyramid build
// it defers runs inside a later LK launch).
static int launch_build(psn_lk_ctx *c, const psn::PyrBuildArgs *a, hipStream_t s, int slot,
                        const psn::ResizeArgs *rz = nullptr) {
    long ti;
    int rc = psn::timer_begin(c, c->t_push, s, ti);
    if (rc) return rc;
    if (rz) HIPCHK(c, psn::launch_resize_gray(*rz, s));
    if (a) HIPCHK(c, psn::launch_pyramid(*a, s));
    if ((rc = psn::timer_end(c, c->t_push, s, ti))) return rc;
    return a ? c->slots.mark_built(slot, s) : PSN_LK_OK;
}

int psn::flush_pending(psn_lk_ctx *c) {
    if (!c->pend) return PSN_LK_OK;
    c->pend = false;
    return launch_build(c, &c->pend_args, c->stream, c->pend_slot);
}

int psn::begin_read(psn_lk_ctx *c, const int *slots, int n, hipStream_t on, hipEvent_t order_ev) {
    for (int i = 0; i < n; i++) {
        const int slot = slots[i];
        int rc = c->pend && slot == c->pend_slot ? flush_pending(c) : PSN_LK_OK;
        if (rc) return rc;
        if (!on) {
            rc = c->slots.wait_ready(slot, c->stream);
        } else if (c->slots.has_build(slot)) {
            rc = c->slots.wait_prev_build(slot, on);
        } else {  // no build event: order by the context stream
            HIPCHK(c, hipEventRecord(order_ev, c->stream));
            HIPCHK(c, hipStreamWaitEvent(on, order_ev, 0));
        }
        if (rc) return rc;
    }
    return PSN_LK_OK;
}

// Pyramid-build arguments of `slot` from a device source frame (the top-level
// tile of a standalone build: psn::pyr_tile_edge).
static psn::PyrBuildArgs build_args(const psn_lk_ctx *c, int slot, const uint8_t *dev, int stride, int channels) {
    psn::PyrBuildArgs a{};
    a.src = dev;
    a.src_stride = stride;
    a.channels = channels;
    a.nlevels = c->cfg.nlevels;
    a.tile = psn::pyr_tile_edge(c->cfg.nlevels - 1);
    for (int l = 0; l < c->cfg.nlevels; l++) a.lv[l] = c->h_slots[(size_t)slot * psn::kMaxLevels + l];
    return a;
}

// The resize of a source frame into `slot`'s gray plane (a scaled context).
static psn::ResizeArgs resize_args(const psn_lk_ctx *c, int slot, const uint8_t *dev, int stride, int channels) {
    psn::ResizeArgs r{};
    r.src = dev;
    r.src_stride = stride;
    r.channels = channels;
    const psn_lk_ctx::FrameClass &f = c->class_of(slot);
    r.sw = f.src_w;
    r.sh = f.src_h;
    r.dst = f.d_gray + (size_t)c->class_index(slot) * f.gray_pitch * f.h;
    r.dst_pitch = f.gray_pitch;
    r.dw = f.w;
    r.dh = f.h;
    r.xofs = f.d_rz_tab;
    r.xcoef = (const uint32_t *)(f.d_rz_tab + f.w);
    r.yofs = f.d_rz_tab + 2 * (size_t)f.w;
    r.ycoef = (const uint32_t *)(f.d_rz_tab + 2 * (size_t)f.w + f.h);
    return r;
}

// What a device frame pushed into `slot` launches: the build from the frame, or
// (a scaled context, unless the frame has the LK size already) the resize into
// the slot's gray plane and the build from that plane.
struct IngestArgs {
    bool rz;
    psn::ResizeArgs r;
    psn::PyrBuildArgs a;
};
static IngestArgs ingest_args(const psn_lk_ctx *c, int slot, const uint8_t *dev, int stride, int channels,
                              bool lk_frame = false) {
    IngestArgs g{};
    g.rz = c->class_of(slot).rz && !lk_frame;
    if (g.rz) g.r = resize_args(c, slot, dev, stride, channels);
    g.a = g.rz ? build_args(c, slot, g.r.dst, g.r.dst_pitch, 1) : build_args(c, slot, dev, stride, channels);
    return g;
}

// Resize (a scaled context) and pyramid build of `slot` from a source-size device frame, on stream s.
static int ingest_build(psn_lk_ctx *c, int slot, const uint8_t *dev, int stride, int channels, hipStream_t s) {
    const IngestArgs g = ingest_args(c, slot, dev, stride, channels);
    return launch_build(c, &g.a, s, slot, g.rz ? &g.r : nullptr);
}

// A push goes to a slot of the user ring.
static int check_user_slot(psn_lk_ctx *c, int slot) {
    if (slot < 0 || slot >= c->cfg.user_slots) return set_err(c, PSN_LK_ERR_SLOT, "slot %d out of range", slot);
    return PSN_LK_OK;
}

// The checks of a host or device frame pushed into `slot`, then the context's
// device made current. The stride is checked against the slot's class's source
// width (class 0's for a slot that check_user_slot refuses next).
static int begin_push(psn_lk_ctx *c, int slot, const uint8_t *frame, int stride, int channels) {
    if (!c || !frame || (channels != 1 && channels != 3)) return PSN_LK_ERR_ARG;
    const int width = c->fcls[slot >= 0 && slot < c->cfg.user_slots ? (size_t)c->slot_fcls[(size_t)slot] : 0].src_w;
    if (stride < width * channels) return PSN_LK_ERR_ARG;
    if (check_user_slot(c, slot)) return PSN_LK_ERR_SLOT;
    HIPCHK(c, hipSetDevice(c->device));
    return PSN_LK_OK;
}

// lk_frame: the frame has the LK size already (psn_calc_optical_flow_pyr_lk's images): no resize.
static int push_device_impl(psn_lk_ctx *c, int slot, const uint8_t *dev, int stride, int channels,
                            bool lk_frame = false) {
    int rc = psn::flush_pending(c);  // at most one deferred build
    if (rc) return rc;
    const IngestArgs g = ingest_args(c, slot, dev, stride, channels, lk_frame);
    c->filled[slot] = 1;
    if (c->overlap == PSN_LK_OVERLAP_FUSED && c->cfg.nlevels > 1) {
        if (g.rz) {
            // the resize runs now, on the LK stream, after the slot's last build (it
            // read the plane, maybe on an ingest stream); only the pyramid build is
            // deferred, and it reads the plane, not the caller's frame
            if ((rc = c->slots.wait_prev_build(slot, c->stream))) return rc;
            if ((rc = launch_build(c, nullptr, c->stream, slot, &g.r))) return rc;
        }
        c->slots.defer(slot);  // readers wait for the build by stream order (it runs first on the LK stream)
        c->pend = true;
        c->pend_slot = slot;
        c->pend_args = g.a;
        c->pend_args.tile = psn::pyr_tile_edge_fused(c->cfg.nlevels - 1);
        return PSN_LK_OK;
    }
    hipStream_t s = c->stream;
    if (c->overlap == PSN_LK_OVERLAP_STREAM) s = c->ingest_stream;  // once the slot's last readers are done
    rc = c->slots.wait_free(slot, s);
    if (rc) return rc;
    rc = c->slots.wait_prev_build(slot, s);
    if (rc) return rc;
    return launch_build(c, &g.a, s, slot, g.rz ? &g.r : nullptr);
}

// The slot's staging buffer, grown to `need` bytes once the copy and ingest
// streams are idle (the old one may still be written or read there).
static int ensure_stage(psn_lk_ctx *c, int slot, size_t need) {
    if (c->stage_cap[slot] >= need) return PSN_LK_OK;
    for (hipStream_t cs : c->copy_streams) HIPCHK(c, hipStreamSynchronize(cs));
    for (hipStream_t is : c->ingest_streams) HIPCHK(c, hipStreamSynchronize(is));
    return psn::grow_exact(c, c->d_stage[slot], c->stage_cap[slot], need);
}

// Decodes n checked frames into their slots' staging buffers in one device pass
// and builds the slots' pyramids. `batch`: through psn_jpeg_decode_batch_device
// (psn_lk_jpeg_batch_stats speaks of a batch only).
static int push_jpeg(psn_lk_ctx *c, const int *slots, const uint8_t *const *jpeg, const size_t *len, int n, bool batch) {
    HIPCHK(c, hipSetDevice(c->device));
    int rc = psn::flush_pending(c);
    if (rc) return rc;
    if (!c->jpeg) {
        if ((rc = psn_jpeg_create(c->device, &c->jpeg))) return set_err(c, rc, "psn_jpeg_create");
        psn_jpeg_set_stream(c->jpeg, c->ingest_stream);
    }
    // (each frame has its slot's class's source size: the callers checked)
    for (int i = 0; i < n; i++)
        if ((rc = ensure_stage(c, slots[i], (size_t)c->class_of(slots[i]).src_w * 3 * c->class_of(slots[i]).src_h))) return rc;
    psn_jpeg_item items[PSN_JPEG_MAX_BATCH];
    for (int i = 0; i < n; i++) {
        if ((rc = c->slots.wait_free(slots[i], c->ingest_stream))) return rc;
        // the slot's previous build may still read d_stage[slot] (an async push builds
        // on either ingest stream): the decode overwrites it only after that build
        if ((rc = c->slots.wait_prev_build(slots[i], c->ingest_stream))) return rc;
        items[i] = {jpeg[i], len[i], c->d_stage[slots[i]], c->class_of(slots[i]).src_w * 3};
    }
    rc = batch ? psn_jpeg_decode_batch_device(c->jpeg, items, n)
               : psn_jpeg_decode_device(c->jpeg, items[0].data, items[0].len, items[0].d_bgr, items[0].stride);
    if (rc) return set_err(c, rc, "JPEG decode: %s", psn_jpeg_last_error(c->jpeg));
    for (int i = 0; i < n; i++) {
        const int slot = slots[i], row = c->class_of(slot).src_w * 3;
        c->filled[slot] = 1;
        c->color_src[slot] = {c->d_stage[slot], row, 3, false, 0};
        if ((rc = ingest_build(c, slot, c->d_stage[slot], row, 3, c->ingest_stream))) return rc;
    }
    return PSN_LK_OK;
}

int psn::push_host_impl(psn_lk_ctx *c, int slot, const uint8_t *host, int stride, int channels, bool lk_frame) {
    const psn_lk_ctx::FrameClass &f = c->class_of(slot);
    const int fw = lk_frame ? f.w : f.src_w, fh = lk_frame ? f.h : f.src_h;
    const size_t row = (size_t)fw * channels, need = row * fh;
    int rc0 = flush_pending(c);  // a deferred build may still read d_src's predecessor frame
    if (rc0) return rc0;
    if ((rc0 = grow_exact(c, c->d_src, c->d_src_cap, need))) return rc0;
    // the stream the build runs on (a fused-mode build of a host frame is not deferred)
    const int mode = c->overlap;
    if (mode == PSN_LK_OVERLAP_FUSED) c->overlap = PSN_LK_OVERLAP_OFF;
    hipStream_t s = c->overlap == PSN_LK_OVERLAP_STREAM ? c->ingest_stream : c->stream;
    hipError_t ce = hipMemcpy2DAsync(c->d_src, row, host, stride, row, fh, hipMemcpyHostToDevice, s);
    int rc = ce == hipSuccess ? push_device_impl(c, slot, c->d_src, (int)row, channels, lk_frame)
                              : set_err(c, PSN_LK_ERR_HIP, "hipMemcpy2DAsync: %s", hipGetErrorString(ce));
    c->overlap = mode;
    c->src_gen++;  // d_src holds this frame now: the colour source of earlier host pushes is gone
    if (rc) return rc;
    c->color_src[slot] = {c->d_src, (int)row, channels, true, c->src_gen};
    HIPCHK(c, hipStreamSynchronize(s));  // the host frame belongs to the caller after return
    return PSN_LK_OK;
}

extern "C" {

int psn_lk_push_frame_jpeg(psn_lk_ctx *c, int slot, const uint8_t *jpeg, size_t len) {
    if (!c || !jpeg) return PSN_LK_ERR_ARG;
    if (check_user_slot(c, slot)) return PSN_LK_ERR_SLOT;
    int w = 0, h = 0;
    const int rc = psn_jpeg_info(jpeg, len, &w, &h, nullptr);
    if (rc) return set_err(c, rc, "JPEG headers");
    const psn_lk_ctx::FrameClass &f = c->class_of(slot);
    if (w != f.src_w || h != f.src_h) return set_err(c, PSN_LK_ERR_ARG, "JPEG %dx%d, context %dx%d", w, h, f.src_w, f.src_h);
    return push_jpeg(c, &slot, &jpeg, &len, 1, false);
}

int psn_lk_push_frames_jpeg(psn_lk_ctx *c, const int *slots, const uint8_t *const *jpeg, const size_t *len, int n) {
    if (!c || !slots || !jpeg || !len) return PSN_LK_ERR_ARG;
    if (n < 1 || n > PSN_JPEG_MAX_BATCH) return set_err(c, PSN_LK_ERR_ARG, "%d frames (1..%d)", n, PSN_JPEG_MAX_BATCH);
    for (int i = 0; i < n; i++) {  // every frame is checked before any slot is touched
        if (!jpeg[i]) return set_err(c, PSN_LK_ERR_ARG, "item %d: null frame", i);
        if (check_user_slot(c, slots[i])) return set_err(c, PSN_LK_ERR_SLOT, "item %d: slot %d out of range", i, slots[i]);
        for (int k = 0; k < i; k++)
            if (slots[k] == slots[i]) return set_err(c, PSN_LK_ERR_SLOT, "item %d: slot %d repeats item %d's", i, slots[i], k);
        int w = 0, h = 0;
        const int rc = psn_jpeg_info(jpeg[i], len[i], &w, &h, nullptr);
        if (rc) return set_err(c, rc, "item %d: JPEG headers", i);
        const psn_lk_ctx::FrameClass &f = c->class_of(slots[i]);
        if (w != f.src_w || h != f.src_h)
            return set_err(c, PSN_LK_ERR_ARG, "item %d: JPEG %dx%d, context %dx%d", i, w, h, f.src_w, f.src_h);
    }
    return push_jpeg(c, slots, jpeg, len, n, true);
}

int psn_lk_jpeg_last_stats(psn_lk_ctx *c, struct psn_jpeg_stats *out) {
    if (!c || !out) return PSN_LK_ERR_ARG;
    if (!c->jpeg) return set_err(c, PSN_LK_ERR_ARG, "no JPEG frame pushed yet");
    const int rc = psn_jpeg_last_stats(c->jpeg, out);
    if (rc) return set_err(c, rc, "JPEG stats: %s", psn_jpeg_last_error(c->jpeg));
    return PSN_LK_OK;
}

int psn_lk_jpeg_batch_stats(psn_lk_ctx *c, int item, struct psn_jpeg_stats *out) {
    if (!c || !out) return PSN_LK_ERR_ARG;
    if (!c->jpeg) return set_err(c, PSN_LK_ERR_ARG, "no JPEG frame pushed yet");
    const int rc = psn_jpeg_batch_stats(c->jpeg, item, out);
    if (rc) return set_err(c, rc, "JPEG stats: %s", psn_jpeg_last_error(c->jpeg));
    return PSN_LK_OK;
}

int psn_lk_push_frame_async(psn_lk_ctx *c, int slot, const uint8_t *host, int stride, int channels) {
    int rc = begin_push(c, slot, host, stride, channels);
    if (rc) return rc;
    if ((rc = psn::flush_pending(c))) return rc;
    const int src_h = c->class_of(slot).src_h;
    const size_t row = (size_t)c->class_of(slot).src_w * channels, need = row * src_h;
    if ((rc = ensure_stage(c, slot, need))) return rc;
    hipStream_t s = c->ingest_streams[c->ingest_rr++ % psn_lk_ctx::kIngestStreams];
    hipStream_t cs = c->copy_streams[c->copy_rr++ % psn_lk_ctx::kCopyStreams];
    // the staging buffer is read only by this slot's previous build (its ready
    // event); the build waits for the upload and for every read of the slot
    if ((rc = c->slots.wait_prev_build(slot, cs))) return rc;
    // ... and by a box-histogram launch (psn_lk_box_histograms, on its own stream)
    if (c->hist_stream && (rc = c->slots.wait_free_of(slot, c->hist_stream, cs))) return rc;
    if ((size_t)stride == row)  // contiguous rows: one linear copy (the DMA engine's fast path)
        HIPCHK(c, hipMemcpyAsync(c->d_stage[slot], host, need, hipMemcpyHostToDevice, cs));
    else
        HIPCHK(c, hipMemcpy2DAsync(c->d_stage[slot], row, host, stride, row, src_h, hipMemcpyHostToDevice, cs));
    HIPCHK(c, hipEventRecord(c->slots.copy_done(slot), cs));
    rc = c->slots.wait_free(slot, s);
    if (rc) return rc;
    HIPCHK(c, hipStreamWaitEvent(s, c->slots.copy_done(slot), 0));
    c->filled[slot] = 1;
    c->color_src[slot] = {c->d_stage[slot], (int)row, channels, false, 0};
    return ingest_build(c, slot, c->d_stage[slot], (int)row, channels, s);
}

int psn_lk_push_frame_device(psn_lk_ctx *c, int slot, const uint8_t *dev, int stride, int channels) {
    int rc = begin_push(c, slot, dev, stride, channels);
    if (rc) return rc;
    rc = push_device_impl(c, slot, dev, stride, channels);
    if (!rc) c->color_src[slot] = {dev, stride, channels, false, 0};
    return rc;
}

int psn_lk_push_frame(psn_lk_ctx *c, int slot, const uint8_t *host, int stride, int channels) {
    const int rc = begin_push(c, slot, host, stride, channels);
    return rc ? rc : psn::push_host_impl(c, slot, host, stride, channels);
}

}  // extern "C"
