// The track calls of include/psn_lk.h (host side of libpsn_lk.so): the executor
// of a planned call (the planner is psn_lk_plan.cpp), the device and host entry
// points and the one-shot psn_calc_optical_flow_pyr_lk.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "psn_lk_ctx.h"

// The large-window kernel's slot buffer of the current stream, grown to `bytes`
// (to a power of two from 16 MB: the demand varies per call with the point
// count and window sizes). The outgrown buffer may still be read by launches in
// flight on the stream: it is retired, not freed, so growth never waits for
// the device (at most the geometric sum, < 2x the final size, stays reserved).
static int ensure_lg_ws(psn_lk_ctx *c, size_t bytes, void **out) {
    psn_lk_ctx::LgWs *ws = nullptr;
    for (auto &e : c->lg_ws)
        if (e.s == c->stream) ws = &e;
    if (!ws) {
        c->lg_ws.emplace_back();
        ws = &c->lg_ws.back();
        ws->s = c->stream;
    }
    if (ws->bytes < bytes) {
        size_t cap = (size_t)16 << 20;
        while (cap < bytes) cap <<= 1;
        void *p = nullptr;
        HIPCHK(c, hipMalloc(&p, cap));
        if (ws->p) c->lg_retired.push_back(ws->p);
        ws->p = p;
        ws->bytes = cap;
    }
    *out = ws->p;
    return PSN_LK_OK;
}

// One planned launch on the context stream: the pointers, the deferred pyramid
// build (single-tile kernel) or the HBM window slots (large-window kernel) it
// takes along, and the launch itself.
static int launch_plan(psn_lk_ctx *c, const psn::LkLaunchPlan &L, const float *d_prev, float *d_next,
                       uint8_t *d_status, float *d_err, const int *d_counts, int count_stride) {
    psn::LkLaunchArgs a{};
    a.slots = c->d_slots;
    a.ring = c->fcls[(size_t)L.fcls].ring;
    a.prev = d_prev;
    a.next = d_next;
    a.status = d_status;
    a.err = d_err;
    a.stamps = c->d_stamps;
    a.samples = c->count_samples ? c->d_samples : nullptr;
    a.counts = d_counts;
    a.count_stride = count_stride;
    a.nq = L.nq;
    std::copy(L.q, L.q + L.nq, a.q);
    int wgs = L.wgs, lds = L.lds;
    if (L.cls == psn::kClsSt) {
        const bool builds = L.may_fuse && c->pend;
        if (builds) {  // fuse the deferred build into this launch's tail
            int tx, ty, plds;
            psn::pyramid_grid(c->pend_args, tx, ty, plds);
            a.pyr = c->pend_args;
            a.pyr_ntiles = tx * ty;
            a.pyr_tiles_x = tx;
            a.pyr_ctr = c->d_ctr;
            // helpers start pulling tiles at once, so the build is done long before
            // the slowest points finish (tiles taken late would extend the launch)
            const int helpers = std::min(c->fused_helpers, a.pyr_ntiles);
            a.lk_wgs = wgs;
            a.total_wgs = wgs + helpers;
            wgs += helpers;
            lds = std::max(lds, psn::kStScratchBytes + plds);
            c->pend = false;
        }
        a.poison_lds = c->poison_lds ? lds : 0;
        HIPCHK(c, psn::launch_lk_st(a, wgs, L.nt, L.ept, L.ow_e, L.occ, lds, c->stream));
        // readers on other streams wait for this launch alone -- the event is
        // recorded right after it, not after the call's later launches of other classes
        return builds ? c->slots.mark_built(c->pend_slot, c->stream) : PSN_LK_OK;
    }
    if (L.cls == psn::kClsBx) {
        a.poison_lds = c->poison_lds ? lds : 0;
        HIPCHK(c, psn::launch_lk_bx(a, wgs, L.upt, L.notail, L.nt, L.fw, lds, c->bx_pack, c->stream));
        return PSN_LK_OK;
    }
    if (L.cls == psn::kClsTiled) {
        HIPCHK(c, psn::launch_lk(a, wgs, L.nt, lds, c->stream));
        return PSN_LK_OK;
    }
    void *ws = nullptr;
    int rc = ensure_lg_ws(c, (size_t)L.lg_slot * 8 * L.grid, &ws);
    if (rc) return rc;
    a.lg_ws = (int2 *)ws;
    a.lg_slot = L.lg_slot;
    a.lk_wgs = wgs;
    a.total_wgs = wgs;
    a.poison_lds = c->poison_lds ? lds : 0;
    HIPCHK(c, psn::launch_lk_lg(a, L.grid, lds, L.key, c->stream));
    for (auto &e : c->lg_ws)
        if (e.s == c->stream) {
            if (!e.done) HIPCHK(c, hipEventCreateWithFlags(&e.done, hipEventDisableTiming));
            HIPCHK(c, hipEventRecord(e.done, c->stream));
        }
    return PSN_LK_OK;
}

static int track_device_impl(psn_lk_ctx *c, const psn_lk_query *q, int nq, const float *d_prev, float *d_next,
                             uint8_t *d_status, float *d_err, bool allow_scratch, const int *d_counts = nullptr,
                             int count_stride = 1) {
    if (d_counts && c->pend) {  // early-exit workgroups cannot take part in a fused build
        int rc = psn::flush_pending(c);
        if (rc) return rc;
    }
    // a bad query fails the call before anything is launched
    psn::LkCallPlan &plan = c->plan;
    int rc = psn::plan_call(c->cfg, q, nq, c->filled.data(), allow_scratch, d_counts != nullptr, count_stride, plan, c->err);
    if (rc) return rc;
    // slots built on the ingest stream must be complete before the LK reads them;
    // a deferred build of a slot this call reads runs first, as its own launch
    const std::vector<int> &used = plan.used_slots;
    if ((rc = psn::begin_read(c, used.data(), (int)used.size()))) return rc;
    long ti;
    if ((rc = psn::timer_begin(c, c->t_track, c->stream, ti))) return rc;
    for (const psn::LkLaunchPlan &L : plan.launches)
        if ((rc = launch_plan(c, L, d_prev, d_next, d_status, d_err, d_counts, count_stride))) return rc;
    if (ti >= 0 && plan.tag) {
        c->track_tag[(size_t)ti] = plan.tag;
        c->track_entry[(size_t)ti] = plan.entry;
        c->track_slide[(size_t)ti] = plan.slide_wgs;
    }
    if ((rc = psn::flush_pending(c))) return rc;  // no launch took it (no single-tile launch)
    if ((rc = psn::timer_end(c, c->t_track, c->stream, ti))) return rc;
    // the next build into these slots waits for this launch
    return used.empty() ? PSN_LK_OK : c->slots.record_free(used.data(), (int)used.size(), c->stream);
}

static int ensure_pts(psn_lk_ctx *c, size_t n) {
    if (c->d_pts_cap >= n) return PSN_LK_OK;
    for (void *p : {(void *)c->d_prev, (void *)c->d_next, (void *)c->d_err, (void *)c->d_status})
        if (p) (void)hipFree(p);
    c->d_prev = c->d_next = c->d_err = nullptr;
    c->d_status = nullptr;
    c->d_pts_cap = 0;
    size_t cap = std::max<size_t>(n, 1024);
    HIPCHK(c, hipMalloc(&c->d_prev, cap * 2 * sizeof(float)));
    HIPCHK(c, hipMalloc(&c->d_next, cap * 2 * sizeof(float)));
    HIPCHK(c, hipMalloc(&c->d_err, cap * sizeof(float)));
    HIPCHK(c, hipMalloc(&c->d_status, cap));
    c->d_pts_cap = cap;
    return PSN_LK_OK;
}

static int track_host_impl(psn_lk_ctx *c, const psn_lk_query *q, int nq, const float *prev_xy, float *next_xy,
                           uint8_t *status, float *err, bool allow_scratch) {
    size_t npts = 0;
    bool init_flow = false;
    for (int i = 0; i < nq; i++) {
        if (q[i].num_pts < 0 || q[i].first_pt < 0) return PSN_LK_ERR_ARG;
        npts = std::max(npts, (size_t)q[i].first_pt + q[i].num_pts);
        init_flow |= (q[i].params.flags & PSN_LK_USE_INITIAL_FLOW) != 0;
    }
    if (npts == 0) return track_device_impl(c, q, nq, nullptr, nullptr, nullptr, nullptr, allow_scratch);
    int rc = ensure_pts(c, npts);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_prev, prev_xy, npts * 2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (init_flow) HIPCHK(c, hipMemcpyAsync(c->d_next, next_xy, npts * 2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    rc = track_device_impl(c, q, nq, c->d_prev, c->d_next, c->d_status, err ? c->d_err : nullptr, allow_scratch);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(next_xy, c->d_next, npts * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(status, c->d_status, npts, hipMemcpyDeviceToHost, c->stream));
    if (err) HIPCHK(c, hipMemcpyAsync(err, c->d_err, npts * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PSN_LK_OK;
}

extern "C" {

int psn_lk_track_device_counted(psn_lk_ctx *c, const psn_lk_query *q, int nq, const int *d_counts,
                                const float *d_prev, float *d_next, uint8_t *d_status, float *d_err) {
    return psn_lk_track_device_counted_strided(c, q, nq, d_counts, 1, d_prev, d_next, d_status, d_err);
}

int psn_lk_track_device_counted_strided(psn_lk_ctx *c, const psn_lk_query *q, int nq, const int *d_counts,
                                        int count_stride, const float *d_prev, float *d_next, uint8_t *d_status,
                                        float *d_err) {
    if (!c || !d_counts || count_stride < 1 || (nq > 0 && (!q || !d_prev || !d_next || !d_status)) || nq < 0)
        return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return track_device_impl(c, q, nq, d_prev, d_next, d_status, d_err, false, d_counts, count_stride);
}

int psn_lk_track_device(psn_lk_ctx *c, const psn_lk_query *q, int nq, const float *d_prev, float *d_next,
                        uint8_t *d_status, float *d_err) {
    if (!c || (nq > 0 && (!q || !d_prev || !d_next || !d_status)) || nq < 0) return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return track_device_impl(c, q, nq, d_prev, d_next, d_status, d_err, false);
}

int psn_lk_track(psn_lk_ctx *c, const psn_lk_query *q, int nq, const float *prev_xy, float *next_xy, uint8_t *status,
                 float *err) {
    if (!c || nq < 0 || (nq > 0 && !q)) return PSN_LK_ERR_ARG;
    for (int i = 0; i < nq; i++)
        if (q[i].num_pts > 0 && (!prev_xy || !next_xy || !status)) return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return track_host_impl(c, q, nq, prev_xy, next_xy, status, err, false);
}

int psn_calc_optical_flow_pyr_lk(psn_lk_ctx *c, const uint8_t *prev_img, const uint8_t *next_img, int stride,
                                 const float *prev_pts, float *next_pts, uint8_t *status, float *err, int npts,
                                 const psn_lk_params *params) {
    if (!c || !prev_img || !next_img || npts < 0 || stride < c->cfg.width) return PSN_LK_ERR_ARG;
    psn_lk_params p;
    if (params)
        p = *params;
    else
        psn_lk_default_params(&p);
    if (p.win_w <= 2 || p.win_h <= 2) return set_err(c, PSN_LK_ERR_WINSIZE, "winSize %dx%d <= 2", p.win_w, p.win_h);
    if (npts == 0) return PSN_LK_OK;  // calcOpticalFlowPyrLK releases outputs and returns
    if (!prev_pts || !next_pts || !status) return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int sa = c->cfg.user_slots, sb = c->cfg.user_slots + 1;
    int rc = psn::push_host_impl(c, sa, prev_img, stride, 1, true);
    if (rc) return rc;
    rc = psn::push_host_impl(c, sb, next_img, stride, 1, true);
    if (rc) return rc;
    psn_lk_query q;
    q.prev_slot = sa;
    q.next_slot = sb;
    q.first_pt = 0;
    q.num_pts = npts;
    q.params = p;
    return track_host_impl(c, &q, 1, prev_pts, next_pts, status, err, true);
}

}  // extern "C"
