// The entry points of include/psn_lk.h that read the ring's frames beside the
// LK: GridFAST (kernels in psn_gridfast.hip) and the RGB box histograms (kernel
// in psn_rgbhist.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "psn_lk_ctx.h"
#include "psn_gridfast.h"

using psn::LevelDev;

extern "C" {

// ---- GridFAST ----

void psn_gridfast_default_params(psn_gridfast_params *p) {
    if (!p) return;
    p->threshold = 10;  // FastFeatureDetector(10, true)
    p->nonmax = 1;
    p->max_total = 1000;  // GridAdaptedFeatureDetector(detector, 1000, 4, 4)
    p->grid_rows = 4;
    p->grid_cols = 4;
    p->cap = 100;  // PSN_2D_FEATURE_MAX_NUM_TRACK (PSNWhere_Tracker2D.cpp:13)
}

// nset sets of rois, set i = nrois[i] rois on ring slot slots[i], all sets'
// rois consecutive in `rois` and in the outputs; a launch covers up to
// kGfMaxRois consecutive rois of any sets of one frame class (the shuffle key
// restarts at 0 per set): GridFastArgs has one w, h, pitch, so a set of another
// class than its predecessor's starts a new launch.
static int gridfast_impl(psn_lk_ctx *c, int nset, const int *slots, const int *nrois, const int *rois,
                         const psn_gridfast_params *pp, uint32_t seed, float *d_xy, int *d_cnt, int *d_tot) {
    psn_gridfast_params p;
    if (pp)
        p = *pp;
    else
        psn_gridfast_default_params(&p);
    const int ncell = p.grid_rows * p.grid_cols;
    if (p.grid_rows <= 0 || p.grid_cols <= 0 || ncell > 256 || p.max_total > psn::kGfMaxTotal || p.cap < 0)
        return set_err(c, PSN_LK_ERR_ARG, "gridfast: grid %dx%d, max_total %d, cap %d", p.grid_rows, p.grid_cols,
                       p.max_total, p.cap);
    for (const psn_lk_ctx::FrameClass &f : c->fcls)
        if ((f.w + p.grid_cols - 1) / p.grid_cols - 6 > psn::kGfMaxRegionW)
            return set_err(c, PSN_LK_ERR_UNSUPPORTED, "gridfast: cell width above %d", psn::kGfMaxRegionW + 6);
    int nroi = 0;
    std::vector<int> used;  // distinct slots with rois
    for (int i = 0; i < nset; i++) {
        const int slot = slots[i];
        if (slot < 0 || slot >= c->cfg.nslots || !c->filled[slot])
            return set_err(c, PSN_LK_ERR_SLOT, "slot %d not filled", slot);
        if (nrois[i] < 0) return set_err(c, PSN_LK_ERR_ARG, "gridfast: set %d has %d rois", i, nrois[i]);
        nroi += nrois[i];
        if (nrois[i] > 0 && std::find(used.begin(), used.end(), slot) == used.end()) used.push_back(slot);
    }
    if (nroi == 0) return PSN_LK_OK;
    int rc = psn::begin_read(c, used.data(), (int)used.size());  // the frames must be in the slots
    if (rc) return rc;
    std::vector<const uint8_t *> roi_img((size_t)nroi);
    std::vector<int> roi_key((size_t)nroi), roi_cls((size_t)nroi);
    for (int i = 0, k = 0; i < nset; i++)
        for (int j = 0; j < nrois[i]; j++, k++) {
            roi_img[k] = c->h_slots[(size_t)slots[i] * psn::kMaxLevels].p;
            roi_key[k] = j;
            roi_cls[k] = c->slot_fcls[(size_t)slots[i]];
        }
    psn::GridFastArgs a{};
    a.threshold = std::min(std::max(p.threshold, 0), 255);
    a.nonmax = p.nonmax ? 1 : 0;
    a.grid_rows = p.grid_rows;
    a.grid_cols = p.grid_cols;
    // GridAdaptedFeatureDetector: nothing when maxTotalKeypoints < cells
    a.per_cell = p.max_total >= ncell ? p.max_total / ncell : 0;
    a.cap = p.cap;
    a.seed = seed;
    if ((rc = psn::grow_exact(c, c->d_gf_kp, c->gf_kp_cap, (size_t)psn::kGfMaxRois * ncell * std::max(a.per_cell, 1)))) return rc;
    if ((rc = psn::grow_exact(c, c->d_gf_cnt, c->gf_cnt_cap, (size_t)psn::kGfMaxRois * ncell))) return rc;
    a.cell_kp = c->d_gf_kp;
    a.cell_cnt = c->d_gf_cnt;
    for (int base = 0, n = 0; base < nroi; base += n) {
        // the run of rois of one frame class from `base`
        n = 1;
        while (n < psn::kGfMaxRois && base + n < nroi && roi_cls[base + n] == roi_cls[base]) n++;
        const psn::RingGeo &g = c->fcls[(size_t)roi_cls[base]].ring;
        const int width = g.w[0], height = g.h[0];
        a.w = width;
        a.h = height;
        a.pitch = g.pitch[0];
        a.nroi = n;
        a.out_xy = d_xy + (size_t)base * p.cap * 2;
        a.out_count = d_cnt + base;
        a.out_total = d_tot ? d_tot + base : nullptr;
        // LDS plan: the widest region a (roi, cell) workgroup can see, the strip
        // height, the single-pass keypoint list (coordinates packed in 12 bits).
        // Strip 16 from rw_max 769 on; strip 8 and a shrunken list_cap cannot occur
        // while kGfMaxRegionW is 1024: strip 16 at rw_max 1024 with the 4096-entry
        // list is 24 * 1032 + 18 * 1026 (+ 12 to 16 B) + 16 * 1024 + 4 * 4096 = 76,016 B
        int rw_max = 1;
        const int cell_w = (width + p.grid_cols - 1) / p.grid_cols - 6;
        for (int i = 0; i < n; i++) rw_max = std::max(rw_max, std::min(rois[4 * (size_t)(base + i) + 2], cell_w));
        a.rw_max = rw_max;
        a.list_cap = (width <= 4096 && height <= 4096) ? 4096 : 0;
        a.strip = 32;
        while (a.strip > 8 && psn::gridfast_lds_bytes(rw_max, a.strip, a.list_cap) > psn::kGfMaxLds) a.strip >>= 1;
        while (a.list_cap > 0 && psn::gridfast_lds_bytes(rw_max, a.strip, a.list_cap) > psn::kGfMaxLds) a.list_cap >>= 1;
        for (int i = 0; i < n; i++) {
            const int *r = rois + 4 * (size_t)(base + i);
            // clip to the image (cropWithSize already did for the reference's rois)
            int x0 = std::max(r[0], 0), y0 = std::max(r[1], 0);
            int x1 = std::min((long long)r[0] + r[2], (long long)width) > x0 ? (int)std::min((long long)r[0] + r[2], (long long)width) : x0;
            int y1 = std::min((long long)r[1] + r[3], (long long)height) > y0 ? (int)std::min((long long)r[1] + r[3], (long long)height) : y0;
            if (r[2] <= 0 || r[3] <= 0) x1 = x0, y1 = y0;
            a.rois[i] = make_int4(x0, y0, x1 - x0, y1 - y0);
            a.roi_img[i] = roi_img[base + i];
            a.roi_key[i] = roi_key[base + i];
        }
        HIPCHK(c, psn::launch_gridfast(a, c->stream));
    }
    // a later build into these slots waits for these reads
    return c->slots.record_free(used.data(), (int)used.size(), c->stream);
}

int psn_gridfast_detect_device(psn_lk_ctx *c, int slot, const int *rois, int nroi, const psn_gridfast_params *p,
                               uint32_t seed, float *d_out_xy, int *d_out_count, int *d_out_total) {
    if (!c || nroi < 0 || (nroi > 0 && (!rois || !d_out_xy || !d_out_count))) return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return gridfast_impl(c, 1, &slot, &nroi, rois, p, seed, d_out_xy, d_out_count, d_out_total);
}

int psn_gridfast_detect_device_sets(psn_lk_ctx *c, int nset, const int *slots, const int *nrois, const int *rois,
                                    const psn_gridfast_params *p, uint32_t seed, float *d_out_xy, int *d_out_count,
                                    int *d_out_total) {
    if (!c || nset < 0 || (nset > 0 && (!slots || !nrois))) return PSN_LK_ERR_ARG;
    long long total = 0;
    for (int i = 0; i < nset; i++) total += std::max(nrois[i], 0);
    if (total > INT32_MAX || (total > 0 && (!rois || !d_out_xy || !d_out_count))) return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return gridfast_impl(c, nset, slots, nrois, rois, p, seed, d_out_xy, d_out_count, d_out_total);
}

int psn_gridfast_detect(psn_lk_ctx *c, int slot, const int *rois, int nroi, const psn_gridfast_params *pp,
                        uint32_t seed, float *out_xy, int *out_count, int *out_total) {
    if (!c || nroi < 0 || (nroi > 0 && (!rois || !out_xy || !out_count))) return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    psn_gridfast_params p;
    if (pp)
        p = *pp;
    else
        psn_gridfast_default_params(&p);
    if (nroi == 0 || p.cap < 0) return gridfast_impl(c, 1, &slot, &nroi, rois, &p, seed, nullptr, nullptr, nullptr);
    int rc = psn::grow_exact(c, c->d_gf_xy, c->gf_out_cap, (size_t)nroi * std::max(p.cap, 1) * 2);
    if (rc) return rc;
    if (c->gf_nroi_cap < nroi) {
        for (int **q : {&c->d_gf_oc, &c->d_gf_ot})
            if (*q) (void)hipFree(*q), *q = nullptr;
        c->gf_nroi_cap = 0;
        HIPCHK(c, hipMalloc(&c->d_gf_oc, (size_t)nroi * sizeof(int)));
        HIPCHK(c, hipMalloc(&c->d_gf_ot, (size_t)nroi * sizeof(int)));
        c->gf_nroi_cap = nroi;
    }
    rc = gridfast_impl(c, 1, &slot, &nroi, rois, &p, seed, c->d_gf_xy, c->d_gf_oc, c->d_gf_ot);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(out_count, c->d_gf_oc, (size_t)nroi * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (out_total)
        HIPCHK(c, hipMemcpyAsync(out_total, c->d_gf_ot, (size_t)nroi * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (p.cap > 0)
        HIPCHK(c, hipMemcpyAsync(out_xy, c->d_gf_xy, (size_t)nroi * p.cap * 2 * sizeof(float), hipMemcpyDeviceToHost,
                                 c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PSN_LK_OK;
}

// ---- RGB box histograms ----

int psn_rgbhist_device(const psn_rgbhist_rect *d_rects, int nrect, uint32_t *d_counts, void *hip_stream) {
    if (nrect < 0 || (nrect > 0 && (!d_rects || !d_counts))) return PSN_LK_ERR_ARG;
    return psn::launch_rgbhist(d_rects, nrect, d_counts, 0, (hipStream_t)hip_stream) == hipSuccess ? PSN_LK_OK
                                                                                                  : PSN_LK_ERR_HIP;
}

int psn_lk_box_histograms(psn_lk_ctx *c, int nset, const int *slots, const int *nrects, const int *rects,
                          uint32_t *counts) {
    if (!c || nset < 0 || (nset > 0 && (!slots || !nrects))) return PSN_LK_ERR_ARG;
    long long total = 0;
    for (int i = 0; i < nset; i++) {
        if (nrects[i] < 0) return set_err(c, PSN_LK_ERR_ARG, "box histograms: set %d has %d rects", i, nrects[i]);
        total += nrects[i];
    }
    if (total > INT32_MAX / psn::kRhBins || (total > 0 && (!rects || !counts))) return PSN_LK_ERR_ARG;
    std::vector<int> used;  // distinct slots with rects
    for (int i = 0; i < nset; i++) {
        const int slot = slots[i];
        if (slot < 0 || slot >= c->cfg.user_slots || !c->filled[slot] || !c->color_src[slot].p)
            return set_err(c, PSN_LK_ERR_SLOT, "box histograms: slot %d not filled", slot);
        const psn_lk_ctx::ColorSrc &cs = c->color_src[slot];
        if (cs.channels != 3)
            return set_err(c, PSN_LK_ERR_UNSUPPORTED, "box histograms: slot %d holds a %d-channel frame", slot, cs.channels);
        if (cs.shared && (cs.gen != c->src_gen || cs.p != c->d_src))
            return set_err(c, PSN_LK_ERR_SLOT, "box histograms: a later host push replaced slot %d's colour frame", slot);
        if (nrects[i] > 0 && std::find(used.begin(), used.end(), slot) == used.end()) used.push_back(slot);
    }
    if (total == 0) return PSN_LK_OK;
    const int n = (int)total;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->hist_stream) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->hist_stream, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->hist_ev, psn::kSlotEventFlags));
    }
    if (c->hist_cap < (size_t)n) {
        HIPCHK(c, hipStreamSynchronize(c->hist_stream));
        for (void **p : {(void **)&c->d_hist_rects, (void **)&c->d_hist_counts})
            if (*p) (void)hipFree(*p), *p = nullptr;
        for (void **p : {(void **)&c->h_hist_rects, (void **)&c->h_hist_counts})
            if (*p) (void)hipHostFree(*p), *p = nullptr;
        c->hist_cap = 0;
        const size_t cap = std::max<size_t>(64, (size_t)n + (size_t)n / 2);
        HIPCHK(c, hipMalloc(&c->d_hist_rects, cap * sizeof(psn_rgbhist_rect)));
        HIPCHK(c, hipMalloc(&c->d_hist_counts, cap * psn::kRhBins * sizeof(uint32_t)));
        HIPCHK(c, hipHostMalloc(&c->h_hist_rects, cap * sizeof(psn_rgbhist_rect), 0));
        HIPCHK(c, hipHostMalloc(&c->h_hist_counts, cap * psn::kRhBins * sizeof(uint32_t), 0));
        c->hist_cap = cap;
    }
    // The frames must be complete: a deferred build of a slot runs first (its
    // source is ordered by the context stream), and the slot's ready event,
    // recorded behind the build that read the source, covers the upload or decode
    // and, for a device frame, the context-stream work that produced it.
    int rc = psn::begin_read(c, used.data(), (int)used.size(), c->hist_stream, c->hist_ev);
    if (rc) return rc;
    int bands = 1;
    for (int i = 0, k = 0; i < nset; i++) {
        const psn_lk_ctx::ColorSrc &cs = c->color_src[slots[i]];
        const int sw = c->class_of(slots[i]).src_w, sh = c->class_of(slots[i]).src_h;
        for (int j = 0; j < nrects[i]; j++, k++) {
            const int *r = rects + 4 * (size_t)k;
            // the four clamps of PSNWhere_Associator3D.cpp:1161-1164, in that order
            long long x = r[0], y = r[1], w = r[2], h = r[3];
            if (x < 0) x = 0;
            if (y < 0) y = 0;
            if (x + w > sw) w = sw - x;  // (the colour frame has the source size of the slot's class)
            if (y + h > sh) h = sh - y;
            if (w <= 0 || h <= 0) x = y = w = h = 0;  // an empty crop
            c->h_hist_rects[k] = psn_rgbhist_rect{cs.p, cs.stride, (int)x, (int)y, (int)w, (int)h};
            bands = std::max(bands, psn::rgbhist_bands((int)w, (int)h));
        }
    }
    HIPCHK(c, hipMemcpyAsync(c->d_hist_rects, c->h_hist_rects, (size_t)n * sizeof(psn_rgbhist_rect), hipMemcpyHostToDevice,
                             c->hist_stream));
    HIPCHK(c, psn::launch_rgbhist(c->d_hist_rects, n, c->d_hist_counts, bands, c->hist_stream));
    // a later push into these slots overwrites their staging buffers only after this read
    rc = c->slots.record_free(used.data(), (int)used.size(), c->hist_stream);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->h_hist_counts, c->d_hist_counts, (size_t)n * psn::kRhBins * sizeof(uint32_t),
                             hipMemcpyDeviceToHost, c->hist_stream));
    HIPCHK(c, hipStreamSynchronize(c->hist_stream));
    memcpy(counts, c->h_hist_counts, (size_t)n * psn::kRhBins * sizeof(uint32_t));
    return PSN_LK_OK;
}

}  // extern "C"
