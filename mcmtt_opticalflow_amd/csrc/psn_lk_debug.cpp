// Timing and debug hooks of include/psn_lk.h (host side of libpsn_lk.so): the
// event rings of timed pushes and track calls and their readers, the
// kernel-variant overrides, the sample and stamp counters, psn_lk_read_level.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <vector>

#include "psn_lk_ctx.h"

using psn::LevelDev;

int psn::timer_begin(psn_lk_ctx *c, psn_lk_ctx::CallTimer &t, hipStream_t s, long &ti) {
    ti = -1;
    if (!(c->tcap && (t.calls++ % c->every) == 0)) return PSN_LK_OK;
    ti = t.n % c->tcap;
    HIPCHK(c, hipEventRecord(t.ev[2 * ti], s));
    return PSN_LK_OK;
}

int psn::timer_end(psn_lk_ctx *c, psn_lk_ctx::CallTimer &t, hipStream_t s, long ti) {
    if (ti < 0) return PSN_LK_OK;
    HIPCHK(c, hipEventRecord(t.ev[2 * ti + 1], s));
    t.n++;
    return PSN_LK_OK;
}

// The timed calls of `t` the ring holds, `cap` at the most.
static long timed_calls(const psn_lk_ctx *c, const psn_lk_ctx::CallTimer &t, long cap = LONG_MAX) {
    return std::min(std::min<long>(t.n, c->tcap), cap);
}

// The device time of the ring's timed call i, once it has ended.
static int call_ms(psn_lk_ctx *c, psn_lk_ctx::CallTimer &t, long i, float *ms) {
    HIPCHK(c, hipEventSynchronize(t.ev[2 * i + 1]));
    HIPCHK(c, hipEventElapsedTime(ms, t.ev[2 * i], t.ev[2 * i + 1]));
    return PSN_LK_OK;
}

static int sum_events(psn_lk_ctx *c, psn_lk_ctx::CallTimer &t, double *ms) {
    *ms = 0.0;
    for (long i = 0, k = timed_calls(c, t); i < k; i++) {
        float one = 0.f;
        const int rc = call_ms(c, t, i, &one);
        if (rc) return rc;
        *ms += one;
    }
    return PSN_LK_OK;
}

extern "C" {

int psn_lk_enable_timing(psn_lk_ctx *c, int capacity, int every) {
    if (!c || capacity < 0 || every < 1) return PSN_LK_ERR_ARG;
    int rc = psn_lk_sync(c);  // no timed call in flight while its events are replaced
    if (rc) return rc;
    for (auto *t : {&c->t_push, &c->t_track}) {
        for (auto e : t->ev)
            if (e) (void)hipEventDestroy(e);
        t->ev.assign(2 * (size_t)capacity, nullptr);
        // timing-only events: no system-scope fence (cache writeback/invalidate) per record
        for (auto &e : t->ev) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
        t->n = t->calls = 0;
    }
    c->tcap = capacity;
    c->track_tag.assign((size_t)capacity, 0);
    c->track_entry.assign((size_t)capacity, 0);
    c->track_slide.assign((size_t)capacity, 0);
    c->every = every;
    return PSN_LK_OK;
}

int psn_lk_timing_stats(psn_lk_ctx *c, int *n_push, double *push_ms, int *n_track, double *track_ms) {
    if (!c) return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    double pm = 0, tm = 0;
    int rc = sum_events(c, c->t_push, &pm);
    if (rc) return rc;
    rc = sum_events(c, c->t_track, &tm);
    if (rc) return rc;
    if (n_push) *n_push = (int)timed_calls(c, c->t_push);
    if (n_track) *n_track = (int)timed_calls(c, c->t_track);
    if (push_ms) *push_ms = pm;
    if (track_ms) *track_ms = tm;
    for (auto *t : {&c->t_push, &c->t_track}) t->n = t->calls = 0;
    return PSN_LK_OK;
}

int psn_lk_timing_launches(psn_lk_ctx *c, int cap, double *ms, int *tag, int *n) {
    if (!c || cap < 0 || !n || (cap > 0 && (!ms || !tag))) return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const long k = timed_calls(c, c->t_track, cap);
    for (long i = 0; i < k; i++) {
        float t = 0.f;
        const int rc = call_ms(c, c->t_track, i, &t);
        if (rc) return rc;
        ms[i] = t;
        tag[i] = c->track_tag[(size_t)i];
    }
    *n = (int)k;
    return PSN_LK_OK;
}

int psn_lk_timing_entries(psn_lk_ctx *c, int cap, int *entry, int *n) {
    if (!c || cap < 0 || !n || (cap > 0 && !entry)) return PSN_LK_ERR_ARG;
    const long k = timed_calls(c, c->t_track, cap);
    std::copy_n(c->track_entry.begin(), k, entry);
    *n = (int)k;
    return PSN_LK_OK;
}

int psn_lk_timing_slides(psn_lk_ctx *c, int cap, int *wgs, int *n) {
    if (!c || cap < 0 || !n || (cap > 0 && !wgs)) return PSN_LK_ERR_ARG;
    const long k = timed_calls(c, c->t_track, cap);
    std::copy_n(c->track_slide.begin(), k, wgs);
    *n = (int)k;
    return PSN_LK_OK;
}

int psn_lk_debug_set_variant(psn_lk_ctx *c, int key, int value) {
    if (!c) return PSN_LK_ERR_ARG;
    switch (key) {
    case PSN_LK_VARIANT_THREADS:
        if (value != 0 && value != 64 && value != 128 && value != 256 && value != 512) return PSN_LK_ERR_ARG;
        c->cfg.force_threads = value;
        return PSN_LK_OK;
    case PSN_LK_VARIANT_GENERIC: c->cfg.force_generic = value != 0; return PSN_LK_OK;
    case PSN_LK_VARIANT_ONEWAVE: c->cfg.onewave = value != 0; return PSN_LK_OK;
    case PSN_LK_VARIANT_BOX:
        c->cfg.box = value != 0;
        c->cfg.box_small = value == 2;
        return PSN_LK_OK;
    case PSN_LK_VARIANT_TILED_LDS: c->cfg.tiled_lds = std::max(16 * 1024, std::min(value, 160 * 1024 - 1024)); return PSN_LK_OK;
    case PSN_LK_VARIANT_FUSED_HELPERS: c->fused_helpers = std::max(0, value); return PSN_LK_OK;
    case PSN_LK_VARIANT_LARGE: c->cfg.force_large = value != 0; return PSN_LK_OK;
    case PSN_LK_VARIANT_LG_LDS: c->cfg.lg_lds = std::max(4 * 1024, std::min(value, 160 * 1024 - 1024)); return PSN_LK_OK;
    case PSN_LK_VARIANT_LG_JR: c->cfg.lg_jr = value != 0; return PSN_LK_OK;
    case PSN_LK_VARIANT_ST_OVL: c->cfg.st_ovl = value != 0; return PSN_LK_OK;
    case PSN_LK_VARIANT_POISON_LDS: c->poison_lds = value != 0; return PSN_LK_OK;
    case PSN_LK_VARIANT_BX_WAVES:
        if (value != 0 && value != 2 && value != 4) return PSN_LK_ERR_ARG;
        c->cfg.bx_waves = value;
        return PSN_LK_OK;
    case PSN_LK_VARIANT_FW:
        if (value != 0 && value != 1 && value != 2) return PSN_LK_ERR_ARG;
        c->cfg.fw = value;
        return PSN_LK_OK;
    case PSN_LK_VARIANT_ERR_STATUS: c->cfg.err_status_ignore = value != 0; return PSN_LK_OK;
    case PSN_LK_VARIANT_BX_PACK:
        if (value != 0 && value != 1) return PSN_LK_ERR_ARG;
        c->bx_pack = value == 0;
        return PSN_LK_OK;
    default: return PSN_LK_ERR_ARG;
    }
}

int psn_lk_debug_count_samples(psn_lk_ctx *c, int on) {
    if (!c) return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (on) {
        if (!c->d_samples) HIPCHK(c, hipMalloc(&c->d_samples, sizeof(unsigned long long)));
        HIPCHK(c, hipDeviceSynchronize());
        HIPCHK(c, hipMemset(c->d_samples, 0, sizeof(unsigned long long)));
    }
    c->count_samples = on != 0;
    return PSN_LK_OK;
}

int psn_lk_debug_read_samples(psn_lk_ctx *c, unsigned long long *out) {
    if (!c || !out) return PSN_LK_ERR_ARG;
    *out = 0;
    if (!c->d_samples) return PSN_LK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());  // launches of every stream the context was driven on
    HIPCHK(c, hipMemcpy(out, c->d_samples, sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return PSN_LK_OK;
}

int psn_lk_debug_set_stamps(psn_lk_ctx *c, void *d_stamps) {
    if (!c) return PSN_LK_ERR_ARG;
#ifdef PSN_LK_STAMPS
    c->d_stamps = (unsigned long long *)d_stamps;
    return PSN_LK_OK;
#else
    (void)d_stamps;
    return PSN_LK_ERR_UNSUPPORTED;
#endif
}

int psn_lk_read_level(psn_lk_ctx *c, int slot, int level, uint8_t *host, int stride) {
    if (!c || !host || slot < 0 || slot >= c->cfg.nslots || level < 0 || level >= c->cfg.nlevels) return PSN_LK_ERR_ARG;
    const LevelDev &L = c->h_slots[(size_t)slot * psn::kMaxLevels + level];
    if (stride < L.w) return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = psn::flush_pending(c);
    if (rc) return rc;
    rc = c->slots.wait_ready(slot, c->stream);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy2DAsync(host, stride, L.p, L.pitch, L.w, L.h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PSN_LK_OK;
}

}  // extern "C"
