// The context of include/psn_lk.h (host side of libpsn_lk.so): creation from
// its layout (psn_lk_layout.cpp), destruction, the class and size accessors,
// the stream, sync and ingest-overlap controls, and the SDMA warm-up. The
// struct is psn_lk_ctx.h; pushes psn_lk_ingest.cpp; track calls
// psn_lk_track.cpp; timing and debug hooks psn_lk_debug.cpp.
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "psn_lk_ctx.h"

using psn::LevelDev;

extern "C" {

// SDMA engine set-up. ROCr creates an SDMA engine's queue on the first copy that
// engine runs: ~15 ms inside hsa_amd_memory_async_copy_on_engine, then ~0
// (tools/probes/probe_sdma_engines: 16 engines on MI355X, H2D 6 MB). The HIP
// runtime spreads async copies over the idle engines, so a frame upload that
// lands on an engine for the first time stalls its caller (the bench's first
// timed step after the device sync before the timed region: ~8 ms). Every
// engine runs one 4-KB copy each way here, once per process and device.
namespace {
struct AgentPick {
    uint32_t bdf = 0, domain = 0;
    char uuid[17] = {};  // the HIP device's UUID (16 characters), empty when HIP has none
    hsa_agent_t gpu{}, cpu{};
    int n_bdf = 0;  // GPU agents on the device's PCI function (> 1: a partitioned device)
    bool have_gpu = false, have_cpu = false, uuid_match = false;
};
hsa_status_t pick_agent(hsa_agent_t a, void *arg) {
    AgentPick *p = (AgentPick *)arg;
    hsa_device_type_t t;
    if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
    if (t == HSA_DEVICE_TYPE_CPU && !p->have_cpu) {
        p->cpu = a;
        p->have_cpu = true;
    } else if (t == HSA_DEVICE_TYPE_GPU) {
        uint32_t bdf = 0, dom = 0;
        if (hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf) != HSA_STATUS_SUCCESS ||
            hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &dom) != HSA_STATUS_SUCCESS ||
            bdf != p->bdf || dom != p->domain)
            return HSA_STATUS_SUCCESS;
        p->n_bdf++;
        // the agent's UUID ("GPU-" + 16 characters) against the HIP device's: on a
        // partitioned device several agents share the PCI function
        char u[32] = {};
        const bool um = p->uuid[0] &&
                        hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_UUID, u) == HSA_STATUS_SUCCESS &&
                        strncmp(u + 4, p->uuid, 16) == 0;
        if (!p->have_gpu || (um && !p->uuid_match)) {
            p->gpu = a;
            p->have_gpu = true;
            p->uuid_match = um;
        }
    }
    return HSA_STATUS_SUCCESS;
}
void warm_sdma_engines(int device) {
    // PSN_LK_SDMA_WARMUP=0: skipped (no create-time cost; the first upload per
    // engine then stalls once, as without the warm-up)
    const char *env = getenv("PSN_LK_SDMA_WARMUP");
    if (env && env[0] == '0') return;
    int bus = 0, dev = 0, dom = 0;
    if (hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, device) != hipSuccess ||
        hipDeviceGetAttribute(&dev, hipDeviceAttributePciDeviceId, device) != hipSuccess ||
        hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, device) != hipSuccess)
        return;
    if (hsa_init() != HSA_STATUS_SUCCESS) return;  // reference-counted: the HIP runtime's instance
    AgentPick p;
    p.bdf = ((uint32_t)bus << 8) | ((uint32_t)dev << 3);
    p.domain = (uint32_t)dom;
    {
        hipUUID hu{};
        if (hipDeviceGetUuid(&hu, device) == hipSuccess) memcpy(p.uuid, hu.bytes, 16);
    }
    hsa_iterate_agents(pick_agent, &p);
    // several agents on the PCI function and none with the HIP device's UUID: the
    // engines of an unknown partition are not warmed (no stall fix, no harm)
    if (p.n_bdf > 1 && !p.uuid_match) p.have_gpu = false;
    void *h = nullptr, *d = nullptr;
    hsa_signal_t sig{};
    if (p.have_gpu && p.have_cpu && hipHostMalloc(&h, 4096, 0) == hipSuccess && hipMalloc(&d, 4096) == hipSuccess &&
        hsa_signal_create(1, 0, nullptr, &sig) == HSA_STATUS_SUCCESS) {
        for (int dir = 0; dir < 2; dir++) {
            const hsa_agent_t da = dir == 0 ? p.gpu : p.cpu, sa = dir == 0 ? p.cpu : p.gpu;
            void *dst = dir == 0 ? d : h;
            const void *src = dir == 0 ? h : d;
            uint32_t mask = 0;
            if (hsa_amd_memory_copy_engine_status(da, sa, &mask) != HSA_STATUS_SUCCESS) continue;
            for (int e = 0; e < 32; e++) {
                if (!(mask & (1u << e))) continue;
                hsa_signal_store_relaxed(sig, 1);
                if (hsa_amd_memory_async_copy_on_engine(dst, da, src, sa, 4096, 0, nullptr, sig,
                                                        (hsa_amd_sdma_engine_id_t)(1u << e), true) == HSA_STATUS_SUCCESS)
                    hsa_signal_wait_scacquire(sig, HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED);
            }
        }
    }
    if (sig.handle) hsa_signal_destroy(sig);
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
    hsa_shut_down();
}
std::mutex g_warm_mu;
std::vector<std::pair<int, double>> g_warmed;  // devices whose engines are set up, with the wall ms it took
void warm_sdma_once(int device) {
    std::lock_guard<std::mutex> lk(g_warm_mu);
    for (const auto &w : g_warmed)
        if (w.first == device) return;
    const auto t0 = std::chrono::steady_clock::now();
    warm_sdma_engines(device);
    g_warmed.push_back({device, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()});
}
}  // namespace

int psn_lk_abi_version(void) { return PSN_LK_ABI_VERSION; }

void psn_lk_default_params(psn_lk_params *p) {
    if (!p) return;
    p->win_w = 21;
    p->win_h = 21;
    p->max_level = 3;
    p->term_type = PSN_LK_TERM_COUNT | PSN_LK_TERM_EPS;
    p->max_count = 30;
    p->epsilon = 0.01;
    p->flags = 0;
    p->min_eig_threshold = 1e-4;
}

int psn_lk_sdma_warmup_ms(int device, double *ms) {
    if (!ms) return PSN_LK_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_warm_mu);
    for (const auto &w : g_warmed)
        if (w.first == device) {
            *ms = w.second;
            return PSN_LK_OK;
        }
    *ms = 0.0;
    return PSN_LK_ERR_ARG;  // no context was created on this device yet
}

// The context of psn_lk_create_classes; psn_lk_create (scale 1.0) and
// psn_lk_create_scaled are its one-class cases.
static int create_impl(int device, const psn_lk_frame_class *cls, int ncls, double scale, int max_level_cap,
                       psn_lk_ctx **out) {
    if (!out) return PSN_LK_ERR_ARG;
    psn_lk_ctx *c = new (std::nothrow) psn_lk_ctx();
    if (!c) return PSN_LK_ERR_NOMEM;
    size_t pyr_bytes = 0;
    if (const int rc = psn::ctx_layout(cls, ncls, scale, max_level_cap, c->cfg, c->fcls, c->slot_fcls, pyr_bytes)) {
        delete c;  // (nothing of the device in it yet)
        return rc;
    }
    *out = nullptr;
    c->device = device;
    c->scale = scale;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
            c->cfg.num_cus = cus;
    }
    auto fail = [&](int rc) {
        psn_lk_destroy(c);
        return rc;
    };
    if (hipSetDevice(device) != hipSuccess) return fail(PSN_LK_ERR_HIP);
    if (psn::lk_kernels_init() != hipSuccess) return fail(PSN_LK_ERR_HIP);
    warm_sdma_once(device);  // (before any stream work: the engines' queues exist from here on)
    if (hipMalloc(&c->d_ctr, 2 * sizeof(unsigned)) != hipSuccess) return fail(PSN_LK_ERR_NOMEM);
    if (hipMemset(c->d_ctr, 0, 2 * sizeof(unsigned)) != hipSuccess) return fail(PSN_LK_ERR_HIP);
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) return fail(PSN_LK_ERR_HIP);
    c->stream = c->own_stream;
    {
        int greatest = 0;
        if (hipDeviceGetStreamPriorityRange(nullptr, &greatest) != hipSuccess) return fail(PSN_LK_ERR_HIP);
        for (hipStream_t &is : c->ingest_streams)
            if (hipStreamCreateWithPriority(&is, hipStreamNonBlocking, greatest) != hipSuccess) return fail(PSN_LK_ERR_HIP);
        c->ingest_stream = c->ingest_streams[0];
    }
    for (hipStream_t &cs : c->copy_streams)
        if (hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) return fail(PSN_LK_ERR_HIP);
    c->copy_stream = c->copy_streams[0];
    // +256 B slack: the LK kernel's aligned dword staging loads may read up to
    // 3 bytes past the last row of a level
    if (hipMalloc(&c->d_pyr, pyr_bytes + 256) != hipSuccess) return fail(PSN_LK_ERR_NOMEM);
    if (hipMemset(c->d_pyr, 0, pyr_bytes + 256) != hipSuccess) return fail(PSN_LK_ERR_HIP);
    // (an address below d_pyr for a class whose first slot is not 0: never dereferenced without its slot term)
    for (psn_lk_ctx::FrameClass &f : c->fcls)
        f.ring.base = (uint8_t *)((uintptr_t)c->d_pyr + f.place - (uintptr_t)f.ring.slot_bytes * (uintptr_t)f.first_slot);
    c->h_slots.assign((size_t)c->cfg.nslots * psn::kMaxLevels, LevelDev{nullptr, 0, 0, 0, 0});
    for (int s = 0; s < c->cfg.nslots; s++) {
        const psn::RingGeo &r = c->class_of(s).ring;
        for (int l = 0; l < c->cfg.nlevels; l++)
            c->h_slots[(size_t)s * psn::kMaxLevels + l] =
                LevelDev{(uint8_t *)((uintptr_t)r.base + (uintptr_t)r.slot_bytes * (uintptr_t)s + (uintptr_t)r.off[l]), r.w[l],
                         r.h[l], r.pitch[l], 0};
    }
    if (hipMalloc(&c->d_slots, sizeof(LevelDev) * c->h_slots.size()) != hipSuccess) return fail(PSN_LK_ERR_NOMEM);
    if (hipMemcpy(c->d_slots, c->h_slots.data(), sizeof(LevelDev) * c->h_slots.size(), hipMemcpyHostToDevice) != hipSuccess)
        return fail(PSN_LK_ERR_HIP);
    c->filled.assign(c->cfg.nslots, 0);
    c->color_src.assign(c->cfg.nslots, {});
    c->d_stage.assign(c->cfg.nslots, nullptr);
    c->stage_cap.assign(c->cfg.nslots, 0);
    if (c->slots.init(c->cfg.nslots, &c->err)) return fail(PSN_LK_ERR_HIP);
    for (psn_lk_ctx::FrameClass &f : c->fcls) {
        if (!f.rz) continue;
        const size_t tab_bytes = f.rz_tab.size() * sizeof(int);
        if (hipMalloc(&f.d_rz_tab, tab_bytes) != hipSuccess) return fail(PSN_LK_ERR_NOMEM);
        if (hipMemcpy(f.d_rz_tab, f.rz_tab.data(), tab_bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(PSN_LK_ERR_HIP);
        if (hipMalloc(&f.d_gray, f.gray_bytes) != hipSuccess) return fail(PSN_LK_ERR_NOMEM);
        if (hipMemset(f.d_gray, 0, f.gray_bytes) != hipSuccess) return fail(PSN_LK_ERR_HIP);
    }
    *out = c;
    return PSN_LK_OK;
}

int psn_lk_create(int device, int width, int height, int ring_slots, int max_level_cap, psn_lk_ctx **out) {
    const psn_lk_frame_class one{width, height, ring_slots};
    return create_impl(device, &one, 1, 1.0, max_level_cap, out);
}

int psn_lk_create_scaled(int device, int width, int height, double scale, int ring_slots, int max_level_cap,
                         psn_lk_ctx **out) {
    const psn_lk_frame_class one{width, height, ring_slots};
    return create_impl(device, &one, 1, scale, max_level_cap, out);
}

int psn_lk_create_classes(int device, const psn_lk_frame_class *cls, int ncls, double scale, int max_level_cap,
                          psn_lk_ctx **out) {
    return create_impl(device, cls, ncls, scale, max_level_cap, out);
}

int psn_lk_num_classes(psn_lk_ctx *c) { return c ? (int)c->fcls.size() : PSN_LK_ERR_ARG; }

int psn_lk_slot_class(psn_lk_ctx *c, int slot, int *cls) {
    if (!c || !cls || slot < 0 || slot >= c->cfg.nslots) return PSN_LK_ERR_ARG;
    *cls = c->slot_fcls[(size_t)slot];
    return PSN_LK_OK;
}

int psn_lk_class_slots(psn_lk_ctx *c, int cls, int *first_slot, int *nslots) {
    if (!c || cls < 0 || cls >= (int)c->fcls.size()) return PSN_LK_ERR_ARG;
    if (first_slot) *first_slot = c->fcls[(size_t)cls].first_slot;
    if (nslots) *nslots = c->fcls[(size_t)cls].nslots;
    return PSN_LK_OK;
}

int psn_lk_class_source_size(psn_lk_ctx *c, int cls, int *w, int *h) {
    if (!c || cls < 0 || cls >= (int)c->fcls.size()) return PSN_LK_ERR_ARG;
    if (w) *w = c->fcls[(size_t)cls].src_w;
    if (h) *h = c->fcls[(size_t)cls].src_h;
    return PSN_LK_OK;
}

int psn_lk_class_level_size(psn_lk_ctx *c, int cls, int level, int *w, int *h) {
    if (!c || cls < 0 || cls >= (int)c->fcls.size() || level < 0 || level >= c->cfg.nlevels) return PSN_LK_ERR_ARG;
    if (w) *w = c->fcls[(size_t)cls].ring.w[level];
    if (h) *h = c->fcls[(size_t)cls].ring.h[level];
    return PSN_LK_OK;
}

int psn_lk_source_size(psn_lk_ctx *c, int *w, int *h) { return psn_lk_class_source_size(c, 0, w, h); }

int psn_lk_level_size(psn_lk_ctx *c, int level, int *w, int *h) {
    return psn_lk_class_level_size(c, 0, level, w, h);
}

int psn_lk_scale(psn_lk_ctx *c, double *s) {
    if (!c || !s) return PSN_LK_ERR_ARG;
    *s = c->scale;
    return PSN_LK_OK;
}

void psn_lk_destroy(psn_lk_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->pend && c->stream) (void)psn::flush_pending(c);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    for (hipStream_t is : c->ingest_streams)
        if (is) (void)hipStreamSynchronize(is);
    for (hipStream_t cs : c->copy_streams)
        if (cs) (void)hipStreamSynchronize(cs);
    if (c->hist_stream) (void)hipStreamSynchronize(c->hist_stream);
    for (auto *t : {&c->t_push, &c->t_track})
        for (auto e : t->ev)
            if (e) (void)hipEventDestroy(e);
    c->slots.destroy();
    for (uint8_t *p : c->d_stage)
        if (p) (void)hipFree(p);
    if (c->jpeg) psn_jpeg_destroy(c->jpeg);
    // the last launch that used each stream's slot buffers (the current and the
    // retired ones: the stream runs in order) -- not the whole device, which
    // other contexts and groups share (a caller's stream may be gone by now, its
    // recorded event stays valid)
    for (auto &ws : c->lg_ws)
        if (ws.done) (void)hipEventSynchronize(ws.done);
    for (auto &ws : c->lg_ws) {
        if (ws.p) (void)hipFree(ws.p);
        if (ws.done) (void)hipEventDestroy(ws.done);
    }
    c->lg_ws.clear();
    for (void *p : c->lg_retired) (void)hipFree(p);
    c->lg_retired.clear();
    for (void *p : {(void *)c->d_samples, (void *)c->d_ctr, (void *)c->d_pyr, (void *)c->d_slots, (void *)c->d_src, (void *)c->d_prev, (void *)c->d_next,
                    (void *)c->d_err, (void *)c->d_status, (void *)c->d_gf_kp, (void *)c->d_gf_cnt, (void *)c->d_gf_xy,
                    (void *)c->d_gf_oc, (void *)c->d_gf_ot})
        if (p) (void)hipFree(p);
    for (const psn_lk_ctx::FrameClass &f : c->fcls)
        for (void *p : {(void *)f.d_gray, (void *)f.d_rz_tab})
            if (p) (void)hipFree(p);
    for (void *p : {(void *)c->d_hist_rects, (void *)c->d_hist_counts})
        if (p) (void)hipFree(p);
    for (void *p : {(void *)c->h_hist_rects, (void *)c->h_hist_counts})
        if (p) (void)hipHostFree(p);
    if (c->hist_ev) (void)hipEventDestroy(c->hist_ev);
    if (c->hist_stream) (void)hipStreamDestroy(c->hist_stream);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    for (hipStream_t is : c->ingest_streams)
        if (is) (void)hipStreamDestroy(is);
    for (hipStream_t cs : c->copy_streams)
        if (cs) (void)hipStreamDestroy(cs);
    delete c;
}

const char *psn_lk_last_error(psn_lk_ctx *c) { return c ? c->err.c_str() : "null context"; }

int psn_lk_set_stream(psn_lk_ctx *c, void *s) {
    if (!c) return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = psn::flush_pending(c);  // a deferred build belongs to the old stream's order
    if (rc) return rc;
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return PSN_LK_OK;
}

void *psn_lk_get_stream(psn_lk_ctx *c) { return c ? (void *)c->stream : nullptr; }

// (psn_lk_enable_timing starts from it too: the deferred build run, both ingest streams and the stream idle)
int psn_lk_sync(psn_lk_ctx *c) {
    if (!c) return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = psn::flush_pending(c);
    if (rc) return rc;
    for (hipStream_t is : c->ingest_streams) HIPCHK(c, hipStreamSynchronize(is));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PSN_LK_OK;
}

int psn_lk_set_ingest_overlap(psn_lk_ctx *c, int mode) {
    if (!c || mode < PSN_LK_OVERLAP_OFF || mode > PSN_LK_OVERLAP_FUSED) return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = psn::flush_pending(c);
    if (rc) return rc;
    c->overlap = mode;
    return PSN_LK_OK;
}

}  // extern "C"
