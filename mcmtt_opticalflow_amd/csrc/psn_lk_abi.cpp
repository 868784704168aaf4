// C-ABI implementation of include/psn_lk.h (host side of libpsn_lk.so): context
// lifecycle, streams, timing, frame ingest, the track entry points and the
// debug hooks. The context is psn_lk_ctx.h; the launch planner
// psn_lk_plan.cpp; slot ordering psn_lk_slots.h; GridFAST and the box
// histograms psn_lk_readers.cpp.
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <mutex>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "psn_lk_ctx.h"
#include "psn_resize.h"

using psn::LevelDev;

static int launch_build(psn_lk_ctx *c, const psn::PyrBuildArgs &a, hipStream_t s, int slot,
                        const psn::ResizeArgs *rz = nullptr);

// Run a deferred (fused-mode) build now, as its own launch on the LK stream.
static int flush_pending(psn_lk_ctx *c) {
    if (!c->pend) return PSN_LK_OK;
    c->pend = false;
    return launch_build(c, c->pend_args, c->stream, c->pend_slot);
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

extern "C" {

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

static int cv_round(float v) { return (int)lrint((double)v); }  // cvRound: to nearest, ties to even

int psn_lk_scaled_size(int width, int height, double scale, int *lw, int *lh) {
    if (width <= 0 || height <= 0 || !(scale > 0.0) || !(scale <= 1.0)) return PSN_LK_ERR_ARG;  // (NaN fails both)
    const int w = (int)((double)width * scale), h = (int)((double)height * scale);
    if (w < 1 || h < 1) return PSN_LK_ERR_ARG;
    if (lw) *lw = w;
    if (lh) *lh = h;
    return PSN_LK_OK;
}

int psn_lk_resize_plan(int src, int dst, int *ofs, int16_t *coef, int is_x) {
    if (src <= 0 || dst <= 0 || !ofs || !coef) return PSN_LK_ERR_ARG;
    const double scale = 1.0 / ((double)dst / (double)src);
    for (int d = 0; d < dst; d++) {
        float f = (float)(((double)d + 0.5) * scale - 0.5);
        int s = (int)floorf(f);
        f -= (float)s;
        if (is_x) {
            if (s < 0) s = 0, f = 0.f;
            if (s >= src - 1) s = src - 1, f = 0.f;
        }
        ofs[d] = s;
        coef[2 * d] = (int16_t)cv_round((1.f - f) * 2048.f);
        coef[2 * d + 1] = (int16_t)cv_round(f * 2048.f);
    }
    return PSN_LK_OK;
}

// The context of psn_lk_create_classes; psn_lk_create (scale 1.0) and
// psn_lk_create_scaled are its one-class cases.
static int create_impl(int device, const psn_lk_frame_class *cls, int ncls, double scale, int max_level_cap,
                       psn_lk_ctx **out) {
    if (!out || !cls || ncls < 1 || ncls > PSN_LK_MAX_FRAME_CLASSES || max_level_cap < 0 ||
        max_level_cap > psn::kPyrMaxTop)
        return PSN_LK_ERR_ARG;
    int lk_w[PSN_LK_MAX_FRAME_CLASSES], lk_h[PSN_LK_MAX_FRAME_CLASSES], user_slots = 0;
    for (int k = 0; k < ncls; k++) {
        if (cls[k].ring_slots <= 0 || user_slots > INT32_MAX / 2 - cls[k].ring_slots) return PSN_LK_ERR_ARG;
        if (psn_lk_scaled_size(cls[k].width, cls[k].height, scale, &lk_w[k], &lk_h[k])) return PSN_LK_ERR_ARG;
        user_slots += cls[k].ring_slots;
    }
    // the pyramid tiles' LDS plan (guarded at build time for every top level:
    // psn::pyr_tiles_fit; kept here so a context never launches past the CU's LDS)
    if (psn::kStScratchBytes + psn::pyr_lds_bytes(max_level_cap, psn::pyr_tile_edge(max_level_cap)) > psn::kMaxLdsBytes)
        return PSN_LK_ERR_UNSUPPORTED;
    *out = nullptr;
    psn_lk_ctx *c = new (std::nothrow) psn_lk_ctx();
    if (!c) return PSN_LK_ERR_NOMEM;
    c->device = device;
    c->cfg.width = lk_w[0];
    c->cfg.height = lk_h[0];
    c->scale = scale;
    c->cfg.user_slots = user_slots;
    c->cfg.nslots = user_slots + 2;
    c->cfg.nlevels = max_level_cap + 1;
    c->fcls.resize((size_t)ncls);
    c->slot_fcls.assign((size_t)c->cfg.nslots, 0);
    for (int k = 0, first = 0; k < ncls; first += cls[k++].ring_slots) {
        psn_lk_ctx::FrameClass &f = c->fcls[(size_t)k];
        f.src_w = cls[k].width;
        f.src_h = cls[k].height;
        f.w = lk_w[k];
        f.h = lk_h[k];
        f.rz = f.src_w != f.w || f.src_h != f.h;
        f.first_slot = first;
        f.nslots = cls[k].ring_slots;
        for (int s = 0; s < f.nslots; s++) c->slot_fcls[(size_t)(first + s)] = k;
        if (ncls > 1) c->cfg.cls[k] = psn::PlanFrameClass{f.w, f.h, f.first_slot, f.nslots};
    }
    c->cfg.ncls = ncls > 1 ? ncls : 0;  // (one class: the planner's width x height over every slot)
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
    // slot layout: levels back to back, rows padded to 256 B (one HBM burst / 4 x 64-B lines)
    // per frame class
    for (psn_lk_ctx::FrameClass &f : c->fcls) {
        size_t slot_bytes = 0;
        int w = f.w, h = f.h;
        for (int l = 0; l < c->cfg.nlevels; l++) {
            f.ring.w[l] = w;
            f.ring.h[l] = h;
            f.ring.pitch[l] = (w + 255) & ~255;
            f.ring.off[l] = (long long)slot_bytes;
            slot_bytes += (size_t)f.ring.pitch[l] * h;
            w = (w + 1) / 2;
            h = (h + 1) / 2;
        }
        f.ring.slot_bytes = (long long)((slot_bytes + 4095) & ~(size_t)4095);
    }
    // Places in d_pyr. A kernel finds a slot at base + slot * slot_bytes of its
    // class, and class 0 owns the user slots [0, n0) and the scratch slots
    // [user_slots, user_slots + 2): its stride spans all nslots slot numbers, and
    // the other classes' slots lie in the gap between its user and its scratch
    // slots where they fit (always, when no class is larger than class 0), else
    // behind the scratch slots. One class: the nslots slots back to back.
    std::vector<size_t> place(c->fcls.size(), 0);
    size_t pyr_bytes = 0;
    {
        const size_t sb0 = (size_t)c->fcls[0].ring.slot_bytes;
        size_t gap = sb0 * c->fcls[0].nslots;
        const size_t gap_end = sb0 * c->cfg.user_slots;
        pyr_bytes = sb0 * c->cfg.nslots;
        for (size_t k = 1; k < c->fcls.size(); k++) {
            const size_t need = (size_t)c->fcls[k].ring.slot_bytes * c->fcls[k].nslots;
            size_t &at = gap + need <= gap_end ? gap : pyr_bytes;
            place[k] = at;
            at += need;
        }
    }
    // +256 B slack: the LK kernel's aligned dword staging loads may read up to
    // 3 bytes past the last row of a level
    if (hipMalloc(&c->d_pyr, pyr_bytes + 256) != hipSuccess) return fail(PSN_LK_ERR_NOMEM);
    if (hipMemset(c->d_pyr, 0, pyr_bytes + 256) != hipSuccess) return fail(PSN_LK_ERR_HIP);
    for (size_t k = 0; k < c->fcls.size(); k++) {
        psn_lk_ctx::FrameClass &f = c->fcls[k];
        // (an address below d_pyr for a class whose first slot is not 0: never dereferenced without its slot term)
        f.ring.base = (uint8_t *)((uintptr_t)c->d_pyr + place[k] - (uintptr_t)f.ring.slot_bytes * (uintptr_t)f.first_slot);
    }
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
    for (size_t k = 0; k < c->fcls.size(); k++) {
        psn_lk_ctx::FrameClass &f = c->fcls[k];
        if (!f.rz) continue;
        const int width = f.w, height = f.h, src_w = f.src_w, src_h = f.src_h;
        // the resize tables, computed once, and one gray plane per slot on the ring's 256-B pitch
        std::vector<int> ofs((size_t)std::max(width, height));
        std::vector<int16_t> coef(2 * ofs.size());
        std::vector<int> tab(2 * ((size_t)width + height));
        for (int ax = 0; ax < 2; ax++) {
            const int n = ax == 0 ? width : height;
            int *t = tab.data() + (ax == 0 ? 0 : 2 * (size_t)width);
            if (psn_lk_resize_plan(ax == 0 ? src_w : src_h, n, ofs.data(), coef.data(), ax == 0)) return fail(PSN_LK_ERR_ARG);
            for (int i = 0; i < n; i++) {
                t[i] = ofs[i];
                t[n + i] = (int)((uint32_t)(uint16_t)coef[2 * i] | ((uint32_t)(uint16_t)coef[2 * i + 1] << 16));
            }
        }
        if (hipMalloc(&f.d_rz_tab, tab.size() * sizeof(int)) != hipSuccess) return fail(PSN_LK_ERR_NOMEM);
        if (hipMemcpy(f.d_rz_tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
            return fail(PSN_LK_ERR_HIP);
        f.gray_pitch = (width + 255) & ~255;
        // (class 0: planes for its scratch slots too, as psn_lk_ctx::class_index counts them)
        const size_t bytes = (size_t)f.gray_pitch * height * (f.nslots + (k == 0 ? 2 : 0));
        if (hipMalloc(&f.d_gray, bytes) != hipSuccess) return fail(PSN_LK_ERR_NOMEM);
        if (hipMemset(f.d_gray, 0, bytes) != hipSuccess) return fail(PSN_LK_ERR_HIP);
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

int psn_lk_scale(psn_lk_ctx *c, double *s) {
    if (!c || !s) return PSN_LK_ERR_ARG;
    *s = c->scale;
    return PSN_LK_OK;
}

void psn_lk_destroy(psn_lk_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->pend && c->stream) (void)flush_pending(c);
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
    int rc = flush_pending(c);  // a deferred build belongs to the old stream's order
    if (rc) return rc;
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return PSN_LK_OK;
}

void *psn_lk_get_stream(psn_lk_ctx *c) { return c ? (void *)c->stream : nullptr; }

int psn_lk_sync(psn_lk_ctx *c) {
    if (!c) return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = flush_pending(c);
    if (rc) return rc;
    for (hipStream_t is : c->ingest_streams) HIPCHK(c, hipStreamSynchronize(is));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PSN_LK_OK;
}

int psn_lk_set_ingest_overlap(psn_lk_ctx *c, int mode) {
    if (!c || mode < PSN_LK_OVERLAP_OFF || mode > PSN_LK_OVERLAP_FUSED) return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = flush_pending(c);
    if (rc) return rc;
    c->overlap = mode;
    return PSN_LK_OK;
}

int psn_lk_enable_timing(psn_lk_ctx *c, int capacity, int every) {
    if (!c || capacity < 0 || every < 1) return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = flush_pending(c);
    if (rc) return rc;
    for (hipStream_t is : c->ingest_streams) HIPCHK(c, hipStreamSynchronize(is));
    HIPCHK(c, hipStreamSynchronize(c->stream));
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

static int sum_events(psn_lk_ctx *c, std::vector<hipEvent_t> &ev, long n, double *ms) {
    *ms = 0.0;
    const long k = std::min<long>(n, c->tcap);
    for (long i = 0; i < k; i++) {
        HIPCHK(c, hipEventSynchronize(ev[2 * i + 1]));
        float t = 0.f;
        HIPCHK(c, hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]));
        *ms += t;
    }
    return PSN_LK_OK;
}

int psn_lk_timing_stats(psn_lk_ctx *c, int *n_push, double *push_ms, int *n_track, double *track_ms) {
    if (!c) return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    double pm = 0, tm = 0;
    int rc = sum_events(c, c->t_push.ev, c->t_push.n, &pm);
    if (rc) return rc;
    rc = sum_events(c, c->t_track.ev, c->t_track.n, &tm);
    if (rc) return rc;
    if (n_push) *n_push = (int)std::min<long>(c->t_push.n, c->tcap);
    if (n_track) *n_track = (int)std::min<long>(c->t_track.n, c->tcap);
    if (push_ms) *push_ms = pm;
    if (track_ms) *track_ms = tm;
    for (auto *t : {&c->t_push, &c->t_track}) t->n = t->calls = 0;
    return PSN_LK_OK;
}

int psn_lk_timing_launches(psn_lk_ctx *c, int cap, double *ms, int *tag, int *n) {
    if (!c || cap < 0 || !n || (cap > 0 && (!ms || !tag))) return PSN_LK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const long k = std::min<long>(std::min<long>(c->t_track.n, c->tcap), cap);
    for (long i = 0; i < k; i++) {
        HIPCHK(c, hipEventSynchronize(c->t_track.ev[2 * i + 1]));
        float t = 0.f;
        HIPCHK(c, hipEventElapsedTime(&t, c->t_track.ev[2 * i], c->t_track.ev[2 * i + 1]));
        ms[i] = t;
        tag[i] = c->track_tag[(size_t)i];
    }
    *n = (int)k;
    return PSN_LK_OK;
}

int psn_lk_timing_entries(psn_lk_ctx *c, int cap, int *entry, int *n) {
    if (!c || cap < 0 || !n || (cap > 0 && !entry)) return PSN_LK_ERR_ARG;
    const long k = std::min<long>(std::min<long>(c->t_track.n, c->tcap), cap);
    for (long i = 0; i < k; i++) entry[i] = c->track_entry[(size_t)i];
    *n = (int)k;
    return PSN_LK_OK;
}

int psn_lk_timing_slides(psn_lk_ctx *c, int cap, int *wgs, int *n) {
    if (!c || cap < 0 || !n || (cap > 0 && !wgs)) return PSN_LK_ERR_ARG;
    const long k = std::min<long>(std::min<long>(c->t_track.n, c->tcap), cap);
    for (long i = 0; i < k; i++) wgs[i] = c->track_slide[(size_t)i];
    *n = (int)k;
    return PSN_LK_OK;
}

int psn_lk_level_size(psn_lk_ctx *c, int level, int *w, int *h) {
    return psn_lk_class_level_size(c, 0, level, w, h);
}

// One standalone pyramid launch of `slot` on stream s, after the resize of a
// scaled context's source into the plane `a` reads (timed when timing is
// enabled); the slot's ready event is recorded after it.
static int launch_build(psn_lk_ctx *c, const psn::PyrBuildArgs &a, hipStream_t s, int slot,
                        const psn::ResizeArgs *rz) {
    long ti;
    int rc = psn::timer_begin(c, c->t_push, s, ti);
    if (rc) return rc;
    if (rz) HIPCHK(c, psn::launch_resize_gray(*rz, s));
    HIPCHK(c, psn::launch_pyramid(a, s));
    if ((rc = psn::timer_end(c, c->t_push, s, ti))) return rc;
    return c->slots.mark_built(slot, s);
}

// Top-level tile of a standalone pyramid build (the level-0 region of a tile is
// 2^top * T + 3 * (2^top - 1) px square: larger tiles re-read less halo;
// psn::pyr_tile_edge, guarded against the LDS at build time).
// Pyramid-build arguments of `slot` from a device source frame.
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

// Resize (a scaled context) and pyramid build of `slot` from a source-size device frame, on stream s.
static int ingest_build(psn_lk_ctx *c, int slot, const uint8_t *dev, int stride, int channels, hipStream_t s) {
    if (!c->class_of(slot).rz) return launch_build(c, build_args(c, slot, dev, stride, channels), s, slot);
    const psn::ResizeArgs r = resize_args(c, slot, dev, stride, channels);
    return launch_build(c, build_args(c, slot, r.dst, r.dst_pitch, 1), s, slot, &r);
}

// The resize alone, timed as a push: a fused-mode push of a scaled context (the
// pyramid build it defers runs inside a later LK launch).
static int launch_resize(psn_lk_ctx *c, const psn::ResizeArgs &r, hipStream_t s) {
    long ti;
    int rc = psn::timer_begin(c, c->t_push, s, ti);
    if (rc) return rc;
    HIPCHK(c, psn::launch_resize_gray(r, s));
    return psn::timer_end(c, c->t_push, s, ti);
}

// The width of the frames pushed into `slot` (its class's source width; class 0's
// for a slot that check_user_slot refuses next).
static int push_width(const psn_lk_ctx *c, int slot) {
    return c->fcls[slot >= 0 && slot < c->cfg.user_slots ? (size_t)c->slot_fcls[(size_t)slot] : 0].src_w;
}

// A push goes to a slot of the user ring.
static int check_user_slot(psn_lk_ctx *c, int slot) {
    if (slot < 0 || slot >= c->cfg.user_slots) return set_err(c, PSN_LK_ERR_SLOT, "slot %d out of range", slot);
    return PSN_LK_OK;
}

// lk_frame: the frame has the LK size already (psn_calc_optical_flow_pyr_lk's images): no resize.
static int push_device_impl(psn_lk_ctx *c, int slot, const uint8_t *dev, int stride, int channels,
                            bool lk_frame = false) {
    int rc = flush_pending(c);  // at most one deferred build
    if (rc) return rc;
    const bool rz = c->class_of(slot).rz && !lk_frame;
    psn::ResizeArgs r{};
    if (rz) r = resize_args(c, slot, dev, stride, channels);
    const psn::PyrBuildArgs a = rz ? build_args(c, slot, r.dst, r.dst_pitch, 1) : build_args(c, slot, dev, stride, channels);
    c->filled[slot] = 1;
    if (c->overlap == PSN_LK_OVERLAP_FUSED && c->cfg.nlevels > 1) {
        if (rz) {
            // the resize runs now, on the LK stream, after the slot's last build (it
            // read the plane, maybe on an ingest stream); only the pyramid build is
            // deferred, and it reads the plane, not the caller's frame
            if ((rc = c->slots.wait_prev_build(slot, c->stream))) return rc;
            if ((rc = launch_resize(c, r, c->stream))) return rc;
        }
        c->slots.defer(slot);  // readers wait for the build by stream order (it runs first on the LK stream)
        c->pend = true;
        c->pend_slot = slot;
        c->pend_args = a;
        c->pend_args.tile = (c->cfg.nlevels - 1) <= 4 ? 8 : 4;  // inside the LK launch's LDS budget
        return PSN_LK_OK;
    }
    hipStream_t s = c->stream;
    if (c->overlap == PSN_LK_OVERLAP_STREAM) s = c->ingest_stream;  // once the slot's last readers are done
    rc = c->slots.wait_free(slot, s);
    if (rc) return rc;
    rc = c->slots.wait_prev_build(slot, s);
    if (rc) return rc;
    return launch_build(c, a, s, slot, rz ? &r : nullptr);
}

// The slot's staging buffer, grown to `need` bytes (the old one may still be read by the ingest stream).
static int ensure_stage(psn_lk_ctx *c, int slot, size_t need) {
    if (c->stage_cap[slot] >= need) return PSN_LK_OK;
    for (hipStream_t cs : c->copy_streams) HIPCHK(c, hipStreamSynchronize(cs));
    for (hipStream_t is : c->ingest_streams) HIPCHK(c, hipStreamSynchronize(is));
    if (c->d_stage[slot]) (void)hipFree(c->d_stage[slot]);
    c->d_stage[slot] = nullptr;
    c->stage_cap[slot] = 0;
    HIPCHK(c, hipMalloc(&c->d_stage[slot], need));
    c->stage_cap[slot] = need;
    return PSN_LK_OK;
}

// Decodes n checked frames into their slots' staging buffers in one device pass
// and builds the slots' pyramids. `batch`: through psn_jpeg_decode_batch_device
// (psn_lk_jpeg_batch_stats speaks of a batch only).
static int push_jpeg(psn_lk_ctx *c, const int *slots, const uint8_t *const *jpeg, const size_t *len, int n, bool batch) {
    HIPCHK(c, hipSetDevice(c->device));
    int rc = flush_pending(c);
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
    if (!c || !host || (channels != 1 && channels != 3) || stride < push_width(c, slot) * channels) return PSN_LK_ERR_ARG;
    if (check_user_slot(c, slot)) return PSN_LK_ERR_SLOT;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = flush_pending(c);
    if (rc) return rc;
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
    if (!c || !dev || (channels != 1 && channels != 3) || stride < push_width(c, slot) * channels) return PSN_LK_ERR_ARG;
    if (check_user_slot(c, slot)) return PSN_LK_ERR_SLOT;
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = push_device_impl(c, slot, dev, stride, channels);
    if (!rc) c->color_src[slot] = {dev, stride, channels, false, 0};
    return rc;
}

static int push_host_impl(psn_lk_ctx *c, int slot, const uint8_t *host, int stride, int channels,
                          bool lk_frame = false) {
    const psn_lk_ctx::FrameClass &f = c->class_of(slot);
    const int fw = lk_frame ? f.w : f.src_w, fh = lk_frame ? f.h : f.src_h;
    const size_t row = (size_t)fw * channels, need = row * fh;
    int rc0 = flush_pending(c);  // a deferred build may still read d_src's predecessor frame
    if (rc0) return rc0;
    if ((rc0 = psn::grow_exact(c, c->d_src, c->d_src_cap, need))) return rc0;
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

int psn_lk_push_frame(psn_lk_ctx *c, int slot, const uint8_t *host, int stride, int channels) {
    if (!c || !host || (channels != 1 && channels != 3) || stride < push_width(c, slot) * channels) return PSN_LK_ERR_ARG;
    if (check_user_slot(c, slot)) return PSN_LK_ERR_SLOT;
    HIPCHK(c, hipSetDevice(c->device));
    return push_host_impl(c, slot, host, stride, channels);
}

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
        int rc = flush_pending(c);
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
    if ((rc = flush_pending(c))) return rc;  // no launch took it (no single-tile launch)
    if ((rc = psn::timer_end(c, c->t_track, c->stream, ti))) return rc;
    // the next build into these slots waits for this launch
    return used.empty() ? PSN_LK_OK : c->slots.record_free(used.data(), (int)used.size(), c->stream);
}

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
    int rc = push_host_impl(c, sa, prev_img, stride, 1, true);
    if (rc) return rc;
    rc = push_host_impl(c, sb, next_img, stride, 1, true);
    if (rc) return rc;
    psn_lk_query q;
    q.prev_slot = sa;
    q.next_slot = sb;
    q.first_pt = 0;
    q.num_pts = npts;
    q.params = p;
    return track_host_impl(c, &q, 1, prev_pts, next_pts, status, err, true);
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
    int rc = flush_pending(c);
    if (rc) return rc;
    rc = c->slots.wait_ready(slot, c->stream);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy2DAsync(host, stride, L.p, L.pitch, L.w, L.h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PSN_LK_OK;
}

}  // extern "C"
