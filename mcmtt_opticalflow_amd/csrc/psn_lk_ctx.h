// psn_lk_ctx: the context behind the C ABI of include/psn_lk.h, shared by the
// host sources of libpsn_lk.so. Internal, not installed.
//
// One psn_lk_ctx per camera replaces what CPSNWhere_Tracker2D kept for
// OpenCV: the 4-slot gray ring (m_vecPtGrayFrameBuffer, PSNWhere_Tracker2D.h:187,
// allocated at PSNWhere_Tracker2D.cpp:258-261) -- here a device ring of full
// pyramids, built ONCE per frame -- and the two calcOpticalFlowPyrLK call sites
// (:776-782, :871-877), which rebuilt both pyramids and the Scharr planes on
// every call.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "psn_lk.h"
#include "psn_jpeg.h"
#include "psn_rgbhist.h"
#include "psn_lk_kernels.h"
#include "psn_lk_layout.h"
#include "psn_lk_plan.h"
#include "psn_lk_slots.h"

struct psn_lk_ctx {
    int device = 0;
    // the LK size of class 0 (ring, pyramids, LK queries, GridFAST rois), the ring,
    // the frame classes' slots and sizes and the kernel-variant overrides: what the
    // launch planner reads
    psn::PlanCfg cfg;
    // psn_lk_create_scaled: pushed frames have the source size and are resized to
    // the LK size (PSN_2D_OPTICALFLOW_SCALE); FrameClass::rz = the sizes differ, so
    // every push runs resize_gray_kernel into the slot's gray plane and the pyramid
    // build reads that plane as a 1-channel source
    double scale = 1.0;
    // psn_lk_create_classes: per frame class its sizes, its user slots, its slot
    // layout in d_pyr (the RingGeo its launches receive: base + slot * slot_bytes
    // holds for the class's own slot numbers, for class 0 the scratch slots too)
    // and, where it resizes, its tables and gray planes. A one-class context has
    // one entry and today's layout.
    using FrameClass = psn::FrameClass;  // psn_lk_layout.h
    std::vector<FrameClass> fcls;
    std::vector<int> slot_fcls;  // [nslots] the class of every slot (scratch slots: 0)
    const FrameClass &class_of(int slot) const { return fcls[(size_t)slot_fcls[(size_t)slot]]; }
    // the slot's place among its class's slots (class 0: the scratch slots follow its user slots)
    int class_index(int slot) const {
        const FrameClass &f = class_of(slot);
        return slot >= cfg.user_slots ? f.nslots + (slot - cfg.user_slots) : slot - f.first_slot;
    }
    hipStream_t own_stream = nullptr, stream = nullptr;
    // ingest overlap: pyramid builds on their own stream, ordered against the
    // LK launches by per-slot events (psn_lk_slots.h)
    psn::SlotOrder slots;
    // psn_lk_push_frame_async builds go round-robin to kIngestStreams streams:
    // consecutive cameras' builds run side by side once their uploads land
    static constexpr int kIngestStreams = 2;
    hipStream_t ingest_streams[kIngestStreams] = {};
    hipStream_t ingest_stream = nullptr;  // ingest_streams[0]
    int ingest_rr = 0;
    // psn_lk_push_frame_async: host uploads on their own stream (copy engine), so
    // the uploads of several frames run back to back while their builds wait on
    // the ingest stream (created at the highest priority: a build gates later
    // LK launches and must not wait behind them for compute-unit slots)
    // Consecutive uploads go round-robin to kCopyStreams copy streams: the cameras
    // of a frame-set upload in parallel on two DMA engines (one engine moves a
    // 1080p BGR frame in ~0.3 ms). Two, not four: after a device sync the first
    // upload on each further copy stream held the host ~7 ms (round-4 A/B over
    // 4/2/1/0 copy streams, tools/gpu_envab.sh: 2 had the best segment median).
    static constexpr int kCopyStreams = 2;
    hipStream_t copy_streams[kCopyStreams] = {};
    hipStream_t copy_stream = nullptr;  // copy_streams[0]
    int copy_rr = 0;
    int overlap = PSN_LK_OVERLAP_OFF;
    // PSN_LK_OVERLAP_FUSED: the last pushed build is deferred and run inside
    // the next LK launch that does not read its slot (tail workgroups)
    bool pend = false;
    int pend_slot = -1;
    psn::PyrBuildArgs pend_args{};
    unsigned *d_ctr = nullptr;  // [2] fused-build work counter + finished workgroups
    int fused_helpers = 0;      // FUSED_HELPERS variant: tile-only workgroups per fused launch
    // psn_lk_push_frame_async: per-slot staging buffer of the uploaded frame
    std::vector<uint8_t *> d_stage;
    std::vector<size_t> stage_cap;
    psn::LkCallPlan plan;  // scratch of track_device_impl
    // psn_lk_box_histograms: per slot the colour source its last push read (the
    // slot's staging buffer, the caller's device frame, or the shared d_src of a
    // host push: valid while no later host push has overwritten it, src_gen)
    struct ColorSrc {
        const uint8_t *p = nullptr;
        int stride = 0, channels = 0;
        bool shared = false;  // p = d_src
        unsigned gen = 0;     // src_gen of that push
    };
    std::vector<ColorSrc> color_src;
    unsigned src_gen = 0;  // host pushes through d_src so far
    // its own stream (created at the first call): the histograms of frame t do
    // not queue behind frame t+1's LK launches
    hipStream_t hist_stream = nullptr;
    hipEvent_t hist_ev = nullptr;             // orders hist_stream after the context stream where no slot event does
    psn_rgbhist_rect *h_hist_rects = nullptr;  // pinned
    psn_rgbhist_rect *d_hist_rects = nullptr;
    uint32_t *h_hist_counts = nullptr;  // pinned
    uint32_t *d_hist_counts = nullptr;
    size_t hist_cap = 0;  // rects
    psn_jpeg_ctx *jpeg = nullptr;  // psn_lk_push_frame_jpeg's decoder (on the ingest stream)
    uint8_t *d_pyr = nullptr;
    psn::LevelDev *d_slots = nullptr;
    std::vector<psn::LevelDev> h_slots;  // [nslots][kMaxLevels]
    std::vector<char> filled;
    // staging
    uint8_t *d_src = nullptr;
    size_t d_src_cap = 0;
    float *d_prev = nullptr, *d_next = nullptr, *d_err = nullptr;
    uint8_t *d_status = nullptr;
    size_t d_pts_cap = 0;
    bool poison_lds = false;  // POISON_LDS 1: LK launches fill their LDS with a pattern first
    bool bx_pack = true;      // BX_PACK 0: two-wave and forward box launches request whole CU slots of LDS
    // the large-window kernel's window-value slots in HBM, one buffer per stream
    // (launches on one stream run in order; launches on different streams may overlap)
    struct LgWs {
        hipStream_t s = nullptr;
        void *p = nullptr;
        size_t bytes = 0;
        hipEvent_t done = nullptr;  // recorded on s after each launch that used a slot buffer of s
    };
    std::vector<LgWs> lg_ws;
    std::vector<void *> lg_retired;  // outgrown slot buffers, freed at destroy (hipFree would wait for the device)
    unsigned long long *d_stamps = nullptr;  // diagnostic build only
    unsigned long long *d_samples = nullptr;  // psn_lk_debug_count_samples
    bool count_samples = false;
    // GridFAST scratch (per-cell keypoints of one launch) and host-call outputs
    uint32_t *d_gf_kp = nullptr;
    int *d_gf_cnt = nullptr;
    size_t gf_kp_cap = 0, gf_cnt_cap = 0;
    float *d_gf_xy = nullptr;
    int *d_gf_oc = nullptr, *d_gf_ot = nullptr;
    size_t gf_out_cap = 0;  // rois x cap floats pairs
    int gf_nroi_cap = 0;
    // timing: per call kind (push, track) an event ring, 2 events per timed call
    struct CallTimer {
        std::vector<hipEvent_t> ev;
        long n = 0;      // timed calls
        long calls = 0;  // all calls since enable_timing
    };
    int tcap = 0;
    CallTimer t_push, t_track;
    std::vector<int> track_tag;  // per timed track call: the kernel it ran (psn_lk_timing_launches)
    std::vector<int> track_entry;  // ... and the entry of that kernel (psn_lk_timing_entries)
    std::vector<int> track_slide;  // ... and its workgroups on the sliding A pass (psn_lk_timing_slides)
    int every = 1;               // time every `every`-th call of each kind
    std::string err;
};

inline int set_err(psn_lk_ctx *c, int code, const char *fmt, ...) {
    if (c) {
        va_list ap;
        va_start(ap, fmt);
        psn::vset_err(c->err, code, fmt, ap);
        va_end(ap);
    }
    return code;
}

#define HIPCHK(c, expr) PSN_HIPCHK((c)->err, expr)

namespace psn {

// Before a launch reads `slots`: a deferred build of one of them runs first, as
// its own launch, then the context stream waits for each slot's last build.
// With a stream `on` of the caller's, that stream waits instead; a slot with no
// build event is ordered behind the context stream through `order_ev`.
int begin_read(psn_lk_ctx *c, const int *slots, int n, hipStream_t on = nullptr, hipEvent_t order_ev = nullptr);

// Runs a deferred (fused-mode) build now, as its own launch on the context stream (psn_lk_ingest.cpp).
int flush_pending(psn_lk_ctx *c);

// Uploads a host frame of `slot`'s source size (lk_frame: of its LK size, no
// resize) and builds the slot's pyramid; the frame is the caller's again on
// return. The slot and the device are the caller's to check (psn_lk_ingest.cpp).
int push_host_impl(psn_lk_ctx *c, int slot, const uint8_t *host, int stride, int channels, bool lk_frame = false);

// Bracket of a timed call on stream s: ti = the call's place in the ring (-1: not timed).
int timer_begin(psn_lk_ctx *c, psn_lk_ctx::CallTimer &t, hipStream_t s, long &ti);
int timer_end(psn_lk_ctx *c, psn_lk_ctx::CallTimer &t, hipStream_t s, long ti);

// A device buffer of exactly `need` elements, reallocated (contents lost) when it is smaller.
template <class T> int grow_exact(psn_lk_ctx *c, T *&p, size_t &cap, size_t need) {
    if (cap >= need) return PSN_LK_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    HIPCHK(c, hipMalloc(&p, need * sizeof(T)));
    cap = need;
    return PSN_LK_OK;
}

}  // namespace psn
