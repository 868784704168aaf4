// The launch planner of a track call: pure arithmetic on the frame size, the
// variant knobs and the queries. No HIP runtime call, no psn_lk_ctx: it builds
// and runs where there is no GPU (tests/cpp/lk_plan_dump.cpp).
#pragma once

#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "psn_lk.h"
#include "psn_lk_kernels.h"

namespace psn {

// The last-error text of a context (psn_lk_last_error); returns `code`.
inline int vset_err(std::string &err, int code, const char *fmt, va_list ap) {
    char buf[512];
    vsnprintf(buf, sizeof(buf), fmt, ap);
    err = buf;
    return code;
}
inline int set_err(std::string &err, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vset_err(err, code, fmt, ap);
    va_end(ap);
    return code;
}

// What the planner knows of a context: the LK frame, the ring and the
// kernel-variant overrides (psn_lk_debug_set_variant; tests and experiments only).
// One frame class of a context (psn_lk_create_classes): user slots
// [first_slot, first_slot + nslots) hold pyramids of width x height (the LK size).
struct PlanFrameClass {
    int width = 0, height = 0;
    int first_slot = 0, nslots = 0;
};

struct PlanCfg {
    int width = 0, height = 0;       // the LK size (of frame class 0)
    int nlevels = 0;                 // max_level_cap + 1
    int user_slots = 0, nslots = 0;  // user ring + 2 scratch slots (one-shot API)
    int num_cus = 256;               // compute units of the device (launch shaping)
    // THREADS = workgroup size, GENERIC = always the tiled kernel
    int force_threads = 0;
    bool force_generic = false;
    bool onewave = true;  // ONEWAVE 0: multi-wave iterations in the single-tile kernel
    bool st_ovl = true;   // ST_OVL 0 (the benchmark's st_ovl=0): every level's A phase in the single-tile prologue
    bool box = true;      // BOX 0: box windows run the row-tiled kernel instead of lk_kernel_bx
    // BOX 2: lk_kernel_bx also for the windows the single-tile kernel takes (tests:
    // box windows of one or two fallback tiles)
    bool box_small = false;
    // BX_WAVES: 0 = planner, 4 = never the two-wave box build, 2 = the two-wave
    // build wherever it fits (psn::bx_two_wave_fits)
    int bx_waves = 0;
    // FW: 0 = planner, 1 = never the forward entry (lk_kernel_fw; the benchmark's fw=1), 2 = the forward
    // entry wherever it fits (psn::bx_fw_fits)
    int fw = 0;
    // ERR_STATUS: 1 = PSN_LK_ERR_STATUS_ONLY is dropped from every query's flags
    // (the launches write err as without it; the benchmark's err_status=1)
    bool err_status_ignore = false;
    // TILED_LDS: LDS budget of a tiled-kernel workgroup (bytes); 76 KB keeps two
    // workgroups per CU (Tracker2D box windows: 64x64 backward, 64x160 forward at 1080p)
    int tiled_lds = 76 * 1024;
    // large-window kernel (lk_kernel_lg): LARGE forces it for every query;
    // lg_lds = LDS budget of one of its workgroups (row bands of the window)
    bool force_large = false;
    int lg_lds = 24 * 1024;
    bool lg_jr = true;  // LG_JR: J region of the iterations in LDS where it fits
    // Frame classes: user slots are numbered class after class, the two scratch
    // slots (user_slots, user_slots + 1) belong to class 0. ncls == 0: one class
    // of width x height over every slot.
    int ncls = 0;
    PlanFrameClass cls[PSN_LK_MAX_FRAME_CLASSES];
    // the frame class of `slot` (in [0, nslots))
    int slot_class(int slot) const {
        for (int k = 1; k < ncls; k++)
            if (slot >= cls[k].first_slot && slot < cls[k].first_slot + cls[k].nslots) return k;
        return 0;
    }
    int class_width(int k) const { return ncls ? cls[k].width : width; }
    int class_height(int k) const { return ncls ? cls[k].height : height; }
};

// Kernel classes of the planner: each track call's queries go to one launch per
// class (per box-kernel build, and per frame class: a launch carries one ring
// geometry), each launch sized for its own windows.
enum LkClass { kClsSt = 0, kClsBx = 1, kClsTiled = 2, kClsLg = 3 };

// The kernel a launch runs, as psn_lk_timing_launches reports it.
inline int kernel_tag(int cls, int key) { return cls == kClsBx ? key : cls == kClsSt ? 1 : cls == kClsTiled ? 2 : 3; }
// ... and the entry that runs it, as psn_lk_timing_entries reports it: the
// kernel's tag, but 10 * units per thread + 3 for a box build on its forward
// entry (lk_kernel_fw)
inline int entry_tag(int cls, int key, bool fw) { return cls == kClsBx && fw ? key - key % 10 + 3 : kernel_tag(cls, key); }

// One launch as planned: everything but pointers and HIP calls.
struct LkLaunchPlan {
    int cls = kClsLg;
    // box kernel: 10 * units per thread + (0 = the scalar-tail build, 1 = no-tail,
    // 2 = no-tail two-wave); large-window kernel: quads per ordered-chain tile
    int key = 0;
    int nq = 0;
    LkQueryDev q[kMaxQueries];  // wg_begin, qidx, sub_pts, sub_pstride, st_ovl / bx_hw set
    int wgs = 0;                // one workgroup per point
    int lds = 0;                // dynamic LDS bytes
    // the kernel's template selection
    int nt = 0;                    // workgroup size: lk_kernel_st, lk_kernel_bx, lk_kernel
    int ept = 0, ow_e = 0, occ = 1;  // lk_kernel_st<nt, ept, ow_e, occ>
    int upt = 0;                   // lk_kernel_bx: units per thread
    bool notail = false;           // + its no-tail build
    bool fw = false;               // + its forward entry, lk_kernel_fw<upt, notail, nt>
    int slide_wgs = 0;             // + its workgroups whose A pass slides (psn::bx_slides)
    // lk_kernel_lg<key>: int2s of one HBM window slot; the grid strides over the points
    long long lg_slot = 0;
    int grid = 0;
    // the launch may take a deferred pyramid build into its tail (the first
    // single-tile launch of an uncounted call); attaching it is the executor's part
    bool may_fuse = false;
    int fcls = 0;  // the frame class of its queries' slots: the executor passes that class's RingGeo
};

// A track call as planned.
struct LkCallPlan {
    std::vector<LkLaunchPlan> launches;  // in launch order
    std::vector<int> used_slots;         // distinct ring slots the call reads
    // kernel_tag of the (class, key) group with the most window pixels, + 1000
    // when the call has several groups; 0: nothing to launch
    int tag = 0;
    // the same with entry_tag: which entry of that kernel runs
    int entry = 0;
    // workgroups of the call whose A pass slides (psn::bx_slides; psn_lk_timing_slides)
    int slide_wgs = 0;
};

// HBM budget of one stream's large-window slots: one slot per point up to it,
// beyond it the grid strides (a slot per resident workgroup at the least)
constexpr size_t kLgWsBudget = 512ull << 20;

// Validate and plan the queries of one track call. filled[slot] != 0: the slot
// holds a frame. counted: per-query point counts on the device, count_stride
// apart. A bad query fails the call (PSN_LK_ERR_*, the text in err) before
// anything is planned for launch; `out` keeps its capacity between calls.
int plan_call(const PlanCfg &cfg, const psn_lk_query *q, int nq, const char *filled, bool allow_scratch, bool counted,
              int count_stride, LkCallPlan &out, std::string &err);

}  // namespace psn
