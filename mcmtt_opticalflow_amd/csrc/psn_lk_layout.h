// The layout of a context (psn_lk_create_classes): per frame class its sizes,
// slots, pyramid levels, place in the pyramid allocation, gray planes and
// resize table, and what the launch planner reads of them. Pure arithmetic on
// the create arguments: no HIP runtime call, no psn_lk_ctx, so it builds and
// runs where there is no GPU (tests/cpp/ctx_layout_dump.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "psn_lk.h"
#include "psn_lk_kernels.h"
#include "psn_lk_plan.h"

namespace psn {

// One frame class of a context: what ctx_layout computes, and the device
// pointers psn_lk_create_classes adds (ring.base, d_gray, d_rz_tab).
struct FrameClass {
    int src_w = 0, src_h = 0;  // pushed frames
    int w = 0, h = 0;          // the LK size
    bool rz = false;           // the sizes differ: every push resizes into the slot's gray plane
    int first_slot = 0, nslots = 0;  // its user slots
    // the RingGeo its launches receive; base = d_pyr + place - slot_bytes * first_slot,
    // so that base + slot * slot_bytes holds for the class's own slot numbers
    RingGeo ring{};
    size_t place = 0;  // bytes from d_pyr to the class's first slot
    // rz only: one gray plane of h rows per slot of the class (class 0: two more, for
    // its scratch slots, as psn_lk_ctx::class_index counts them), gray_pitch apart
    uint8_t *d_gray = nullptr;
    int gray_pitch = 0;
    size_t gray_bytes = 0;
    // rz only: xofs[w] | xcoef[w] | yofs[h] | ycoef[h], coefficients as a0 | a1 << 16
    std::vector<int> rz_tab;
    int *d_rz_tab = nullptr;
};

// Checks the arguments of psn_lk_create_classes and lays the context out.
// Fills cfg's width, height, user_slots, nslots, nlevels, ncls and cls[] (its
// other fields stay), fcls (every field but the device pointers), slot_fcls
// ([nslots] the class of every slot; scratch slots: 0) and pyr_bytes (the
// pyramid allocation, without its read slack). PSN_LK_ERR_ARG for a bad class
// count, ring, size, scale or level cap, PSN_LK_ERR_UNSUPPORTED for a level cap
// whose pyramid tiles exceed the LDS; the outputs are then untouched.
int ctx_layout(const psn_lk_frame_class *cls, int ncls, double scale, int max_level_cap, PlanCfg &cfg,
               std::vector<FrameClass> &fcls, std::vector<int> &slot_fcls, size_t &pyr_bytes);

}  // namespace psn
