// The context layout (psn_lk_layout.h) and the pure size and table functions of
// include/psn_lk.h it is made of.
#include "psn_lk_layout.h"

#include <algorithm>
#include <cmath>
#include <utility>

static int cv_round(float v) { return (int)lrint((double)v); }  // cvRound: to nearest, ties to even

extern "C" {

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

}  // extern "C"

namespace psn {

int ctx_layout(const psn_lk_frame_class *cls, int ncls, double scale, int max_level_cap, PlanCfg &cfg,
               std::vector<FrameClass> &fcls, std::vector<int> &slot_fcls, size_t &pyr_bytes) {
    if (!cls || ncls < 1 || ncls > PSN_LK_MAX_FRAME_CLASSES || max_level_cap < 0 || max_level_cap > kPyrMaxTop)
        return PSN_LK_ERR_ARG;
    std::vector<FrameClass> fc((size_t)ncls);
    int user_slots = 0;
    for (int k = 0; k < ncls; k++) {
        FrameClass &f = fc[(size_t)k];
        if (cls[k].ring_slots <= 0 || user_slots > INT32_MAX / 2 - cls[k].ring_slots) return PSN_LK_ERR_ARG;
        if (psn_lk_scaled_size(cls[k].width, cls[k].height, scale, &f.w, &f.h)) return PSN_LK_ERR_ARG;
        f.src_w = cls[k].width;
        f.src_h = cls[k].height;
        f.rz = f.src_w != f.w || f.src_h != f.h;
        f.first_slot = user_slots;
        f.nslots = cls[k].ring_slots;
        user_slots += f.nslots;
    }
    // the pyramid tiles' LDS plan (guarded at build time for every top level:
    // pyr_tiles_fit; kept here so a context never launches past the CU's LDS)
    if (kStScratchBytes + pyr_lds_bytes(max_level_cap, pyr_tile_edge(max_level_cap)) > kMaxLdsBytes)
        return PSN_LK_ERR_UNSUPPORTED;
    const int nslots = user_slots + 2, nlevels = max_level_cap + 1;
    std::vector<int> sf((size_t)nslots, 0);
    for (int k = 0; k < ncls; k++) {
        FrameClass &f = fc[(size_t)k];
        std::fill_n(sf.begin() + f.first_slot, f.nslots, k);
        // slot layout: levels back to back, rows padded to 256 B (one HBM burst / 4 x 64-B lines)
        size_t slot_bytes = 0;
        for (int l = 0, w = f.w, h = f.h; l < nlevels; l++, w = (w + 1) / 2, h = (h + 1) / 2) {
            f.ring.w[l] = w;
            f.ring.h[l] = h;
            f.ring.pitch[l] = (w + 255) & ~255;
            f.ring.off[l] = (long long)slot_bytes;
            slot_bytes += (size_t)f.ring.pitch[l] * h;
        }
        f.ring.slot_bytes = (long long)((slot_bytes + 4095) & ~(size_t)4095);
        if (!f.rz) continue;
        // the resize tables, and one gray plane per slot on the ring's 256-B pitch
        std::vector<int> ofs((size_t)std::max(f.w, f.h));
        std::vector<int16_t> coef(2 * ofs.size());
        f.rz_tab.resize(2 * ((size_t)f.w + f.h));
        for (int ax = 0; ax < 2; ax++) {
            const int n = ax == 0 ? f.w : f.h;
            int *t = f.rz_tab.data() + (ax == 0 ? 0 : 2 * (size_t)f.w);
            if (psn_lk_resize_plan(ax == 0 ? f.src_w : f.src_h, n, ofs.data(), coef.data(), ax == 0)) return PSN_LK_ERR_ARG;
            for (int i = 0; i < n; i++) {
                t[i] = ofs[i];
                t[n + i] = (int)((uint32_t)(uint16_t)coef[2 * i] | ((uint32_t)(uint16_t)coef[2 * i + 1] << 16));
            }
        }
        f.gray_pitch = (f.w + 255) & ~255;
        f.gray_bytes = (size_t)f.gray_pitch * f.h * (f.nslots + (k == 0 ? 2 : 0));
    }
    // Places in the pyramid allocation. A kernel finds a slot at base + slot *
    // slot_bytes of its class, and class 0 owns the user slots [0, n0) and the
    // scratch slots [user_slots, user_slots + 2): its stride spans all nslots slot
    // numbers, and the other classes' slots lie in the gap between its user and its
    // scratch slots where they fit (always, when no class is larger than class 0),
    // else behind the scratch slots. One class: the nslots slots back to back.
    const size_t sb0 = (size_t)fc[0].ring.slot_bytes;
    size_t gap = sb0 * fc[0].nslots, end = sb0 * nslots;
    const size_t gap_end = sb0 * user_slots;
    for (int k = 1; k < ncls; k++) {
        const size_t need = (size_t)fc[(size_t)k].ring.slot_bytes * fc[(size_t)k].nslots;
        size_t &at = gap + need <= gap_end ? gap : end;
        fc[(size_t)k].place = at;
        at += need;
    }
    cfg.width = fc[0].w;
    cfg.height = fc[0].h;
    cfg.user_slots = user_slots;
    cfg.nslots = nslots;
    cfg.nlevels = nlevels;
    cfg.ncls = ncls > 1 ? ncls : 0;  // (one class: the planner's width x height over every slot)
    for (int k = 0; k < cfg.ncls; k++) cfg.cls[k] = PlanFrameClass{fc[(size_t)k].w, fc[(size_t)k].h, fc[(size_t)k].first_slot, fc[(size_t)k].nslots};
    fcls = std::move(fc);
    slot_fcls = std::move(sf);
    pyr_bytes = end;
    return PSN_LK_OK;
}

}  // namespace psn
