// Appearance records of include/psn_tracker2d.h: the crop rectangle
// Tracklet2D_UpdateTracklets takes of a reported box (PSNWhere_Associator3D.cpp:1130,
// :1160-1164), the normalisation of GetRGBFeature (:2542-2556) and the wire slot
// that carries the counts beside the result slot. Host arithmetic only: no
// device call, no other library.
#include <climits>
#include <cmath>
#include <cstring>

#include "psn_lk.h"
#include "psn_tracker2d.h"

namespace {

constexpr uint32_t kMagicA = 0x41325450u;  // "PT2A"
struct SlotHeaderA {
    uint32_t magic, version, cam_id, frame_idx, nobj, bytes_used;
};
struct SlotAppearance {
    uint32_t id, n_pixels;
    int32_t rect[4];
    uint32_t counts[PSN_T2D_APPEARANCE_BINS];
};
static_assert(sizeof(SlotHeaderA) == 24 && sizeof(SlotAppearance) == 216, "wire layout");

// (int)v of cv::Rect's constructor; a value beyond the int range saturates
// (the cast itself would be undefined)
long long trunc_int(double v) {
    if (v >= (double)INT_MAX) return INT_MAX;
    if (v <= (double)INT_MIN) return INT_MIN;
    return (long long)(int)v;
}

}  // namespace

extern "C" {

int psn_t2d_appearance_rect(psn_rect b, int width, int height, int rect_out[4]) {
    if (!rect_out || width <= 0 || height <= 0) return PSN_LK_ERR_ARG;
    if (std::isnan(b.x) || std::isnan(b.y) || std::isnan(b.w) || std::isnan(b.h)) return PSN_LK_ERR_ARG;
    // PSN_Rect::cropWithSize (PSNWhere_Types.h:146-153), in doubles
    const double cx = b.x > 0.0 ? b.x : 0.0, cy = b.y > 0.0 ? b.y : 0.0;
    const double cw = std::fmin((double)width - cx - 1.0, b.w), ch = std::fmin((double)height - cy - 1.0, b.h);
    // .cv(): cv::Rect((int)x, (int)y, (int)w, (int)h) (:181)
    long long x = trunc_int(cx), y = trunc_int(cy), w = trunc_int(cw), h = trunc_int(ch);
    // PSNWhere_Associator3D.cpp:1161-1164, in that order
    if (x < 0) x = 0;
    if (y < 0) y = 0;
    if (x + w > width) w = width - x;
    if (y + h > height) h = height - y;
    if (w <= 0 || h <= 0) x = y = w = h = 0;  // an empty crop
    rect_out[0] = (int)x;
    rect_out[1] = (int)y;
    rect_out[2] = (int)w;
    rect_out[3] = (int)h;
    return 0;
}

void psn_t2d_appearance_normalize(psn_t2d_appearance *a) {
    if (!a) return;
    // [OCV246] featureR / numPixels on a CV_64F Mat: convertTo with alpha = 1.0 / numPixels
    const double alpha = a->n_pixels ? 1.0 / (double)a->n_pixels : 0.0;
    for (int i = 0; i < PSN_T2D_APPEARANCE_BINS; i++) a->feature[i] = a->n_pixels ? (double)a->counts[i] * alpha : 0.0;
}

size_t psn_t2d_appearance_slot_bytes(int max_objects) {
    if (max_objects < 0) return 0;
    const size_t n = sizeof(SlotHeaderA) + (size_t)max_objects * sizeof(SlotAppearance);
    return (n + 63) & ~(size_t)63;
}

int psn_t2d_pack_appearance(unsigned cam_id, unsigned frame_idx, const psn_t2d_appearance *a, int n, void *slot,
                            size_t slot_bytes) {
    if (!slot || n < 0 || (n > 0 && !a)) return PSN_LK_ERR_ARG;
    const size_t need = sizeof(SlotHeaderA) + (size_t)n * sizeof(SlotAppearance);
    if (need > slot_bytes || need > UINT32_MAX) return PSN_T2D_ERR_CAPACITY;
    uint8_t *p = (uint8_t *)slot;
    const SlotHeaderA h{kMagicA, 1u, cam_id, frame_idx, (uint32_t)n, (uint32_t)need};
    std::memcpy(p, &h, sizeof h);
    size_t off = sizeof h;
    for (int i = 0; i < n; i++, off += sizeof(SlotAppearance)) {
        SlotAppearance s;
        s.id = a[i].id;
        s.n_pixels = a[i].n_pixels;
        for (int k = 0; k < 4; k++) s.rect[k] = a[i].rect[k];
        std::memcpy(s.counts, a[i].counts, sizeof s.counts);
        std::memcpy(p + off, &s, sizeof s);
    }
    return 0;
}

int psn_t2d_unpack_appearance(const void *slot, size_t slot_bytes, unsigned *cam_id, unsigned *frame_idx,
                              psn_t2d_appearance *out, int cap, int *n) {
    if (!slot || !n || cap < 0 || slot_bytes < sizeof(SlotHeaderA)) return PSN_LK_ERR_ARG;
    const uint8_t *p = (const uint8_t *)slot;
    SlotHeaderA h;
    std::memcpy(&h, p, sizeof h);
    if (h.magic != kMagicA || h.version != 1u || h.bytes_used > slot_bytes ||
        (size_t)h.bytes_used != sizeof h + (size_t)h.nobj * sizeof(SlotAppearance))
        return PSN_LK_ERR_ARG;
    if (h.nobj > (uint32_t)cap) return PSN_T2D_ERR_CAPACITY;  // (unsigned: a count >= 2^31 does not pass as negative)
    if (h.nobj && !out) return PSN_LK_ERR_ARG;
    size_t off = sizeof h;
    for (uint32_t i = 0; i < h.nobj; i++, off += sizeof(SlotAppearance)) {
        SlotAppearance s;
        std::memcpy(&s, p + off, sizeof s);
        psn_t2d_appearance &a = out[i];
        a.id = s.id;
        a.n_pixels = s.n_pixels;
        for (int k = 0; k < 4; k++) a.rect[k] = s.rect[k];
        std::memcpy(a.counts, s.counts, sizeof s.counts);
        psn_t2d_appearance_normalize(&a);
    }
    if (cam_id) *cam_id = h.cam_id;
    if (frame_idx) *frame_idx = h.frame_idx;
    *n = (int)h.nobj;
    return 0;
}

}  // extern "C"
