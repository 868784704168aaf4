// Gray resize of the ingest path at a reduced optical-flow scale (kernel in
// psn_resize.hip; the tables, psn_lk_resize_plan of include/psn_lk.h, in
// psn_lk_layout.cpp; psn_lk_create_scaled in psn_lk_context.cpp).
//
// cvtColor(BGR2GRAY) then cv::resize(gray, ring[slot], Size(w * s, h * s)) of
// PSNWhere_Tracker2D.cpp:257-262: OpenCV 2.4.6 resize(INTER_LINEAR) for CV_8UC1
// [OCV246 imgproc/src/imgwarp.cpp: resizeGeneric_, HResizeLinear<uchar, int,
// short, 2048>, VResizeLinear with FixedPtCast<int, uchar, 22>], restated:
//   D(r, dx) = S[r][xofs[dx]] * a0[dx] + S[r][min(xofs[dx] + 1, sw - 1)] * a1[dx]
//   out(dy, dx) = (((b0[dy] * (D(r0, dx) >> 4)) >> 16) + ((b1[dy] * (D(r1, dx) >> 4)) >> 16) + 2) >> 2
//   r0 = clamp(yofs[dy], 0, sh - 1), r1 = clamp(yofs[dy] + 1, 0, sh - 1)
// with the offset and coefficient tables computed on the host
// (psn_lk_resize_plan). Integer work from the tables on: exact.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace psn {

constexpr int kRzThreads = 256;
constexpr int kRzTW = 64, kRzTH = 16;  // output tile: a thread writes 4 pixels of one row as a dword
static_assert(kRzTW / 4 * kRzTH == kRzThreads, "resize tile: one output dword per thread");
// LDS rows of the staged source: the two source rows of each output row of the
// tile, kRzRowDw aligned dwords each (32 KB: five workgroups per CU). A tile
// whose source columns need more (a scale below about 0.19 for BGR, 0.06 for
// gray) reads its pixels from the frame instead.
constexpr int kRzRows = 2 * kRzTH;
constexpr int kRzRowDw = 256;

struct ResizeArgs {
    const uint8_t *src;  // gray or BGR frame, any alignment
    int src_stride, channels;
    int sw, sh;          // source size
    uint8_t *dst;        // gray plane, dword-aligned rows (pitch % 4 == 0, pitch >= (dw + 3) & ~3)
    int dst_pitch;
    int dw, dh;          // output size
    // device tables: xofs[dw] (border rule applied, 0 <= xofs < sw), yofs[dh]
    // (not clamped), coefficients as a0 | a1 << 16
    const int *xofs, *yofs;
    const uint32_t *xcoef, *ycoef;
};

hipError_t launch_resize_gray(const ResizeArgs &a, hipStream_t s);

}  // namespace psn
