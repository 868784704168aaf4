// RGB box histograms of Associator3D's appearance feature (kernel in
// psn_rgbhist.hip; the C ABI, psn_rgbhist_device / psn_lk_box_histograms of
// include/psn_lk.h, in psn_lk_readers.cpp).
//
// GetRGBFeature (psn_where/PSNWhere_Associator3D.cpp:2542-2556) over
// psn::histogram (psn_where/PSNWhere_Utils.cpp:445-460): 16 bins of 16 grey
// values per channel, counted over the w x h pixels of a crop of the BGR
// frame, output R[16], G[16], B[16].
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "psn_lk.h"

namespace psn {

constexpr int kRhBins = 3 * PSN_RGBHIST_BINS;  // counters per rect, R G B
constexpr int kRhThreads = 256;                // workgroup: 4 waves
constexpr int kRhWaves = kRhThreads / 64;
// Sub-histograms per wave: lane l adds into replica l & 31, and replica r of
// every bin lies in LDS bank r (a dword LDS operation is served in two groups
// of 32 lanes over 32 banks), so no two lanes of a group ever meet in a bank,
// whatever the pixels are (a constant-colour patch included).
constexpr int kRhReps = 32;
constexpr int kRhLdsWords = kRhWaves * kRhBins * kRhReps;  // 24 KB
// A workgroup takes a band of rows of about this many frame bytes: a 64 x 160
// box (30 KB) is one workgroup, a 1080p frame 216, a 4K frame 1080 bands.
constexpr int kRhBandBytes = 32 * 1024;
constexpr int kRhMaxGridY = 256;  // bands beyond gridDim.y are looped over

inline int rgbhist_band_rows(int w) { return w > 0 && 3LL * w < kRhBandBytes ? kRhBandBytes / (3 * w) : 1; }
inline int rgbhist_bands(int w, int h) {
    if (w <= 0 || h <= 0) return 0;
    const int rows = rgbhist_band_rows(w);
    return (h + rows - 1) / rows;
}

// Zeroes d_counts[nrect][kRhBins] and counts every rect, all on stream s.
// grid_y = workgroups per rect (each loops over the bands b, b + grid_y, ...);
// <= 0: chosen from nrect alone (the rects are device data).
hipError_t launch_rgbhist(const psn_rgbhist_rect *d_rects, int nrect, uint32_t *d_counts, int grid_y, hipStream_t s);

}  // namespace psn
