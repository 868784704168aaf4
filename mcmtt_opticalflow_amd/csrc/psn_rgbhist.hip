// RGB box histograms on the device (psn_rgbhist.h): the crop + cv::split +
// psn::histogram of GetRGBFeature (PSNWhere_Associator3D.cpp:2542-2556,
// PSNWhere_Utils.cpp:445-460) for any number of rects on any number of BGR
// frames in one launch. Exact integer work: bin = value >> 4 (floor(v / 16.0)).
//
// Grid: x = rect, y = workgroups of the rect; a workgroup takes the row bands
// y, y + gridDim.y, ... of its rect (a band = about kRhBandBytes of rows).
// Reads: a row's bytes [3x, 3(x + w)) start at any alignment (3x, and a stride
// that is no multiple of 4), so the row is read as the naturally aligned dwords
// that hold at least one of its bytes; bytes outside the span are masked. Such
// a dword shares an aligned 4 bytes, hence a page, with a valid byte. The
// channel of a byte is its offset in the row mod 3 (B, G, R).
// Counting: each wave adds into its own kRhReps sub-histograms in LDS (32-bit
// counters, replica = lane & 31 = the LDS bank, conflict-free for any data), the
// workgroup sums them in LDS and adds its non-zero bins to the zeroed output
// with one global atomic each. Integer adds commute: the result is deterministic.
#include "psn_rgbhist.h"

namespace psn {

__global__ __launch_bounds__(kRhThreads) void rgbhist_kernel(const psn_rgbhist_rect *__restrict__ rects,
                                                             uint32_t *__restrict__ counts) {
    __shared__ uint32_t hist[kRhLdsWords];
    const psn_rgbhist_rect R = rects[blockIdx.x];
    if (R.w <= 0 || R.h <= 0) return;  // an empty crop: its counts stay 0
    const unsigned span = 3u * (unsigned)R.w;  // bytes of one row of the rect
    const unsigned rows = span < (unsigned)kRhBandBytes ? (unsigned)kRhBandBytes / span : 1u;
    const unsigned nbands = ((unsigned)R.h + rows - 1) / rows;
    if (blockIdx.y >= nbands) return;
    const unsigned tid = threadIdx.x;
    for (unsigned i = tid; i < (unsigned)kRhLdsWords; i += kRhThreads) hist[i] = 0;
    __syncthreads();
    uint32_t *my = hist + (tid >> 6) * (kRhBins * kRhReps) + (tid & (kRhReps - 1));
    // dwords that can hold bytes of one row: its first byte lies at offset o <= 3 of the first
    const unsigned D = (span + 3 + 3) / 4;
    const unsigned step_r = kRhThreads / D, step_d = kRhThreads % D;
    constexpr int U = 4;  // loads in flight per thread
    for (unsigned band = blockIdx.y; band < nbands; band += gridDim.y) {
        const unsigned r0 = band * rows;
        const unsigned nr = min(rows, (unsigned)R.h - r0);
        const unsigned total = nr * D;  // (row, dword) items of the band
        const uint8_t *base = R.frame + ((size_t)R.y + r0) * (size_t)R.stride + 3 * (size_t)R.x;
        unsigned r = tid / D, d = tid % D;
        for (unsigned i = tid; i < total; i += U * kRhThreads) {
            uint32_t v[U];
            unsigned p0[U], ch[U];  // span position of the dword's byte 0 (wraps below 0), its channel
#pragma unroll
            for (int u = 0; u < U; u++) {
                v[u] = 0;
                p0[u] = span;  // nothing valid
                ch[u] = 0;
                if (i + u * kRhThreads < total) {
                    const uint8_t *rowp = base + (size_t)r * (size_t)R.stride;
                    const unsigned o = (unsigned)((uintptr_t)rowp & 3);
                    if (4 * d < o + span) {  // the dword holds a byte of the span
                        v[u] = *(const uint32_t *)(rowp - o + 4 * (size_t)d);
                        p0[u] = 4 * d - o;
                        ch[u] = (d + 6 - o) % 3;  // (4d - o) mod 3
                    }
                }
                r += step_r;
                d += step_d;
                if (d >= D) d -= D, r++;
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                unsigned c = ch[u];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (p0[u] + k < span) {  // (a position below 0 wrapped to a huge one)
                        const unsigned bin = (v[u] >> (8 * k + 4)) & 15u;
                        atomicAdd(&my[((2 - c) * PSN_RGBHIST_BINS + bin) * kRhReps], 1u);  // B G R -> R G B
                    }
                    c = c == 2 ? 0 : c + 1;
                }
            }
        }
    }
    __syncthreads();
    // waves -> wave 0's sub-histograms, then the replicas of each bin
    for (unsigned i = tid; i < (unsigned)(kRhBins * kRhReps); i += kRhThreads) {
        uint32_t s = hist[i];
#pragma unroll
        for (int w = 1; w < kRhWaves; w++) s += hist[w * (kRhBins * kRhReps) + i];
        hist[i] = s;
    }
    __syncthreads();
    if (tid < (unsigned)kRhBins) {
        uint32_t s = 0;
        for (unsigned j = 0; j < (unsigned)kRhReps; j++) s += hist[tid * kRhReps + ((tid + j) & (kRhReps - 1))];
        if (s) atomicAdd(&counts[(size_t)blockIdx.x * kRhBins + tid], s);
    }
}

hipError_t launch_rgbhist(const psn_rgbhist_rect *d_rects, int nrect, uint32_t *d_counts, int grid_y, hipStream_t s) {
    if (nrect <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(d_counts, 0, (size_t)nrect * kRhBins * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    // the rects are device data: without a hint, about 2048 workgroups in all
    // (those beyond a rect's bands leave at once)
    if (grid_y <= 0) grid_y = 2048 / nrect;
    grid_y = grid_y < 1 ? 1 : (grid_y > kRhMaxGridY ? kRhMaxGridY : grid_y);
    rgbhist_kernel<<<dim3((unsigned)nrect, (unsigned)grid_y), kRhThreads, 0, s>>>(d_rects, d_counts);
    return hipGetLastError();
}

}  // namespace psn
