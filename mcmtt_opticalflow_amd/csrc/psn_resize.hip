// resize_gray_kernel (psn_resize.h): BGR2GRAY + resize(INTER_LINEAR) of one
// source frame into the slot's gray plane, one launch per pushed frame.
//
// Grid: one workgroup per kRzTW x kRzTH output tile. The tile needs at most two
// source rows per output row (kRzRows row slots: slot 2i + k = source row
// clamp(yofs[y0 + i] + k)) and the source columns xofs[first] .. xofs[last] + 1.
// Staging: each row slot's bytes are copied into LDS as the naturally aligned
// dwords that hold at least one of them (any frame pointer, any stride: the
// alignment offset o is per row; such a dword shares an aligned 4 bytes, hence
// a page, with a valid byte), so a source byte is fetched from memory once per
// tile and as part of a coalesced dword row. The gray conversion and both
// passes then read bytes from LDS. A tile whose column span does not fit the LDS
// rows reads the frame's bytes directly (the same arithmetic, byte loads).
// Each thread forms 4 output pixels and stores them as one dword (the plane's
// row padding past dw takes zeros).
#include "psn_resize.h"

namespace psn {

// Gray value of the pixel whose first byte is row[i]: the byte itself, or
// RGB2Gray<uchar> of B, G, R (the pyramid build's constants: B2Y=1868,
// G2Y=9617, R2Y=4899, 14 bits).
template <int CH>
__device__ __forceinline__ int rz_gray(const uint8_t *row, int i) {
    if (CH == 1) return row[i];
    return (row[i] * 1868 + row[i + 1] * 9617 + row[i + 2] * 4899 + (1 << 13)) >> 14;
}

// One output pixel from its two source rows; i0 / i1 = byte index in the rows
// of the left / right source pixel.
template <int CH>
__device__ __forceinline__ uint32_t rz_pixel(const uint8_t *r0, const uint8_t *r1, int i0, int i1, uint32_t ac,
                                             uint32_t bc) {
    const int a0 = (int)(ac & 0xffffu), a1 = (int)(ac >> 16);
    const int b0 = (int)(bc & 0xffffu), b1 = (int)(bc >> 16);
    const int d0 = rz_gray<CH>(r0, i0) * a0 + rz_gray<CH>(r0, i1) * a1;
    const int d1 = rz_gray<CH>(r1, i0) * a0 + rz_gray<CH>(r1, i1) * a1;
    return (uint32_t)((((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2) & 255u;
}

template <int CH>
__global__ __launch_bounds__(kRzThreads) void resize_gray_kernel(const ResizeArgs a) {
    __shared__ uint32_t raw[kRzRows * kRzRowDw];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kRzTW, y0 = blockIdx.y * kRzTH;
    const int xl = min(x0 + kRzTW, a.dw) - 1;  // the tile's last output column
    // source columns of the tile (xofs is non-decreasing)
    const int c0 = a.xofs[x0];
    const int c1 = min(a.xofs[xl] + 1, a.sw - 1);
    const int nb = (c1 - c0 + 1) * CH;  // bytes per row slot
    const bool staged = nb + 3 <= 4 * kRzRowDw;  // + o <= 3: (o + nb + 3) / 4 dwords
    if (staged) {
        // wave w copies the row slots w, w + 4, ...: a slot is consecutive dwords
        for (int j = tid >> 6; j < kRzRows; j += kRzThreads / 64) {
            const int y = y0 + (j >> 1);
            if (y >= a.dh) break;
            const int sr = min(max(a.yofs[y] + (j & 1), 0), a.sh - 1);
            const uint8_t *rp = a.src + (size_t)sr * (size_t)a.src_stride + (size_t)c0 * CH;
            const int o = (int)((uintptr_t)rp & 3);
            const int nd = (o + nb + 3) >> 2;
            const uint32_t *ap = (const uint32_t *)(rp - o);
            for (int d = tid & 63; d < nd; d += 64) raw[j * kRzRowDw + d] = ap[d];
        }
    }
    __syncthreads();
    const int ty = tid >> 4, x = x0 + 4 * (tid & 15), y = y0 + ty;
    if (y >= a.dh || x >= a.dw) return;
    const int sy = a.yofs[y];
    const int sr0 = min(max(sy, 0), a.sh - 1), sr1 = min(max(sy + 1, 0), a.sh - 1);
    const uint32_t bc = a.ycoef[y];
    const uint8_t *g0 = a.src + (size_t)sr0 * (size_t)a.src_stride;
    const uint8_t *g1 = a.src + (size_t)sr1 * (size_t)a.src_stride;
    // staged rows: source column c is at byte o + (c - c0) * CH of its row slot
    const uint8_t *l0 = (const uint8_t *)(raw + (2 * ty) * kRzRowDw);
    const uint8_t *l1 = (const uint8_t *)(raw + (2 * ty + 1) * kRzRowDw);
    const int o0 = (int)((uintptr_t)(g0 + (size_t)c0 * CH) & 3), o1 = (int)((uintptr_t)(g1 + (size_t)c0 * CH) & 3);
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (x + k < a.dw) {
            const int sx = a.xofs[x + k], sx1 = min(sx + 1, a.sw - 1);
            const uint32_t ac = a.xcoef[x + k];
            uint32_t v;
            if (staged)
                v = rz_pixel<CH>(l0 + o0, l1 + o1, (sx - c0) * CH, (sx1 - c0) * CH, ac, bc);
            else
                v = rz_pixel<CH>(g0, g1, sx * CH, sx1 * CH, ac, bc);
            out |= v << (8 * k);
        }
    }
    *(uint32_t *)(a.dst + (size_t)y * (size_t)a.dst_pitch + x) = out;
}

hipError_t launch_resize_gray(const ResizeArgs &a, hipStream_t s) {
    if (a.dw <= 0 || a.dh <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.dw + kRzTW - 1) / kRzTW), (unsigned)((a.dh + kRzTH - 1) / kRzTH));
    if (a.channels == 3)
        resize_gray_kernel<3><<<grid, kRzThreads, 0, s>>>(a);
    else
        resize_gray_kernel<1><<<grid, kRzThreads, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace psn
