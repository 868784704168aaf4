// Device code of one pyramid tile, shared by pyramid_kernel (psn_lk_kernels.hip)
// and the fused build behind the single-tile LK kernel (pyr_tail, psn_lk_st.hip).
// (the LDS plan of a tile, pyr_lds_bytes, and its build-time guards: psn_lk_kernels.h)
// Internal.
#pragma once

#include "psn_lk_device.h"

namespace psn {

__device__ __forceinline__ uint8_t load_src(const PyrBuildArgs &a, int y, int x) {
    const uint8_t *row = a.src + (size_t)y * a.src_stride;
    if (a.channels == 1) return row[x];
    const uint8_t *p = row + 3 * x;  // BGR: RGB2Gray<uchar> with B2Y=1868, G2Y=9617, R2Y=4899
    return (uint8_t)((p[0] * 1868 + p[1] * 9617 + p[2] * 4899 + (1 << 13)) >> 14);
}

// One top-level tile (bx, by) of a multi-level build (top >= 1) by NT threads
// laid out 16 wide (no index divisions). The tile recomputes its halo through
// the levels in LDS: level-0 region (dword loads for interior gray tiles,
// reflect-101 byte gathers otherwise), then per level a horizontal [1 4 6 4 1]
// pass into int16 and a vertical pass with (sum + 128) >> 8; region positions
// outside a level take their reflect-101 source. Each level's own tile goes
// out as dword stores. Called by pyramid_kernel and, for a deferred build
// fused into an LK launch, by the LK launch's workgroups (pyr_tail).
template <int NT>
__device__ __forceinline__ void pyr_tile(const PyrBuildArgs &a, int bx, int by, uint8_t *smem) {
    constexpr int TX = 16, TY = NT / 16;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x / TX;
    const int top = a.nlevels - 1;
    const int W0 = a.lv[0].w, H0 = a.lv[0].h;
    const int T = a.tile;
    const int topx = bx * T, topy = by * T;
    const int n0 = pyr_region_n(top, 0, T);
    const int span = 1 << top;
    const int s0x = span * topx - 2 * (span - 1), s0y = span * topy - 2 * (span - 1);
    const int ax = s0x & ~3, off0 = s0x - ax, S0 = pyr_s0(n0);
    uint8_t *B0 = smem;
    int16_t *Ht = (int16_t *)(smem + pyr_lds_off(top, top, T));

    // level-0 region
    {
        const int m = (off0 + n0 + 3) >> 2;  // dwords per row
        const bool dw = s0x >= 0 && s0y >= 0 && ax + 4 * m <= W0 && s0y + n0 <= H0 &&
                        ((uintptr_t)a.src & 3) == 0 && (a.src_stride & 3) == 0;
        if (dw && a.channels == 1) {
            for (int r = ty; r < n0; r += TY) {
                const uint32_t *srow = (const uint32_t *)(a.src + (size_t)(s0y + r) * a.src_stride + ax);
                for (int d = tx; d < m; d += TX) *(uint32_t *)(B0 + r * S0 + 4 * d) = srow[d];
            }
        } else if (dw) {
            // BGR interior region: 4 pixels = 3 aligned dwords -> RGB2Gray<uchar> -> one dword
            for (int r = ty; r < n0; r += TY) {
                const uint32_t *srow = (const uint32_t *)(a.src + (size_t)(s0y + r) * a.src_stride + 3 * ax);
                for (int d = tx; d < m; d += TX) {
                    const uint32_t w0 = srow[3 * d], w1 = srow[3 * d + 1], w2 = srow[3 * d + 2];
                    const uint32_t bgr[12] = {w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255, w0 >> 24,
                                              w1 & 255, (w1 >> 8) & 255, (w1 >> 16) & 255, w1 >> 24,
                                              w2 & 255, (w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24};
                    uint32_t out = 0;
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        out |= ((bgr[3 * k] * 1868 + bgr[3 * k + 1] * 9617 + bgr[3 * k + 2] * 4899 + (1 << 13)) >> 14)
                               << (8 * k);
                    *(uint32_t *)(B0 + r * S0 + 4 * d) = out;
                }
            }
        } else {
            for (int r = ty; r < n0; r += TY) {
                const int gy = refl101(s0y + r, H0);
                for (int c = tx; c < n0; c += TX) B0[r * S0 + off0 + c] = load_src(a, gy, refl101(s0x + c, W0));
            }
        }
    }
    __syncthreads();
    // own level-0 tile
    {
        const int own = span * T, d0 = 2 * (span - 1);
        const int ox = topx * span, oy = topy * span;
        uint8_t *dst = a.lv[0].p;
        const int pitch = a.lv[0].pitch;
        for (int r = ty; r < own && oy + r < H0; r += TY) {
            const uint8_t *srow = B0 + (r + d0) * S0 + off0 + d0;
            uint8_t *drow = dst + (size_t)(oy + r) * pitch + ox;
            for (int q = tx; q < own / 4; q += TX) {
                const uint8_t *sp4 = srow + 4 * q;
                if (ox + 4 * q + 4 <= W0) {
                    *(uint32_t *)(drow + 4 * q) =
                        sp4[0] | ((uint32_t)sp4[1] << 8) | ((uint32_t)sp4[2] << 16) | ((uint32_t)sp4[3] << 24);
                } else {
                    for (int b = 0; b < 4; b++)
                        if (ox + 4 * q + b < W0) drow[4 * q + b] = sp4[b];
                }
            }
        }
    }

    for (int l = 1; l <= top; l++) {
        const int sp = 1 << (top - l);
        const int nl = (l == top) ? T : pyr_region_n(top, l, T);
        const int np = pyr_region_n(top, l - 1, T);
        const int slx = sp * topx - 2 * (sp - 1), sly = sp * topy - 2 * (sp - 1);
        const int Wl = a.lv[l].w, Hl = a.lv[l].h;
        const uint8_t *Bp = l == 1 ? B0 + off0 : smem + pyr_lds_off(top, l - 1, T);
        const int Sp = l == 1 ? S0 : np;
        // horizontal [1 4 6 4 1] over the previous region (rows np, cols nl)
        for (int r = ty; r < np; r += TY)
            for (int c = tx; c < nl; c += TX) {
                const uint8_t *q = Bp + r * Sp + 2 * c;
                Ht[r * nl + c] = (int16_t)(q[0] + q[4] + 4 * (q[1] + q[3]) + 6 * q[2]);
            }
        __syncthreads();
        if (l < top) {
            uint8_t *Bl = smem + pyr_lds_off(top, l, T);
            for (int r = ty; r < nl; r += TY)
                for (int c = tx; c < nl; c += TX) {
                    const int gy = sly + r, gx = slx + c;
                    if ((unsigned)gy < (unsigned)Hl && (unsigned)gx < (unsigned)Wl) {
                        const int16_t *cc = Ht + 2 * r * nl + c;
                        const int v = cc[0] + cc[4 * nl] + 4 * (cc[nl] + cc[3 * nl]) + 6 * cc[2 * nl];
                        Bl[r * nl + c] = (uint8_t)((v + 128) >> 8);
                    }
                }
            __syncthreads();
            const bool border = slx < 0 || sly < 0 || slx + nl > Wl || sly + nl > Hl;
            if (border) {  // positions outside the level: copy their reflect-101 source
                for (int r = ty; r < nl; r += TY)
                    for (int c = tx; c < nl; c += TX) {
                        const int gy = sly + r, gx = slx + c;
                        if ((unsigned)gy >= (unsigned)Hl || (unsigned)gx >= (unsigned)Wl) {
                            const int ry = refl101(gy, Hl) - sly, rx = refl101(gx, Wl) - slx;
                            Bl[r * nl + c] = Bl[ry * nl + rx];
                        }
                    }
                __syncthreads();
            }
            const int own = sp * T, d = 2 * (sp - 1);
            const int ox = topx * sp, oy = topy * sp;
            uint8_t *dst = a.lv[l].p;
            const int pitch = a.lv[l].pitch;
            for (int r = ty; r < own && oy + r < Hl; r += TY) {
                const uint8_t *srow = Bl + (r + d) * nl + d;
                uint8_t *drow = dst + (size_t)(oy + r) * pitch + ox;
                for (int q = tx; q < own / 4; q += TX) {
                    const uint8_t *sp4 = srow + 4 * q;
                    if (ox + 4 * q + 4 <= Wl) {
                        *(uint32_t *)(drow + 4 * q) =
                            sp4[0] | ((uint32_t)sp4[1] << 8) | ((uint32_t)sp4[2] << 16) | ((uint32_t)sp4[3] << 24);
                    } else {
                        for (int b = 0; b < 4; b++)
                            if (ox + 4 * q + b < Wl) drow[4 * q + b] = sp4[b];
                    }
                }
            }
        } else {
            uint8_t *dst = a.lv[l].p;
            const int pitch = a.lv[l].pitch;
            for (int r = ty; r < T; r += TY)
                for (int c = tx; c < T; c += TX) {
                    const int gy = topy + r, gx = topx + c;
                    if (gy < Hl && gx < Wl) {
                        const int16_t *cc = Ht + 2 * r * nl + c;
                        const int v = cc[0] + cc[4 * nl] + 4 * (cc[nl] + cc[3 * nl]) + 6 * cc[2 * nl];
                        dst[(size_t)gy * pitch + gx] = (uint8_t)((v + 128) >> 8);
                    }
                }
        }
        __syncthreads();
    }
}

}  // namespace psn
