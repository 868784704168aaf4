// The single-tile LK kernel of libpsn_lk.so (gfx950): lk_kernel_st with its
// private helpers, its instantiation list PSN_ST_KERNELS, launch_lk_st and
// st_kernels_init.
//
// The whole window (I, Ix, Iy in registers, product planes in LDS)
// is LDS-resident. Per iteration: ONE fused pass computes the J bilinear
// window, the b-products (written chain-major into a double-buffered plane)
// and their integer sums; one barrier exchanges the per-wave DPP sums; if the
// exact-integer condition fails, EVERY wave sums the 10 float chains itself
// (lanes 0-9, software-pipelined 16-float LDS reads) and reads the results
// with readlane, so no second barrier is needed. Double buffering of the
// planes and of the reduce scratch keeps one barrier per iteration race-free:
// a wave can be at most one iteration ahead of the slowest one.
#include "psn_lk_bx.h"  // the packed 16-bit dots: sdot2, pack_w, s16x2
#include "psn_lk_pyr.h"

namespace psn {

// Diagnostic build (-DPSN_LK_STAMPS, psn_lk_stamps.h): thread 0's shader clock at
// workgroup phase `slot` (or a value) into stamps[workgroup][slot].
#define LK_STAMP(slot) PSN_STAMP(A.stamps, threadIdx.x == 0, (size_t)blockIdx.x * 64 + (slot))
#define LK_COUNT(slot, v) PSN_STAMP_VAL(A.stamps, threadIdx.x == 0, (size_t)blockIdx.x * 64 + (slot), v)

__device__ __forceinline__ float add16(float acc, const float4 &a, const float4 &b, const float4 &c, const float4 &d) {
    acc = acc + a.x; acc = acc + a.y; acc = acc + a.z; acc = acc + a.w;
    acc = acc + b.x; acc = acc + b.y; acc = acc + b.z; acc = acc + b.w;
    acc = acc + c.x; acc = acc + c.y; acc = acc + c.z; acc = acc + c.w;
    acc = acc + d.x; acc = acc + d.y; acc = acc + d.z; acc = acc + d.w;
    return acc;
}

// Ordered float sum of nb*16 LDS floats (zero padding is exact: the running
// sum of integer-valued floats starting at +0 is never -0).
__device__ __forceinline__ float chain_sum16(const float *p, int nb) {
    float acc = 0.f;
    if (nb <= 0) return acc;
    const float4 *q = (const float4 *)p;
    float4 a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3];
    for (int b = 1; b < nb; b++) {
        const float4 c0 = q[4 * b], c1 = q[4 * b + 1], c2 = q[4 * b + 2], c3 = q[4 * b + 3];
        acc = add16(acc, a0, a1, a2, a3);
        a0 = c0;
        a1 = c1;
        a2 = c2;
        a3 = c3;
    }
    return add16(acc, a0, a1, a2, a3);
}

// Chain-major geometry of a w x h window, regions padded to 16 floats.
struct ChainGeo {
    int nL, tL;      // per-row terms in each SSE2 lane chain / in the tail chain
    int S, T, P;     // lane-region stride, tail-region stride, plane size (floats)
    int lenL, lenT;  // chain lengths
};
__device__ __forceinline__ ChainGeo chain_geo_A(int w, int h, bool sse) {
    ChainGeo g;
    const int nA = sse ? w / 4 : 0;
    g.nL = nA;
    g.tL = w - 4 * nA;
    g.lenL = h * nA;
    g.lenT = h * g.tL;
    g.S = round16i(g.lenL);
    g.T = round16i(g.lenT + 1);
    g.P = lk_st_planeA(w, h, sse);
    return g;
}
__device__ __forceinline__ ChainGeo chain_geo_B(int w, int h, bool sse) {
    ChainGeo g;
    const int nB = sse ? w / 8 : 0;
    g.nL = 2 * nB;
    g.tL = w - 8 * nB;
    g.lenL = h * 2 * nB;
    g.lenT = h * g.tL;
    g.S = round16i(g.lenL);
    g.T = round16i(g.lenT + 1);
    g.P = lk_st_planeB(w, h, sse);
    return g;
}
__device__ __forceinline__ int posA(const ChainGeo &g, int y, int x) {
    const int nA = g.nL;
    return x < 4 * nA ? (x & 3) * g.S + y * nA + (x >> 2) : 4 * g.S + y * g.tL + (x - 4 * nA);
}
__device__ __forceinline__ int posB(const ChainGeo &g, int y, int x) {
    const int n8 = 4 * g.nL;  // 8*nB
    return x < n8 ? (x & 3) * g.S + y * g.nL + 2 * (x >> 3) + ((x >> 2) & 1) : 4 * g.S + y * g.tL + (x - n8);
}
// Zero the padding slots of `np` planes (never product positions).
template <int NT>
__device__ __forceinline__ void zero_pads(float *plane0, const ChainGeo &g, int np) {
    for (int k = threadIdx.x; k < np * 80; k += NT) {
        const int pl = k / 80, c = (k >> 4) % 5, o = k & 15;
        const int len = c < 4 ? g.lenL : g.lenT;
        const int stride = c < 4 ? g.S : g.T;
        if (o < stride - len) plane0[pl * g.P + c * g.S + len + o] = 0.f;
    }
}

// Workgroup sums of (s1 wrapping, s2 wrapping, a saturating): DPP within each
// wave, then the waves' totals through LDS scratch `ri` and ONE barrier (the
// caller's phase barrier). Results are uniform.
template <int NT>
__device__ __forceinline__ void block_sums3(int &s1, int &s2, unsigned &a, int *ri) {
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    a = wave_sum_sat(a);
    if constexpr (NT > 64) {
        const int wid = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
            ri[4 * wid + 0] = s1;
            ri[4 * wid + 1] = s2;
            ri[4 * wid + 2] = (int)a;
        }
        __syncthreads();
        int t1 = 0, t2 = 0;
        unsigned ta = 0;
#pragma unroll
        for (int k = 0; k < NT / 64; k++) {
            t1 += ri[4 * k];
            t2 += ri[4 * k + 1];
            ta = sat_add(ta, (unsigned)ri[4 * k + 2]);
        }
        s1 = t1;
        s2 = t2;
        a = ta;
    } else {
        __syncthreads();  // single wave: orders this phase's LDS writes before the next phase's reads
    }
}

// Element walk of a region with m elements per row: this thread's first
// element (row, column) and the per-NT step (computed once per kernel).
struct JWalk {
    int ey0, ex0, sy, sx, m;
};
__device__ __forceinline__ JWalk jwalk_t(int t, int m, int nt, unsigned mg) {
    JWalk wk;
    wk.m = m;
    wk.ey0 = qdiv(t, mg);
    wk.ex0 = t - wk.ey0 * m;
    wk.sy = qdiv(nt, mg);
    wk.sx = nt - wk.sy * m;
    return wk;
}

// Register-staged load of a J region into LDS in PAIR format: dword c of a
// row holds J[c] | J[c+1] << 16, so one LDS read feeds one packed dot
// (v_dot2_i32_i16) half of the bilinear interpolation. load() issues the
// global loads and store() writes LDS, so the memory latency overlaps whatever
// the caller does in between (the next level's region is prefetched at its
// predicted position while this level iterates). The region origin is a
// multiple of 4 columns: interior regions move 8 bytes per element (two
// aligned dwords) and write 4 pairs with one 16-B LDS store; regions that cross
// the image border gather the 2 bytes of each pair through reflect-101. KJ*NT
// elements are held in registers; the rest move synchronously in store().
// With cs > 0 the region is written COLUMN-major (pair (r, c) at c * cs + r),
// the layout of the one-wave iteration kernel.
constexpr int KJ = 4;
template <int NT>
struct JPStage {
    uint2 v[KJ];
    const uint8_t *src;
    int pitch, lw, lh, gy0, gx0, PW, PH;
    int cs = 0;
    bool interior;
    JWalk wk;
    __device__ __forceinline__ void setup(const LevelDev &L, int y0, int x0, int pw, int ph, const JWalk &wi,
                                          const JWalk &wb) {
        src = L.p;
        pitch = L.pitch;
        lw = L.w;
        lh = L.h;
        gy0 = y0;
        gx0 = x0;
        PW = pw;
        PH = ph;
        interior = y0 >= 0 && x0 >= 0 && y0 + ph <= lh && x0 + pw <= lw;
        wk = interior ? wi : wb;
    }
    __device__ __forceinline__ void step(int &y, int &x) const {
        x += wk.sx;
        y += wk.sy;
        if (x >= wk.m) {
            x -= wk.m;
            y++;
        }
    }
    __device__ __forceinline__ void fetch(int y, int x, uint2 &out) const {
        typedef const __attribute__((address_space(1))) unsigned gu32;
        if (interior) {
            // bytes 4x .. 4x+7 of the row (the last element reads 4 bytes past the
            // region: inside the 256-B padded pitch, the next row, or the slot slack)
            gu32 *q = (gu32 *)(src + (size_t)(gy0 + y) * pitch + gx0 + 4 * x);
            out.x = q[0];
            out.y = q[1];
        } else {
            const uint8_t *row = src + (size_t)refl101(gy0 + y, lh) * pitch;
            out.x = row[refl101(gx0 + x, lw)];
            out.y = row[refl101(gx0 + x + 1, lw)];
        }
    }
    __device__ __forceinline__ void put(uint32_t *dst, int y, int x, const uint2 &val) const {
        if (interior) {
            uint4 q;
            q.x = __builtin_amdgcn_perm(val.y, val.x, 0x0c010c00u);  // J[4x]   | J[4x+1] << 16
            q.y = __builtin_amdgcn_perm(val.y, val.x, 0x0c020c01u);
            q.z = __builtin_amdgcn_perm(val.y, val.x, 0x0c030c02u);
            q.w = __builtin_amdgcn_perm(val.y, val.x, 0x0c040c03u);  // J[4x+3] | J[4x+4] << 16
            if (cs > 0) {
                uint32_t *d = dst + 4 * x * cs + y;
                d[0] = q.x;
                d[cs] = q.y;
                d[2 * cs] = q.z;
                d[3 * cs] = q.w;
            } else {
                *(uint4 *)(dst + y * PW + 4 * x) = q;
            }
        } else {
            dst[cs > 0 ? x * cs + y : y * PW + x] = val.x | (val.y << 16);
        }
    }
    __device__ __forceinline__ void load(const LevelDev &L, int y0, int x0, int pw, int ph, const JWalk &wi,
                                         const JWalk &wb) {
        setup(L, y0, x0, pw, ph, wi, wb);
        int y = wk.ey0, x = wk.ex0;
#pragma unroll
        for (int k = 0; k < KJ; k++) {
            if (y < PH) fetch(y, x, v[k]);
            step(y, x);
        }
    }
    __device__ __forceinline__ void store(uint32_t *dst) const {
        int y = wk.ey0, x = wk.ex0;
#pragma unroll
        for (int k = 0; k < KJ; k++) {
            if (y < PH) put(dst, y, x, v[k]);
            step(y, x);
        }
        while (y < PH) {
            uint2 t;
            fetch(y, x, t);
            put(dst, y, x, t);
            step(y, x);
        }
    }
    // synchronous load + store (restage inside the iterations)
    __device__ __forceinline__ void copy(uint32_t *dst, const LevelDev &L, int y0, int x0, int pw, int ph,
                                         const JWalk &wi, const JWalk &wb) {
        setup(L, y0, x0, pw, ph, wi, wb);
        int y = wk.ey0, x = wk.ex0;
        while (y < PH) {
            uint2 t;
            fetch(y, x, t);
            put(dst, y, x, t);
            step(y, x);
        }
    }
};

// Level table in LDS (single-tile kernel): entry (pyramid s, level l) = 8 ints
// {ptr lo, ptr hi, w, h, pitch}; s = 0 the I (prev) pyramid, 1 the J (next).
__device__ __forceinline__ void tbl_put(int *tbl, int s, int l, const LevelDev &L) {
    int *e = tbl + (s * kMaxLevels + l) * 8;
    const unsigned long long pv = (unsigned long long)L.p;
    *(int4 *)e = make_int4((int)(unsigned)pv, (int)(unsigned)(pv >> 32), L.w, L.h);
    e[4] = L.pitch;
}
__device__ __forceinline__ LevelDev tbl_get(const int *tbl, int s, int l) {
    const int *e = tbl + (s * kMaxLevels + l) * 8;
    const int4 a = *(const int4 *)e;
    LevelDev L;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane(a.x), hi = (unsigned)__builtin_amdgcn_readfirstlane(a.y);
    L.p = (uint8_t *)(((unsigned long long)hi << 32) | lo);
    L.w = __builtin_amdgcn_readfirstlane(a.z);
    L.h = __builtin_amdgcn_readfirstlane(a.w);
    L.pitch = __builtin_amdgcn_readfirstlane(e[4]);
    L.pad_ = 0;
    return L;
}

// Four simultaneous 64-lane sums (one-wave iterations): s1, s2 and the
// per-lane sum|t1|, sum|t2|, clamped per lane to 2^25 + 1 first (a clamped lane
// alone fails the exactness test below; totals stay below 2^31).
__device__ __forceinline__ void wave_sum4(int &s1, int &s2, unsigned &a1, unsigned &a2) {
    a1 = min(a1, (1u << 25) + 1u);
    a2 = min(a2, (1u << 25) + 1u);
#define PSN_DPP4(ctl, rm)                                                   \
    s1 += __builtin_amdgcn_update_dpp(0, s1, ctl, rm, 0xf, false);          \
    s2 += __builtin_amdgcn_update_dpp(0, s2, ctl, rm, 0xf, false);          \
    a1 += (unsigned)__builtin_amdgcn_update_dpp(0, (int)a1, ctl, rm, 0xf, false); \
    a2 += (unsigned)__builtin_amdgcn_update_dpp(0, (int)a2, ctl, rm, 0xf, false)
    PSN_DPP4(0x111, 0xf);
    PSN_DPP4(0x112, 0xf);
    PSN_DPP4(0x114, 0xf);
    PSN_DPP4(0x118, 0xf);
    PSN_DPP4(0x142, 0xa);
    PSN_DPP4(0x143, 0xc);
#undef PSN_DPP4
    s1 = __builtin_amdgcn_readlane(s1, 63);
    s2 = __builtin_amdgcn_readlane(s2, 63);
    a1 = (unsigned)__builtin_amdgcn_readlane((int)a1, 63);
    a2 = (unsigned)__builtin_amdgcn_readlane((int)a2, 63);
}
// Level geometry of the I window (prevPt/2^l - halfWin): top-left, validity and weights.
struct IGeo {
    int ipx, ipy, w00, w01, w10, w11;
    bool valid;
};
__device__ __forceinline__ IGeo i_geo(float px0, float py0, float hwx, float hwy, int level, int w, int h, int cols,
                                      int rows) {
    IGeo gg;
    const float scale = ldexpf(1.f, -level);
    const float px = __fsub_rn(__fmul_rn(px0, scale), hwx), py = __fsub_rn(__fmul_rn(py0, scale), hwy);
    gg.ipx = cv_floor(px);
    gg.ipy = cv_floor(py);
    gg.valid = !win_outside(gg.ipx, gg.ipy, w, h, cols, rows);
    bilin_weights(__fsub_rn(px, (float)gg.ipx), __fsub_rn(py, (float)gg.ipy), gg.w00, gg.w01, gg.w10, gg.w11);
    return gg;
}

// Fused next-frame ingest (PSN_LK_OVERLAP_FUSED): helper workgroups, and LK
// workgroups whose point is done, pull top-level pyramid tiles from a work
// counter while slower points keep iterating. Every workgroup of the launch
// counts itself done once it stopped pulling; the last one resets the counters
// for the next launch on the stream.
template <int NT>
__device__ __forceinline__ void pyr_tail(const LkLaunchArgs &A, uint8_t *smem) {
    int *tile_slot = (int *)(smem + 2 * kMaxLevels * 8 * 4) + kStRiTile;  // inside the scratch area
    __builtin_amdgcn_s_setprio(0);
    for (;;) {
        __syncthreads();  // every wave is done with LDS (LK state / previous tile)
        if (threadIdx.x == 0) tile_slot[0] = (int)atomicAdd(&A.pyr_ctr[0], 1u);
        __syncthreads();
        const int tile = tile_slot[0];
        if (tile >= A.pyr_ntiles) break;
        const int by = tile / A.pyr_tiles_x, bx = tile - by * A.pyr_tiles_x;
        pyr_tile<NT>(A.pyr, bx, by, smem + kStScratchBytes);  // past the scratch holding tile_slot
    }
    if (threadIdx.x == 0) {
        __threadfence();
        const unsigned done = atomicAdd(&A.pyr_ctr[1], 1u);
        if (done == (unsigned)A.total_wgs - 1) {
            A.pyr_ctr[0] = 0;
            A.pyr_ctr[1] = 0;
        }
    }
}

// Solver table of one level from the A sums (a11, a22 saturating, s12 wrapping)
// and the 15 ordered chain sums c[] (sum s = 0..2: chains 5s..5s+3 the SSE2 lanes,
// 5s+4 the tail; used only when the sum is not exact as an integer):
// {A11, A12, A22, 1/D, minEig, ok} as LKTrackerInvoker computes them (lk_solve).
__device__ __forceinline__ void st_level_table(float *lv, unsigned a11, int s12, unsigned a22, const float (&c)[15],
                                               bool sse, int wh, float min_eig) {
    // a sum whose every term and every partial sum (in any order) is an
    // integer <= 2^24 is exact in float: its integer value; otherwise the
    // ordered chains, combined in the SSE2 build's order
    const auto chain = [&](int i) { return c[i]; };
    const float s0 = combine_a5(chain, 0, sse), s1 = combine_a5(chain, 1, sse), s2 = combine_a5(chain, 2, sse);
    const LkSolve S = lk_solve(a11 <= (unsigned)kExact ? (float)a11 : s0,
                               ((a11 + a22) >> 1) <= (unsigned)kExact ? (float)s12 : s1,
                               a22 <= (unsigned)kExact ? (float)a22 : s2, wh, min_eig);
    lv[0] = S.A11;
    lv[1] = S.A12;
    lv[2] = S.A22;
    lv[3] = S.ok ? S.invD : 0.f;
    lv[4] = S.minEig;
    lv[5] = S.ok ? 1.f : 0.f;
}

// ---- the phases of lk_kernel_st, each written once. The helpers take scalar
// fields and pointers, never the launch arguments or a query whole (an inlined
// function reading those through a parameter keeps a private copy in scratch:
// psn_lk_bx_body.inc). ----

// Scharr plane (Ix, Iy as short2, (h + 1) x DW) of one level's I patch P (row
// stride RS, top-left at image pixel (ipx - 1, ipy - 1)); zero where the centre
// pixel is outside the cols x rows image. Thread t of a group of NT.
template <int NT>
__device__ __forceinline__ void scharr_plane(short2 *Dg, const uint8_t *P, int RS, int DW, int h, unsigned dv_dw, int ipx,
                                             int ipy, int cols, int rows, int t) {
    Walk wk;
    wk.init_m(t, NT, DW, dv_dw);
    for (int idx = t; idx < (h + 1) * DW; idx += NT, wk.step()) {
        const int gy = ipy + wk.y, gx = ipx + wk.x;
        short2 d = make_short2(0, 0);
        if ((unsigned)gy < (unsigned)rows && (unsigned)gx < (unsigned)cols) {
            const uint8_t *p = P + wk.y * RS + wk.x;
            const int a0 = p[0], a1 = p[1], a2 = p[2];
            const int b0 = p[RS], b2 = p[RS + 2];
            const int c0 = p[2 * RS], c1 = p[2 * RS + 1], c2 = p[2 * RS + 2];
            d.x = (short)(3 * (a2 + c2) + 10 * b2 - 3 * (a0 + c0) - 10 * b0);
            d.y = (short)(3 * ((c0 - a0) + (c2 - a2)) + 10 * (c1 - a1));
        }
        Dg[idx] = d;
    }
}

// One window pixel of the A phase: the bilinear window value (5 fractional bits)
// and gradients from the patch at p and the Scharr plane at d, {Iw, Ix | Iy << 16}
// into *iw when the pixel is valid, the three tensor products into the chain planes
// PA (plane stride GP) at pos, and the thread's integer sums. An idle lane
// (!valid) carries zero gradients and writes its zero products into a pad slot.
__device__ __forceinline__ void a_pixel(const uint8_t *p, int RS, const short2 *d, int DW, const IGeo &gg, bool valid,
                                        int2 *iw_out, float *PA, int GP, int pos, unsigned &s11, int &s12, unsigned &s22) {
    const int iw = PSN_DESCALE(__mul24((int)p[0], gg.w00) + __mul24((int)p[1], gg.w01) +
                                   __mul24((int)p[RS], gg.w10) + __mul24((int)p[RS + 1], gg.w11), 9);
    const short2 d00 = d[0], d01 = d[1], d10 = d[DW], d11 = d[DW + 1];
    int ix = PSN_DESCALE(__mul24((int)d00.x, gg.w00) + __mul24((int)d01.x, gg.w01) +
                             __mul24((int)d10.x, gg.w10) + __mul24((int)d11.x, gg.w11), 14);
    int iy = PSN_DESCALE(__mul24((int)d00.y, gg.w00) + __mul24((int)d01.y, gg.w01) +
                             __mul24((int)d10.y, gg.w10) + __mul24((int)d11.y, gg.w11), 14);
    if (valid) *iw_out = make_int2(iw, (ix & 0xffff) | (iy << 16));
    ix = valid ? ix : 0;
    iy = valid ? iy : 0;
    const int xx2 = __mul24(ix, ix), xy = __mul24(ix, iy), yy2 = __mul24(iy, iy);
    PA[pos] = (float)xx2;
    PA[GP + pos] = (float)xy;
    PA[2 * GP + pos] = (float)yy2;
    s11 += (unsigned)xx2;  // |Ix|, |Iy| <= 4080: up to 16 pixels per thread stay < 2^30
    s12 += xy;
    s22 += (unsigned)yy2;
}

// Chain ch (0-3 the SSE2 lanes, 4 the tail) of A sum s (0: A11, 1: A12, 2: A22)
// of the level whose three planes start at PA: its ordered float sum, or 0 when
// the sum is exact as an integer and st_level_table will not use the chains.
// Per-sum exactness: A11 (terms >= 0) is exact when s11 <= 2^24, A22 when
// s22 <= 2^24, A12 when sum|xy| <= (s11 + s22) / 2 <= 2^24.
__device__ __forceinline__ float a_chain(const float *PA, const ChainGeo &GA, int s, int ch, unsigned a11, unsigned a22) {
    const unsigned bound = s == 0 ? a11 : s == 2 ? a22 : (a11 + a22) >> 1;
    float acc = 0.f;
    if (bound > (unsigned)kExact) {
        const int base = s * GA.P + (ch < 4 ? ch * GA.S : 4 * GA.S);
        acc = chain_sum16(PA + base, (ch < 4 ? GA.S : GA.T) >> 4);
    }
    return acc;
}

// The 10 ordered b chains of the planes at pb (lanes 0-9 of the calling wave sum
// one chain each), combined in the SSE2 build's order. Uniform results.
__device__ __forceinline__ void b_chains(const float *pb, const ChainGeo &GB, bool sse, int lane, float &b1, float &b2) {
    float acc = 0.f;
    if (lane < 10) {
        const int ch = lane % 5, s = lane / 5;
        const int base = s * GB.P + (ch < 4 ? ch * GB.S : 4 * GB.S);
        const int nb = (ch < 4 ? GB.S : GB.T) >> 4;
        acc = chain_sum16(pb + base, nb);
    }
    combine_b10([&](int i) { return readlane_f(acc, i); }, sse, b1, b2);
}

// Start of a level: NP becomes the level's guess; the level's solver row lv; run
// = the I window is inside the image and the system is solvable; status and err
// of a level that does not run (they count at level 0 only); the J window's
// start (nx, ny) = NP - halfWin.
struct LevelStart {
    float nx, ny;
    const float *lv;
    bool run;
};
__device__ __forceinline__ LevelStart level_start(int level, int maxL, int flags, float px0, float py0, float hwx,
                                                  float hwy, int w, int h, int cols, int rows, const float *LV,
                                                  float &NPx, float &NPy, int &status, float &errv) {
    LevelStart ls;
    const Guess gs = level_guess(level, maxL, flags, px0, py0, NPx, NPy);
    NPx = gs.x;
    NPy = gs.y;
    const IGeo gg = i_geo(px0, py0, hwx, hwy, level, w, h, cols, rows);
    ls.lv = LV + level * kStLvFloats;
    ls.run = gg.valid && ls.lv[5] != 0.f;
    if (!gg.valid) {
        if (level == 0) {
            status = 0;
            errv = 0.f;
        }
    } else {
        if (flags & PSN_LK_GET_MIN_EIGENVALS) errv = ls.lv[4];
        if (!ls.run && level == 0) status = 0;
    }
    ls.nx = __fsub_rn(gs.x, hwx);
    ls.ny = __fsub_rn(gs.y, hwy);
    return ls;
}

// Origin of the J region staged for a window whose integer start is (ix, iy):
// kStJMargin pixels up and left, the column aligned down to 4 (JPStage).
// uniform: through readfirstlane, for an origin every lane computed alike.
struct JOrigin {
    int x0, y0;
};
__device__ __forceinline__ JOrigin jr_origin(int ix, int iy, bool uniform) {
    JOrigin o;
    o.x0 = (ix - kStJMargin) & ~3;
    o.y0 = iy - kStJMargin;
    if (uniform) {
        o.x0 = __builtin_amdgcn_readfirstlane(o.x0);
        o.y0 = __builtin_amdgcn_readfirstlane(o.y0);
    }
    return o;
}

// Synchronous restage of the J region at origin o into dst by the threads of the
// walk pair (wi interior, wb border). cs > 0: column-major with stride cs (the
// one-wave layout), 0: row-major. wave_local: one wave restages a region that it
// alone reads, between its own reads of the old contents and of the new -- LDS
// executes a wave's accesses in order, the waits keep the compiler from moving
// them across the copy; without it the caller's barriers order the copy.
template <int NT>
__device__ __forceinline__ void jr_restage(uint32_t *dst, const LevelDev &J, JOrigin o, int JRW, int JRH, int cs,
                                           const JWalk &wi, const JWalk &wb, bool wave_local) {
    JPStage<NT> cp;
    cp.cs = cs;
    if (wave_local) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    cp.copy(dst, J, o.y0, o.x0, JRW, JRH, wi, wb);
    if (wave_local) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// Diagnostic stamps of the single-tile kernel (PSN_LK_STAMPS): 60 start, 50
// prologue landed, 51 Scharr of all levels, 52 A products + reduction, 53
// solver table; per level L*10+0 start, +1 J staged, +2 window loaded, +7
// iterations done, +8 iteration count; 40..45 accumulated iteration phases.
template <int NT, int EPT, int E, int OCC = 1>
__global__ __launch_bounds__(NT, OCC) void lk_kernel_st(LkLaunchArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = blockIdx.x;
    if (A.poison_lds) lds_poison<NT>(smem, A.poison_lds);
    if (A.pyr_ntiles > 0 && g >= A.lk_wgs) {  // fused-build helper: tiles only
        pyr_tail<NT>(A, smem);
        return;
    }
    int qi = 0;
    while (qi + 1 < A.nq && g >= A.q[qi + 1].wg_begin) qi++;
    const LkQueryDev &Q = A.q[qi];
    const int pi = lk_query_point(Q, A.counts, A.count_stride, g);
    if (pi < 0) return;  // past the query's device count
    const int w = Q.win_w, h = Q.win_h, wh = w * h;
    const int maxL = Q.max_level, nlev = maxL + 1;
    const int flags = Q.flags;
    const bool sse = (flags & PSN_LK_ACCUM_SCALAR) == 0;
    const int JRW = st_jreg_w(w), JRH = st_jreg_h(h);
    const int PW = w + 3, DW = w + 1;
    const int RS = lk_pat_rs(w);  // I patch row stride (bytes)

    // overlapped A phase (one-wave builds at two workgroups per CU): the prologue
    // computes the coarsest level only; waves 1-3 compute the finer levels while
    // wave 0 iterates (the per-level barriers order their tables before use)
    // (not the 4-row build: its VGPRs would pass 170, one workgroup less per CU)
    const bool ovl = E > 4 && OCC == 1 && Q.st_ovl != 0;
    const int lo = ovl ? maxL : 0;  // the prologue's levels: lo..maxL
    const LkStLayout lay(w, h, sse, nlev, E > 0, ovl);
    int *RI = (int *)(smem + lay.ri);
    float *LV = (float *)(smem + lay.lv);
    uint32_t *JP = (uint32_t *)(smem + lay.jp);
    float *R = (float *)(smem + lay.r);    // b chain planes (iterations)
    float *RA = (float *)(smem + lay.ra);  // A-phase chain planes (prologue; == R outside the one-wave layout)
    const ChainGeo GA = chain_geo_A(w, h, sse), GB = chain_geo_B(w, h, sse);

    // ---- per-thread window pixels (fixed for the whole kernel). Idle lanes
    // (pixel index >= w*h) read pixel 0, carry zero gradients and write their
    // zero products into a pad slot of the chain planes: branch-free loops.
    int ofsJ[EPT], ofsP[EPT], ofsD[EPT], posA_[EPT], posB_[EPT], pix[EPT];
    bool ev[EPT];
#pragma unroll
    for (int k = 0; k < EPT; k++) {
        const int idx = tid + k * NT;
        ev[k] = idx < wh;
        const int i = ev[k] ? idx : 0;
        const int y = qdiv(i, Q.dv_w), x = i - y * w;
        pix[k] = i;
        ofsJ[k] = y * JRW + x;
        ofsP[k] = (y + 1) * RS + x + 1;
        ofsD[k] = y * DW + x;
        posA_[k] = ev[k] ? posA(GA, y, x) : 4 * GA.S + GA.lenT;
        posB_[k] = ev[k] ? posB(GB, y, x) : 4 * GB.S + GB.lenT;
    }

    // the point's waves outrank fused pyramid-tile waves sharing their SIMDs
    if (A.pyr_ntiles > 0) __builtin_amdgcn_s_setprio(2);
    // ---- prologue: zero the A planes' chain padding (ordered by the barrier
    // after the DMA); level geometry comes from the kernel arguments ----
    zero_pads<NT>(RA, GA, 3 * nlev);
    const JWalk wk_int = jwalk_t(tid, JRW >> 2, NT, Q.dv_jrw4), wk_bord = jwalk_t(tid, JRW, NT, Q.dv_jrw);  // J staging walks
    LK_STAMP(60);

    const float hwx = __fmul_rn((float)(w - 1), 0.5f), hwy = __fmul_rn((float)(h - 1), 0.5f);
    const float px0 = A.prev[2 * pi], py0 = A.prev[2 * pi + 1];
    float NPx = 0.f, NPy = 0.f;
    if (flags & PSN_LK_USE_INITIAL_FLOW) {
        NPx = A.next[2 * pi];
        NPy = A.next[2 * pi + 1];
    }
    PSN_STAMPS_ONLY(asm volatile("s_waitcnt vmcnt(0)" ::: "memory");)  // point landed
    LK_STAMP(58);

    // ---- the I patch of every level by LDS-DMA; the coarsest J region into registers ----
#pragma unroll
    for (int l = 0; l < kStMaxLev; l++) {
        if (l > maxL) break;
        if (l < lo) continue;
        const LevelDev I = ring_level(A.ring, Q.prev_slot, l);
        const IGeo gg = i_geo(px0, py0, hwx, hwy, l, w, h, I.w, I.h);
        if (!gg.valid) continue;
        dma_patch<NT>(smem + lay.pim + l * lay.pim_stride, I, gg.ipy - 1, gg.ipx - 1, PW, h + 3, lk_pat_m(w), Q.dv_pm);
    }
    LK_STAMP(62);
    // level table for the level loops (ordered by the barrier below)
    int *TBL = (int *)(smem + lay.tbl);
    if (tid < 2 * kStMaxLev) {
        const int ts = tid >= kStMaxLev ? 1 : 0, tl = tid - ts * kStMaxLev;
        LevelDev L = ring_level(A.ring, ts ? Q.next_slot : Q.prev_slot, 0);
#pragma unroll
        for (int l = 1; l < kStMaxLev; l++)
            if (tl == l) L = ring_level(A.ring, ts ? Q.next_slot : Q.prev_slot, l);
        tbl_put(TBL, ts, tl, L);
    }
    LK_STAMP(63);
    JPStage<NT> pf;  // prefetched J region of level pf_level at origin pfo
    int pf_level = maxL;
    JOrigin pfo;
    {
        // the coarsest level's start as level_start will compute it
        const Guess gs = level_guess(maxL, maxL, flags, px0, py0, NPx, NPy);
        pfo = jr_origin(cv_floor(__fsub_rn(gs.x, hwx)), cv_floor(__fsub_rn(gs.y, hwy)), false);
        pf.load(ring_level_u(A.ring, Q.next_slot, maxL), pfo.y0, pfo.x0, JRW, JRH, wk_int, wk_bord);
    }
    LK_STAMP(59);
    dma_wait();
    __syncthreads();
    LK_STAMP(50);

    // ---- A phase for ALL levels at once (the I window does not depend on the
    // flow): Scharr of every patch; window values, tensor products and sums;
    // one reduction barrier; wave 0 sums the float chains of every level in
    // parallel lanes and writes the per-level solver table LV ----
#pragma unroll
    for (int l = 0; l < kStMaxLev; l++) {
        if (l > maxL) break;
        if (l < lo) continue;
        const LevelDev I = ring_level(A.ring, Q.prev_slot, l);
        const IGeo gg = i_geo(px0, py0, hwx, hwy, l, w, h, I.w, I.h);
        if (!gg.valid) continue;
        const uint8_t *P = smem + lay.pim + l * lay.pim_stride + ((gg.ipx - 1) & 3);
        short2 *Dg = (short2 *)(smem + lay.dg + l * lay.dg_stride);
        scharr_plane<NT>(Dg, P, RS, DW, h, Q.dv_dw, gg.ipx, gg.ipy, I.w, I.h, tid);
    }
    __syncthreads();
    LK_STAMP(51);
#pragma unroll
    for (int l = 0; l < kStMaxLev; l++) {
        if (l > maxL) break;
        if (l < lo) continue;
        const LevelDev I = ring_level(A.ring, Q.prev_slot, l);
        const IGeo gg = i_geo(px0, py0, hwx, hwy, l, w, h, I.w, I.h);
        // s11 and s22 are reduced saturating, s12 wrapping (a_chain: the exactness bounds)
        unsigned s11 = 0, s22 = 0;
        int s12 = 0;
        if (gg.valid) {
            const uint8_t *P = smem + lay.pim + l * lay.pim_stride + ((gg.ipx - 1) & 3);
            const short2 *Dg = (const short2 *)(smem + lay.dg + l * lay.dg_stride);
            int2 *IW = (int2 *)(smem + lay.iw + l * lay.iw_stride);
            float *PA = RA + l * 3 * GA.P;
#pragma unroll
            for (int k = 0; k < EPT; k++)
                a_pixel(P + ofsP[k], RS, Dg + ofsD[k], DW, gg, ev[k], IW + pix[k], PA, GA.P, posA_[k], s11, s12, s22);
        }
        s11 = wave_sum_sat(s11);
        s12 = wave_sum(s12);
        s22 = wave_sum_sat(s22);
        if (lane == 0) {
            int *ra = RI + kStRiA + l * 4 * 8 + wid;
            ra[0] = (int)s11;
            ra[8] = s12;
            ra[16] = (int)s22;
        }
    }
    __syncthreads();
    LK_STAMP(52);
    if (wid == 0) {
        float *CH = (float *)RI;  // 15 chain results per level (the iteration scratch is still unused)
        // chain pass: slot q -> (level q/15, sum (q%15)/5, chain q%5); two slots per lane
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int q = lane + 64 * half;
            const int l = q / 15, r = q - 15 * (q / 15);
            if (l <= maxL && l >= lo) {
                unsigned a11 = 0, a22 = 0;
#pragma unroll
                for (int ww = 0; ww < NW; ww++) {
                    a11 = sat_add(a11, (unsigned)RI[kStRiA + l * 32 + ww]);
                    a22 = sat_add(a22, (unsigned)RI[kStRiA + l * 32 + 16 + ww]);
                }
                const int s = r / 5, ch = r - 5 * (r / 5);
                CH[q] = a_chain(RA + l * 3 * GA.P, GA, s, ch, a11, a22);
            }
        }
        // CH written by other lanes of this wave: LDS executes a wave's accesses in
        // order; the clobber keeps the compiler from hoisting the reads
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane <= maxL && lane >= lo) {
            const int l = lane;
            unsigned a11 = 0, a22 = 0;
            int s12 = 0;
#pragma unroll
            for (int ww = 0; ww < NW; ww++) {
                const int *ra = RI + kStRiA + l * 32 + ww;
                a11 = sat_add(a11, (unsigned)ra[0]);
                s12 += ra[8];
                a22 = sat_add(a22, (unsigned)ra[16]);
            }
            float c[15];
#pragma unroll
            for (int k = 0; k < 15; k++) c[k] = CH[l * 15 + k];
            st_level_table(LV + l * kStLvFloats, a11, s12, a22, c, sse, wh, Q.min_eig);
        }
    }
    __syncthreads();  // LV published; the A planes in R are dead from here
    LK_STAMP(53);
    zero_pads<NT>(R, GB, 4);  // b planes (2 buffers x 2 sums) now own R; ordered by the first iteration's barrier

    int status = 1;
    float errv = 0.f;
    // accumulated iteration phases (slots 40..47), ordered stamps
    PSN_STAMPS_ONLY(unsigned long long acc_ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t_ph = 0;)
    JOrigin jr = {0, 0};  // origin of the staged J region

    if constexpr (E > 0) {
        // ---- one-wave iterations: wave 0 runs the LK iterations of every level
        // with no workgroup barrier inside the loop; waves 1..NW-1 meanwhile
        // stage the next level's J region (predicted start) into the other
        // half of the double-buffered, column-major J region. ----
        const int JRHc = st_jrh_cm(h);
        uint32_t *const JPB0 = JP, *const JPB1 = JP + st_jp_cm_dw(w, h);
        // lane -> (window column, row group): columns sorted by SSE2 chain class
        // (class c < 4: x = c, c+4, ... < n8; class 4 = the scalar tail)
        const int G = Q.ow_g, RG = Q.ow_rg;
        const int n8 = sse ? (w / 8) * 8 : 0, cw = n8 / 4;
        const int cr = qdiv(lane, Q.dv_g), gi = lane - cr * G;
        const bool lane_on = cr < w;
        const int ccl = qdiv(cr, sse ? Q.dv_cw : 0u);  // chain class of an SSE2 column
        const int colx = !lane_on ? 0 : (cr < n8 ? ccl + 4 * (cr - ccl * cw) : cr);
        const int oy0 = gi * RG;
        const int lane_off = colx * JRHc + oy0;
        // class c occupies lanes (last[c-1], last[c]]; empty classes repeat the previous bound
        const int last4 = w * G - 1;
        // this lane ends class cls_end (it publishes the class's scans), or -1; with
        // no tail columns (w % 8 == 0) the last lane ends class 3 and the empty class
        // 4 alike and publishes both (class 4's sums are then 0)
        int cls_end = -1;
        bool end3 = false;
        if (lane == last4) {
            cls_end = 4;
            end3 = n8 > 0 && n8 == w;
        }
        if (n8 > 0)
            for (int c = 0; c < 4; c++)
                if (lane == (c + 1) * cw * G - 1 && lane != last4) cls_end = c;
        int4 *CSX = (int4 *)(RI + kStRiIt + 16);  // 5 x int4 class scans
        if (n8 == 0 && tid < 4) CSX[tid] = make_int4(0, 0, 0, 0);  // ordered by the first level barrier
        // loop constants pinned in registers (not re-read from the kernel arguments)
        double eps2 = Q.eps2;
        int maxc = Q.max_count;
        asm volatile("" : "+v"(eps2), "+s"(maxc));
        const int th = max(tid - 64, 0);
        const JWalk wkh_int = jwalk_t(th, JRW >> 2, NT - 64, Q.dv_jrw4), wkh_bord = jwalk_t(th, JRW, NT - 64, Q.dv_jrw);
        const JWalk wk0_int = jwalk_t(lane, JRW >> 2, 64, Q.dv_jrw4), wk0_bord = jwalk_t(lane, JRW, 64, Q.dv_jrw);
        pf.cs = JRHc;
        // overlapped A phase of level l by ONE wave (no barrier: a wave's LDS
        // accesses complete in order): I patch by LDS-DMA, Scharr plane, window
        // values and A products, the 15 ordered chains when a sum is inexact, and
        // the level's solver table -- the prologue's arithmetic, one wave wide
        auto a_level_wave = [&](int l) {
            const LevelDev I = tbl_get(TBL, 0, l);
            const IGeo gg = i_geo(px0, py0, hwx, hwy, l, w, h, I.w, I.h);
            if (!gg.valid) return;
            uint8_t *const pim = smem + lay.pim + l * lay.pim_stride;
            dma_patch_t<64>(pim, I, gg.ipy - 1, gg.ipx - 1, PW, h + 3, lk_pat_m(w), Q.dv_pm, lane);
            dma_wait();
            const uint8_t *P = pim + ((gg.ipx - 1) & 3);
            short2 *Dg = (short2 *)(smem + lay.dg + l * lay.dg_stride);
            scharr_plane<64>(Dg, P, RS, DW, h, Q.dv_dw, gg.ipx, gg.ipy, I.w, I.h, lane);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            int2 *IW = (int2 *)(smem + lay.iw + l * lay.iw_stride);
            float *PA = RA + l * 3 * GA.P;
            unsigned s11 = 0, s22 = 0;
            int s12 = 0;
            for (int i0 = 0; i0 < wh; i0 += 64) {
                const int idx = i0 + lane;
                const bool v = idx < wh;
                const int i = v ? idx : 0;
                const int y = qdiv(i, Q.dv_w), x = i - y * w;
                a_pixel(P + (y + 1) * RS + x + 1, RS, Dg + y * DW + x, DW, gg, v, IW + i, PA, GA.P,
                        v ? posA(GA, y, x) : 4 * GA.S + GA.lenT, s11, s12, s22);
            }
            s11 = wave_sum_sat(s11);
            s12 = wave_sum(s12);
            s22 = wave_sum_sat(s22);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            float acc = 0.f;
            if (lane < 15) acc = a_chain(PA, GA, lane / 5, lane - 5 * (lane / 5), s11, s22);
            float c[15];
#pragma unroll
            for (int k = 0; k < 15; k++) c[k] = readlane_f(acc, k);
            if (lane == 0)
                st_level_table(LV + l * kStLvFloats, s11, s12, s22, c, sse, wh, Q.min_eig);
        };
        LK_STAMP(54);
        bool pf_regs = true;  // the prefetched region is still in registers (prologue) vs already in LDS
        int buf = 0;
        float *XCH = (float *)(RI + kStRiIt);  // wave 0 -> all: NPx, NPy at the end of a level

        for (int level = maxL; level >= 0; level--) {
            LK_STAMP(level * 10 + 0);
            const LevelDev I = tbl_get(TBL, 0, level);
            const LevelDev J = tbl_get(TBL, 1, level);
            const int cols = I.w, rows = I.h;
            const LevelStart ls =
                level_start(level, maxL, flags, px0, py0, hwx, hwy, w, h, cols, rows, LV, NPx, NPy, status, errv);
            const float *lv = ls.lv;
            const bool run = ls.run;
            float nx = ls.nx, ny = ls.ny;
            uint32_t *const JC = buf ? JPB1 : JPB0;
            if (run) {
                const int inx0 = __builtin_amdgcn_readfirstlane(cv_floor(nx));
                const int iny0 = __builtin_amdgcn_readfirstlane(cv_floor(ny));
                if (pf_level == level && jr_covers(inx0, iny0, w, h, pfo.x0, pfo.y0, JRW, JRH)) {
                    if (pf_regs) {
                        LK_STAMP(55);
                        pf.store(JC);
                        LK_STAMP(56);
                    }
                    jr = pfo;
                } else {
                    jr = jr_origin(inx0, iny0, false);
                    jr_restage<NT>(JC, J, jr, JRW, JRH, JRHc, wk_int, wk_bord, false);
                }
            }
            pf_regs = false;
            __syncthreads();  // JC complete; every wave is past the previous level
            LK_STAMP(level * 10 + 1);
            // next level's region where this level's start predicts it
            pf_level = level > 0 ? level - 1 : -1;
            const Guess gn = level_guess(level - 1, maxL, flags, px0, py0, NPx, NPy);
            pfo = jr_origin(cv_floor(__fsub_rn(gn.x, hwx)), cv_floor(__fsub_rn(gn.y, hwy)), true);

            if (wid != 0) {
                if (ovl && level == maxL) {  // the finer levels' A phase: wave k takes levels maxL - k, maxL - k - 3, ...
                    for (int l = maxL - wid; l >= 0; l -= NW - 1) a_level_wave(l);
                    // wave k's A phase done: slot 59 - 10 k
                    PSN_STAMP(A.stamps, lane == 0 && wid < 4, (size_t)blockIdx.x * 64 + 59 - 10 * wid);
                }
                if (level > 0)
                    jr_restage<NT>(buf ? JPB0 : JPB1, tbl_get(TBL, 1, level - 1), pfo, JRW, JRH, JRHc, wkh_int, wkh_bord,
                                   false);
            } else if (run) {
                const float A11 = lv[0], A12 = lv[1], A22 = lv[2], D = lv[3];
                // the lane's window rows, two rows per dword (int16 halves): I, Ix,
                // Iy, |Ix| + |Iy|; rows past the window carry zero gradients
                constexpr int E2 = (E + 1) / 2;
                unsigned IxP[E2], IyP[E2], AxP[E2], AyP[E2];
                int Cw[2 * E2];  // 256 - 512 * I: the bilinear sum plus Cw, >> 9, is J* - I*
                int Iw_[E];
                {
                    const int2 *IW = (const int2 *)(smem + lay.iw + level * lay.iw_stride);
                    int iw[2 * E2], ix[2 * E2], iy[2 * E2];
#pragma unroll
                    for (int k = 0; k < 2 * E2; k++) {
                        const int y = oy0 + k;
                        const bool v = k < E && lane_on && k < RG && y < h;
                        const int2 t = IW[v ? y * w + colx : 0];
                        iw[k] = k < E ? t.x : 0;
                        ix[k] = v ? (int)(short)(t.y & 0xffff) : 0;
                        iy[k] = v ? (t.y >> 16) : 0;
                        if (k < E) Iw_[k] = t.x;
                    }
#pragma unroll
                    for (int q = 0; q < E2; q++) {
                        Cw[2 * q] = 256 - 512 * iw[2 * q];
                        Cw[2 * q + 1] = 256 - 512 * iw[2 * q + 1];
                        IxP[q] = pack_w(ix[2 * q], ix[2 * q + 1]);
                        IyP[q] = pack_w(iy[2 * q], iy[2 * q + 1]);
                        AxP[q] = pack_w(abs(ix[2 * q]), abs(ix[2 * q + 1]));
                        AyP[q] = pack_w(abs(iy[2 * q]), abs(iy[2 * q + 1]));
                    }
                }
                LK_STAMP(level * 10 + 2);
                float pdx = 0.f, pdy = 0.f;
                int jdone = 0;
                unsigned dP[E2];
                // diffs J - I of the lane's rows at offset (ox, oy) of the region
                // (packed pairs into dP) and the lane's s1, s2, sum|t1|, sum|t2|
                auto products = [&](int ox, int oy, unsigned W0, unsigned W1, int &s1, int &s2, unsigned &a,
                                    unsigned &a2) {
                    const uint32_t *jb = JC + __mul24(ox, JRHc) + oy + lane_off;
                    unsigned rr[2 * E2 + 1];
#pragma unroll
                    for (int k = 0; k <= 2 * E2; k++) rr[k] = jb[k];
                    s1 = 0;
                    s2 = 0;
                    a = 0;
                    a2 = 0;
#pragma unroll
                    for (int q = 0; q < E2; q++) {
                        // (sum + 256) >> 9 - I == (sum + 256 - 512 I) >> 9: the diffs directly
                        const int d0 = sdot2v(rr[2 * q + 1], W1, sdot2v(rr[2 * q], W0, Cw[2 * q])) >> 9;
                        const int d1 = sdot2v(rr[2 * q + 2], W1, sdot2v(rr[2 * q + 1], W0, Cw[2 * q + 1])) >> 9;
                        const s16x2 d = __builtin_bit_cast(s16x2, __builtin_amdgcn_perm((unsigned)d1, (unsigned)d0, 0x05040100u));
                        dP[q] = __builtin_bit_cast(unsigned, d);
                        s1 = sdot2(dP[q], IxP[q], s1);
                        s2 = sdot2(dP[q], IyP[q], s2);
                        const s16x2 ad = __builtin_elementwise_max(d, (s16x2)0 - d);
                        a = udot2(__builtin_bit_cast(unsigned, ad), AxP[q], a);  // per lane < 2^29
                        a2 = udot2(__builtin_bit_cast(unsigned, ad), AyP[q], a2);
                    }
                };
                for (int j = 0; j < maxc; j++) {
                    jdone = j + 1;
                    PSN_CLK_ORDERED(t_ph);
                    const int inx = cv_floor(nx), iny = cv_floor(ny);
                    int iw00, iw01, iw10, iw11;
                    bilin_weights(__fsub_rn(nx, (float)inx), __fsub_rn(ny, (float)iny), iw00, iw01, iw10, iw11);
                    const unsigned W0 = pack_w(iw00, iw01), W1 = pack_w(iw10, iw11);
                    // speculative: the offsets are clamped into the region, the
                    // bounds / region tests below decide whether the sums count
                    const int ox = min(max(inx - jr.x0, 0), JRW - w - 1), oy = min(max(iny - jr.y0, 0), JRH - h - 1);
                    int s1, s2;
                    unsigned a, a2;
                    products(ox, oy, W0, W1, s1, s2, a, a2);
                    int sinx = __builtin_amdgcn_readfirstlane(inx), siny = __builtin_amdgcn_readfirstlane(iny);
                    // keep the (rarely taken) branches below the products: the
                    // conditions formally depend on them
                    asm volatile("; order %2 %3 %4 %5" : "+s"(sinx), "+s"(siny) : "v"(s1), "v"(s2), "v"(a), "v"(a2));
                    // (win_outside, written out: through the helper the one-wave builds' VGPR counts move)
                    if (sinx < -w || sinx >= cols || siny < -h || siny >= rows) {
                        if (level == 0) status = 0;
                        break;
                    }
                    if (!(jr_covers(sinx, siny, w, h, jr.x0, jr.y0, JRW, JRH))) {
                        // restage by this wave alone (the other waves never read JC)
                        jr = jr_origin(sinx, siny, true);
                        jr_restage<NT>(JC, J, jr, JRW, JRH, JRHc, wk0_int, wk0_bord, true);
                        products(sinx - jr.x0, siny - jr.y0, W0, W1, s1, s2, a, a2);
                        PSN_PH_COUNT(acc_ph, 5);
                    }
                    PSN_PH_MARK(acc_ph, t_ph, 0);
                    const int l1 = s1, l2 = s2;  // the lane's own sums (class path)
                    const unsigned la1 = a, la2 = a2;
                    wave_sum4(s1, s2, a, a2);
                    PSN_PH_MARK(acc_ph, t_ph, 1);
                    float b1, b2;
                    if (sums_exact(a, s1) && sums_exact(a2, s2)) {
                        // every partial sum in any order is an integer of magnitude <= 2^24
                        b1 = (float)s1;
                        b2 = (float)s2;
                    } else {
                        PSN_PH_COUNT(acc_ph, 6);
                        // per SSE2 chain class: inclusive scans of the lanes' sums and
                        // of sum|t1|, sum|t2|; class-end lanes publish to LDS
                        unsigned a1 = min(la1, (1u << 25) + 1u);  // a clamped lane fails its class
                        a2 = min(la2, (1u << 25) + 1u);
                        const int c1 = wave_scan(l1), c2 = wave_scan(l2);
                        a1 = (unsigned)wave_scan((int)a1);
                        a2 = (unsigned)wave_scan((int)a2);
                        if (cls_end >= 0) CSX[cls_end] = make_int4(c1, c2, (int)a1, (int)a2);
                        if (end3) CSX[3] = make_int4(c1, c2, (int)a1, (int)a2);
                        int S1[5], S2[5];
                        bool exact = true;
                        int4 pv = make_int4(0, 0, 0, 0);
#pragma unroll
                        for (int c = 0; c < 5; c++) {
                            const int4 cv = CSX[c];  // classes 0-3 stay zero without SSE2 lanes
                            S1[c] = cv.x - pv.x;     // wrapping: exact whenever the class passes
                            S2[c] = cv.y - pv.y;
                            exact = exact && sums_exact((unsigned)(cv.z - pv.z), S1[c]) &&
                                    sums_exact((unsigned)(cv.w - pv.w), S2[c]);
                            pv = cv;
                        }
                        if (exact) {
                            // every chain's partial sums are integers <= 2^24: each chain
                            // sum is its integer sum; combine in the SSE2 build's order
                            combine_b10([&](int i) { return (float)(i < 5 ? S1[i] : S2[i - 5]); }, sse, b1, b2);
                        } else {
                            // ordered float chains: products chain-major into R, one lane per chain
#pragma unroll
                            for (int k = 0; k < E; k++) {
                                const int y = oy0 + k;
                                if (lane_on && k < RG && y < h) {
                                    const int d = (int)(short)(k & 1 ? dP[k >> 1] >> 16 : dP[k >> 1] & 0xffff);
                                    const int gx = (int)(short)(k & 1 ? IxP[k >> 1] >> 16 : IxP[k >> 1] & 0xffff);
                                    const int gy = (int)(short)(k & 1 ? IyP[k >> 1] >> 16 : IyP[k >> 1] & 0xffff);
                                    const int pos = posB(GB, y, colx);
                                    R[pos] = (float)__mul24(d, gx);
                                    R[GB.P + pos] = (float)__mul24(d, gy);
                                }
                            }
                            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                            b_chains(R, GB, sse, lane, b1, b2);
                            PSN_PH_COUNT(acc_ph, 4);
                        }
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // CSX / R reads done before the next writes
                    }
                    PSN_PH_MARK(acc_ph, t_ph, 2);
                    float dx, dy;
                    const double dd = lk_update(A11, A12, A22, D, b1, b2, hwx, hwy, nx, ny, NPx, NPy, dx, dy);
                    PSN_PH_MARK(acc_ph, t_ph, 3);
                    if (lk_stop(dd, eps2, j, dx, dy, pdx, pdy, NPx, NPy)) break;
                }
                LK_STAMP(level * 10 + 7);
                LK_COUNT(level * 10 + 8, jdone);
                (void)jdone;

                if (level == 0 && status && A.err && (flags & PSN_LK_GET_MIN_EIGENVALS) == 0) {
                    const float qx = __fsub_rn(NPx, hwx), qy = __fsub_rn(NPy, hwy);
                    const int iqx = cv_floor(qx), iqy = cv_floor(qy);
                    if (win_outside(iqx, iqy, w, h, cols, rows)) {
                        status = 0;
                    } else if ((flags & PSN_LK_ERR_STATUS_ONLY) == 0) {  // (else the re-check was all: err[] = 0)
                        int iw00, iw01, iw10, iw11;
                        bilin_weights(__fsub_rn(qx, (float)iqx), __fsub_rn(qy, (float)iqy), iw00, iw01, iw10, iw11);
                        if (!(jr_covers(iqx, iqy, w, h, jr.x0, jr.y0, JRW, JRH))) {
                            jr = jr_origin(iqx, iqy, false);
                            jr_restage<NT>(JC, J, jr, JRW, JRH, JRHc, wk0_int, wk0_bord, true);
                        }
                        const unsigned W0 = pack_w(iw00, iw01), W1 = pack_w(iw10, iw11);
                        const uint32_t *jb = JC + (iqx - jr.x0) * JRHc + (iqy - jr.y0) + lane_off;
                        unsigned ea = 0;
#pragma unroll
                        for (int k = 0; k < E; k++) {
                            const int jv = sdot2(jb[k + 1], W1, sdot2(jb[k], W0, 1 << 8)) >> 9;
                            const int y = oy0 + k;
                            ea += (unsigned)((lane_on && k < RG && y < h) ? abs(jv - Iw_[k]) : 0);
                        }
                        ea = (unsigned)__builtin_amdgcn_readlane(wave_scan((int)ea), 63);
                        // ea <= kStErrSumMax <= kExact (psn_lk_kernels.h): every partial sum of
                        // errval += |diff|, in any order, is an exact integer
                        const float errval = (float)ea;
                        errv = lk_err(errval, wh);
                    }
                }
            }
            if (tid == 0) {
                XCH[0] = NPx;
                XCH[1] = NPy;
            }
            __syncthreads();  // wave 0 done with JC; the next level's region staged
            NPx = XCH[0];
            NPy = XCH[1];
            buf ^= 1;
        }
    } else {
        // ---- multi-wave iterations: the windows with more than kOwMaxRows rows per
        // lane of the one-wave geometry (40x20, 33x31, 20x50, every w > 64), a
        // one-wave plan past the LDS cap, and the forced workgroup sizes. Every wave
        // owns EPT pixels per thread; one workgroup barrier per iteration. ----
        for (int level = maxL; level >= 0; level--) {
            LK_STAMP(level * 10 + 0);
            const LevelDev I = tbl_get(TBL, 0, level);
            const LevelDev J = tbl_get(TBL, 1, level);
            const int cols = I.w, rows = I.h;
            const LevelStart ls =
                level_start(level, maxL, flags, px0, py0, hwx, hwy, w, h, cols, rows, LV, NPx, NPy, status, errv);
            const float *lv = ls.lv;
            const bool run = ls.run;
            float nx = ls.nx, ny = ls.ny;
            if (run) {
                // this level's J region: the prefetched registers if they cover the start
                const int inx0 = cv_floor(nx), iny0 = cv_floor(ny);
                if (pf_level == level && jr_covers(inx0, iny0, w, h, pfo.x0, pfo.y0, JRW, JRH)) {
                    pf.store(JP);
                    jr = pfo;
                } else {
                    jr = jr_origin(inx0, iny0, false);
                    jr_restage<NT>(JP, J, jr, JRW, JRH, 0, wk_int, wk_bord, false);
                }
            }
            pf_level = -1;
            if (level > 0) {  // prefetch the next level's region where this level's start predicts it
                const Guess gn = level_guess(level - 1, maxL, flags, px0, py0, NPx, NPy);
                pfo = jr_origin(cv_floor(__fsub_rn(gn.x, hwx)), cv_floor(__fsub_rn(gn.y, hwy)), false);
                pf_level = level - 1;
                pf.load(tbl_get(TBL, 1, level - 1), pfo.y0, pfo.x0, JRW, JRH, wk_int, wk_bord);
            }
            if (!run) continue;
            __syncthreads();  // JP published (every wave finished the previous level's reads)
            LK_STAMP(level * 10 + 1);

            const float A11 = lv[0], A12 = lv[1], A22 = lv[2], D = lv[3];
            int Iw_[EPT], Ix_[EPT], Iy_[EPT];
            unsigned Sxy[EPT];
            {
                const int2 *IW = (const int2 *)(smem + lay.iw + level * lay.iw_stride);
#pragma unroll
                for (int k = 0; k < EPT; k++) {
                    const int2 t = IW[pix[k]];
                    Iw_[k] = t.x;
                    Ix_[k] = ev[k] ? (int)(short)(t.y & 0xffff) : 0;
                    Iy_[k] = ev[k] ? (t.y >> 16) : 0;
                    Sxy[k] = (unsigned)(abs(Ix_[k]) + abs(Iy_[k]));
                }
            }
            LK_STAMP(level * 10 + 2);
            float pdx = 0.f, pdy = 0.f;
            int jdone = 0;

            for (int j = 0; j < Q.max_count; j++) {
                jdone = j + 1;
                PSN_CLK_ORDERED(t_ph);
                const int inx = cv_floor(nx), iny = cv_floor(ny);
                if (win_outside(inx, iny, w, h, cols, rows)) {
                    if (level == 0) status = 0;
                    break;
                }
                int iw00, iw01, iw10, iw11;
                bilin_weights(__fsub_rn(nx, (float)inx), __fsub_rn(ny, (float)iny), iw00, iw01, iw10, iw11);
                if (!(jr_covers(inx, iny, w, h, jr.x0, jr.y0, JRW, JRH))) {
                    // every wave's JP reads of iteration j-1 precede that iteration's
                    // barrier, which this wave has passed
                    jr = jr_origin(inx, iny, false);
                    jr_restage<NT>(JP, J, jr, JRW, JRH, 0, wk_int, wk_bord, false);
                    __syncthreads();
                    PSN_PH_COUNT(acc_ph, 5);
                }
                const unsigned W0 = pack_w(iw00, iw01), W1 = pack_w(iw10, iw11);
                const uint32_t *jb = JP + (iny - jr.y0) * JRW + (inx - jr.x0);
                float *pb = R + (j & 1) * 2 * GB.P;
                int s1 = 0, s2 = 0;
                unsigned a = 0;
#pragma unroll
                for (int k = 0; k < EPT; k++) {
                    const uint32_t *p = jb + ofsJ[k];
                    const int jv = sdot2(p[JRW], W1, sdot2(p[0], W0, 1 << 8)) >> 9;
                    const int diff = jv - Iw_[k];
                    const int t1 = __mul24(diff, Ix_[k]), t2 = __mul24(diff, Iy_[k]);
                    pb[posB_[k]] = (float)t1;
                    pb[GB.P + posB_[k]] = (float)t2;
                    s1 += t1;
                    s2 += t2;
                    // |t1| + |t2| (both factors < 2^14); per thread < 2^30
                    a += (unsigned)__mul24(abs(diff), (int)Sxy[k]);
                }
                PSN_PH_MARK(acc_ph, t_ph, 0);
                block_sums3<NT>(s1, s2, a, RI + kStRiIt + 32 * (j & 1));  // the iteration's barrier
                PSN_PH_MARK(acc_ph, t_ph, 1);
                float b1, b2;
                if (a <= (unsigned)kExact) {
                    b1 = (float)s1;
                    b2 = (float)s2;
                } else {
                    b_chains(pb, GB, sse, lane, b1, b2);  // every wave for itself: no second barrier
                    PSN_PH_COUNT(acc_ph, 4);
                }
                PSN_PH_MARK(acc_ph, t_ph, 2);
                float dx, dy;
                const double dd = lk_update(A11, A12, A22, D, b1, b2, hwx, hwy, nx, ny, NPx, NPy, dx, dy);
                PSN_PH_MARK(acc_ph, t_ph, 3);
                if (lk_stop(dd, Q.eps2, j, dx, dy, pdx, pdy, NPx, NPy)) break;
            }
            LK_STAMP(level * 10 + 7);
            LK_COUNT(level * 10 + 8, jdone);
            (void)jdone;

            if (level == 0 && status && A.err && (flags & PSN_LK_GET_MIN_EIGENVALS) == 0) {
                const float qx = __fsub_rn(NPx, hwx), qy = __fsub_rn(NPy, hwy);
                const int iqx = cv_floor(qx), iqy = cv_floor(qy);
                if (win_outside(iqx, iqy, w, h, cols, rows)) {
                    status = 0;
                    continue;
                }
                if (flags & PSN_LK_ERR_STATUS_ONLY) continue;  // the re-check was all: err[] = 0
                int iw00, iw01, iw10, iw11;
                bilin_weights(__fsub_rn(qx, (float)iqx), __fsub_rn(qy, (float)iqy), iw00, iw01, iw10, iw11);
                __syncthreads();  // every wave is done with JP
                if (!(jr_covers(iqx, iqy, w, h, jr.x0, jr.y0, JRW, JRH))) {
                    jr = jr_origin(iqx, iqy, false);
                    jr_restage<NT>(JP, J, jr, JRW, JRH, 0, wk_int, wk_bord, false);
                    __syncthreads();
                }
                const unsigned W0 = pack_w(iw00, iw01), W1 = pack_w(iw10, iw11);
                const uint32_t *jb = JP + (iqy - jr.y0) * JRW + (iqx - jr.x0);
                int e1 = 0, e2 = 0;
                unsigned ea = 0;
#pragma unroll
                for (int k = 0; k < EPT; k++) {
                    const uint32_t *p = jb + ofsJ[k];
                    const int jv = sdot2(p[JRW], W1, sdot2(p[0], W0, 1 << 8)) >> 9;
                    ea += (unsigned)(ev[k] ? abs(jv - Iw_[k]) : 0);
                }
                block_sums3<NT>(e1, e2, ea, RI + kStRiErr);
                // ea <= kStErrSumMax <= kExact (psn_lk_kernels.h): every partial sum of
                // errval += |diff|, in any order, is an exact integer
                const float errval = (float)ea;
                errv = lk_err(errval, wh);
            }
        }
    }  // multi-wave iterations

    LK_STAMP(61);
    for (int i = 0; i < 8; i++) LK_COUNT(40 + i, acc_ph[i]);
    if (tid == 0) {
        A.next[2 * pi] = NPx;
        A.next[2 * pi + 1] = NPy;
        A.status[pi] = (uint8_t)status;
        if (A.err) A.err[pi] = errv;
    }
    if (A.pyr_ntiles > 0) pyr_tail<NT>(A, smem);
}

// The instantiations of lk_kernel_st, written ONCE: the launch dispatch and the
// dynamic-LDS attribute loop of st_kernels_init are both generated from this
// list, so a variant cannot launch without its attribute.
// X(NT workgroup size, EPT window pixels per thread, E one-wave
// rows per lane (0: multi-wave iterations), OCC workgroups per CU the build is
// held to). The OCC 3 builds are the one-wave kernels held to 168 VGPRs: three
// workgroups per CU when the launch has more points than two per CU can hold.
#define PSN_ST_KERNELS(X)                                                                 \
    X(64, 2, 0, 1) X(64, 4, 0, 1) X(128, 2, 0, 1) X(128, 4, 0, 1) X(256, 2, 0, 1)         \
    X(512, 1, 0, 1) X(512, 2, 0, 1) X(256, 2, 4, 1) X(256, 2, 7, 1) X(256, 2, 8, 1)       \
    X(256, 4, 8, 1) X(256, 2, 16, 1) X(256, 4, 16, 1) X(256, 4, 0, 1) X(256, 2, 4, 3)     \
    X(256, 2, 7, 3) X(256, 2, 8, 3)

hipError_t launch_lk_st(const LkLaunchArgs &a, int total_wgs, int nt, int ept, int e, int occ, int lds_bytes,
                        hipStream_t s) {
    if (total_wgs <= 0) return hipSuccess;
    const dim3 grid(total_wgs);
#define PSN_ST_LAUNCH(NT, EPT, E, OCC)                                                              \
    if (nt == NT && ept == EPT && e == E && occ == OCC) {                                           \
        hipLaunchKernelGGL((lk_kernel_st<NT, EPT, E, OCC>), grid, dim3(NT), lds_bytes, s, a);       \
        return hipGetLastError();                                                                   \
    }
    PSN_ST_KERNELS(PSN_ST_LAUNCH)
#undef PSN_ST_LAUNCH
    return hipErrorInvalidValue;
}

hipError_t st_kernels_init() {
#define PSN_ST_FN(NT, EPT, E, OCC) (const void *)lk_kernel_st<NT, EPT, E, OCC>,
    const void *fns[] = {PSN_ST_KERNELS(PSN_ST_FN)};
#undef PSN_ST_FN
    for (const void *f : fns) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace psn
