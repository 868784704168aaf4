// HIP kernels for gfx950 (CDNA4) of the Tracker2D pyramidal-LK path: the pyramid
// build and the tiled LK kernel, their launchers, and lk_kernels_init. The other
// kernel families have a translation unit each: psn_lk_st.hip (single-tile
// windows), psn_lk_bx.hip (box windows), psn_lk_large.hip (large windows).
//
//   pyramid_kernel  ingest (gray copy or BGR->gray) + all pyrDown levels of one
//                   frame in ONE launch: each workgroup owns a tile of the top
//                   level and recomputes its halo through the levels in LDS.
//                   Replaces cv::cvtColor/resize (PSNWhere_Tracker2D.cpp:257-262)
//                   and buildOpticalFlowPyramid inside every calcOpticalFlowPyrLK
//                   call (:776-782, :871-877).
//   lk_kernel       LKTrackerInvoker over all levels for one point per
//                   workgroup: I patch + Scharr + bilinear window staged in LDS,
//                   J window staged in LDS with a margin, per-iteration 2x2 solve.
//
// Numerics follow OpenCV 2.4.6 exactly (integer fixed-point bilinear, float
// normal equations). The float sums reproduce the SSE2 build's summation
// ORDER (4 lanes for A, 2x4 lanes for b, scalar tail): the per-pixel products
// are computed by all lanes in parallel into LDS, laid out "chain-major", and
// each SSE2 lane / tail chain is summed sequentially by one lane. The result is
// bit-identical to oracle/lk_oracle.c. MFMA is not used: the work is a batch of
// tiny 2x2 solves, not a contraction.
#include "psn_gridfast.h"
#include "psn_lk_bx.h"  // xcd_remap
#include "psn_lk_pyr.h"

namespace psn {

// ---------------------------------------------------------------------------
// Pyramid (one tile: pyr_tile, psn_lk_pyr.h)
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void pyramid_kernel(PyrBuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if (a.nlevels == 1) {  // single level: ingest only, 64x64 tiles
        const int W0 = a.lv[0].w, H0 = a.lv[0].h;
        const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 64;
        for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
            int gy = y0 + (idx >> 6), gx = x0 + (idx & 63);
            if (gy < H0 && gx < W0) a.lv[0].p[(size_t)gy * a.lv[0].pitch + gx] = load_src(a, gy, gx);
        }
        return;
    }
    // XCD-aware tile order (as lk_kernel_bx): runs of consecutive row-major tiles
    // share one XCD's L2, so the halo a tile re-reads of its neighbours is an L2 hit
    const int n = gridDim.x * gridDim.y, t = xcd_remap((int)(blockIdx.y * gridDim.x + blockIdx.x), n);
    pyr_tile<256>(a, t % gridDim.x, t / gridDim.x, smem);
}

void pyramid_grid(const PyrBuildArgs &a, int &tiles_x, int &tiles_y, int &lds_bytes) {
    const int top = a.nlevels - 1;
    if (top == 0) {
        tiles_x = (a.lv[0].w + 63) / 64;
        tiles_y = (a.lv[0].h + 63) / 64;
        lds_bytes = 0;
    } else {
        tiles_x = (a.lv[top].w + a.tile - 1) / a.tile;
        tiles_y = (a.lv[top].h + a.tile - 1) / a.tile;
        lds_bytes = pyr_lds_bytes(top, a.tile);
    }
}

hipError_t launch_pyramid(const PyrBuildArgs &a, hipStream_t s) {
    int tx, ty, lds;
    pyramid_grid(a, tx, ty, lds);
    hipLaunchKernelGGL(pyramid_kernel, dim3(tx, ty), dim3(256), lds, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Tiled LK kernel
// ---------------------------------------------------------------------------

template <int NT>
__global__ __launch_bounds__(NT) void lk_kernel(LkLaunchArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x;
    const int g = blockIdx.x;
    int qi = 0;
    while (qi + 1 < A.nq && g >= A.q[qi + 1].wg_begin) qi++;
    const LkQueryDev &Q = A.q[qi];
    const int pi = lk_query_point(Q, A.counts, A.count_stride, g);
    if (pi < 0) return;  // past the query's device count
    const int w = Q.win_w, h = Q.win_h;
    const int TR = Q.tile_rows;
    const int maxL = Q.max_level;
    const int flags = Q.flags;
    const bool sse = (flags & PSN_LK_ACCUM_SCALAR) == 0;
    const int JRW = lk_jreg_w(w), JRH = lk_jreg_h(h);
    const int PW = w + 3, DW = w + 1;

    int16_t *Iw = (int16_t *)smem;
    short2 *Dw = (short2 *)(smem + lk_off_dw(w, h));
    uint8_t *JR = smem + lk_off_jr(w, h);
    float *RED = (float *)(smem + lk_off_red(w, h));
    int *REDI = (int *)(RED + 48);  // 16 ints of block-reduce scratch
    uint8_t *Pimg = smem + lk_off_tile(w, h);
    short2 *Dg = (short2 *)(Pimg + lk_tile_pimg_bytes(w, TR));
    float *Prod = (float *)((uint8_t *)Dg + lk_tile_dg_bytes(w, TR));

    const float hwx = __fmul_rn((float)(w - 1), 0.5f), hwy = __fmul_rn((float)(h - 1), 0.5f);
    const float px0 = A.prev[2 * pi], py0 = A.prev[2 * pi + 1];
    float NPx = 0.f, NPy = 0.f;
    if (flags & PSN_LK_USE_INITIAL_FLOW) {
        NPx = A.next[2 * pi];
        NPy = A.next[2 * pi + 1];
    }
    int status = 1;
    float errv = 0.f;

    for (int level = maxL; level >= 0; level--) {
        const LevelDev I = A.slots[Q.prev_slot * kMaxLevels + level];
        const LevelDev J = A.slots[Q.next_slot * kMaxLevels + level];
        const int cols = I.w, rows = I.h;
        const float scale = ldexpf(1.f, -level);
        float px = __fmul_rn(px0, scale), py = __fmul_rn(py0, scale);
        float nx, ny;
        if (level == maxL) {
            if (flags & PSN_LK_USE_INITIAL_FLOW) {
                nx = __fmul_rn(NPx, scale);
                ny = __fmul_rn(NPy, scale);
            } else {
                nx = px;
                ny = py;
            }
        } else {
            nx = __fmul_rn(NPx, 2.f);
            ny = __fmul_rn(NPy, 2.f);
        }
        NPx = nx;
        NPy = ny;
        px = __fsub_rn(px, hwx);
        py = __fsub_rn(py, hwy);
        const int ipx = cv_floor(px), ipy = cv_floor(py);
        // (win_outside, written out at this kernel's three sites: through the helper the
        // compiler folds the tests differently and lk_kernel<256> changes its VGPR count)
        if (ipx < -w || ipx >= cols || ipy < -h || ipy >= rows) {
            if (level == 0) {
                status = 0;
                errv = 0.f;
            }
            continue;
        }
        int iw00, iw01, iw10, iw11;
        bilin_weights(__fsub_rn(px, (float)ipx), __fsub_rn(py, (float)ipy), iw00, iw01, iw10, iw11);

        // J region for the first iteration, fetched together with the I patch
        nx = __fsub_rn(nx, hwx);
        ny = __fsub_rn(ny, hwy);
        int jr_x0 = cv_floor(nx) - kJMargin, jr_y0 = cv_floor(ny) - kJMargin;
        bool jr_valid = false;

        // ---- A-phase: I window, Scharr, structure tensor ----
        int sA11 = 0, sA12 = 0;
        unsigned aA12 = 0, sA22 = 0;
        for (int r0 = 0; r0 < h; r0 += TR) {
            const int th = min(TR, h - r0);
            if (r0 > 0) __syncthreads();  // previous tile's Pimg/Dg readers are done
            if (r0 == 0) {
                stage_two<NT>(Pimg, I, ipy - 1, ipx - 1, PW, th + 3, JR, J, jr_y0, jr_x0, JRW, JRH);
                jr_valid = true;
            } else {
                stage_one<NT>(Pimg, I, ipy + r0 - 1, ipx - 1, PW, th + 3);
            }
            __syncthreads();
            {  // Scharr on (th+1) x (w+1) positions; zero outside the image
                Walk wk;
                wk.init(tid, NT, DW);
                for (int idx = tid; idx < (th + 1) * DW; idx += NT, wk.step()) {
                    const int yy = wk.y, xx = wk.x;
                    const int gy = ipy + r0 + yy, gx = ipx + xx;
                    short2 d = make_short2(0, 0);
                    if ((unsigned)gy < (unsigned)rows && (unsigned)gx < (unsigned)cols) {
                        const uint8_t *p = Pimg + yy * PW + xx;
                        const int v0l = 3 * (p[0] + p[2 * PW]) + 10 * p[PW];
                        const int v0r = 3 * (p[2] + p[2 * PW + 2]) + 10 * p[PW + 2];
                        const int v1l = p[2 * PW] - p[0];
                        const int v1c = p[2 * PW + 1] - p[1];
                        const int v1r = p[2 * PW + 2] - p[2];
                        d.x = (short)(v0r - v0l);
                        d.y = (short)(3 * (v1l + v1r) + 10 * v1c);
                    }
                    Dg[idx] = d;
                }
            }
            __syncthreads();
            {  // bilinear I / Ix / Iy window rows; integer structure-tensor sums
                Walk wk;
                wk.init(tid, NT, w);
                for (int idx = tid; idx < th * w; idx += NT, wk.step()) {
                    const int yl = wk.y, x = wk.x;
                    const uint8_t *p = Pimg + (yl + 1) * PW + x + 1;
                    const int ival = PSN_DESCALE(p[0] * iw00 + p[1] * iw01 + p[PW] * iw10 + p[PW + 1] * iw11, 9);
                    const short2 *d = Dg + yl * DW + x;
                    const int ixv = PSN_DESCALE(d[0].x * iw00 + d[1].x * iw01 + d[DW].x * iw10 + d[DW + 1].x * iw11, 14);
                    const int iyv = PSN_DESCALE(d[0].y * iw00 + d[1].y * iw01 + d[DW].y * iw10 + d[DW + 1].y * iw11, 14);
                    const int y = r0 + yl;
                    Iw[y * w + x] = (int16_t)ival;
                    Dw[y * w + x] = make_short2((short)ixv, (short)iyv);
                    const int xy = ixv * iyv;
                    sA11 = (int)sat_add((unsigned)sA11, (unsigned)(ixv * ixv));
                    sA12 += xy;
                    aA12 = sat_add(aA12, (unsigned)abs(xy));
                    sA22 = sat_add(sA22, (unsigned)(iyv * iyv));
                }
            }
        }
        __syncthreads();  // Iw / Dw complete
        block_reduce4<NT, true>(sA11, sA12, aA12, sA22, REDI);
        const bool ex11 = sA11 <= kExact, ex12 = aA12 <= (unsigned)kExact, ex22 = sA22 <= (unsigned)kExact;
        float r11 = (float)sA11, r12 = (float)sA12, r22 = (float)sA22;  // the raw A sums
        if (!(ex11 && ex12 && ex22)) {
            // ordered float chains over (float)(Ix*Ix), (float)(Ix*Iy), (float)(Iy*Iy)
            float acc = 0.f;
            for (int r0 = 0; r0 < h; r0 += TR) {
                const int th = min(TR, h - r0);
                const ChainA C(w, th, sse);
                if (r0 > 0) __syncthreads();
                Walk wk;
                wk.init(tid, NT, w);
                for (int idx = tid; idx < th * w; idx += NT, wk.step()) {
                    const short2 d = Dw[(r0 + wk.y) * w + wk.x];
                    const int pos = C.pos(wk.y, wk.x);
                    Prod[pos] = (float)(d.x * d.x);
                    Prod[C.P + pos] = (float)(d.x * d.y);
                    Prod[2 * C.P + pos] = (float)(d.y * d.y);
                }
                __syncthreads();
                if (tid < 15) {
                    const int ch = tid % 5, s = tid / 5;
                    const int base = ch < 4 ? ch * C.SA : 4 * C.SA;
                    const int len = ch < 4 ? th * C.nA : th * C.tA;
                    acc = chain_sum(Prod + s * C.P + base, len, acc);
                }
            }
            if (tid < 15) RED[tid] = acc;
            __syncthreads();
            float s3[3];
#pragma unroll
            for (int s = 0; s < 3; s++) s3[s] = combine_a5([&](int i) { return RED[i]; }, s, sse);
            if (!ex11) r11 = s3[0];
            if (!ex12) r12 = s3[1];
            if (!ex22) r22 = s3[2];
        }
        const LkSolve S = lk_solve(r11, r12, r22, w * h, Q.min_eig);
        if (flags & PSN_LK_GET_MIN_EIGENVALS) errv = S.minEig;
        if (!S.ok) {
            if (level == 0) status = 0;
            __syncthreads();
            continue;
        }
        float pdx = 0.f, pdy = 0.f;

        for (int j = 0; j < Q.max_count; j++) {
            const int inx = cv_floor(nx), iny = cv_floor(ny);
            if (inx < -w || inx >= cols || iny < -h || iny >= rows) {
                if (level == 0) status = 0;
                break;
            }
            bilin_weights(__fsub_rn(nx, (float)inx), __fsub_rn(ny, (float)iny), iw00, iw01, iw10, iw11);
            if (!(jr_valid && jr_covers(inx, iny, w, h, jr_x0, jr_y0, JRW, JRH))) {
                jr_x0 = inx - kJMargin;
                jr_y0 = iny - kJMargin;
                jr_valid = true;
                __syncthreads();
                stage_one<NT>(JR, J, jr_y0, jr_x0, JRW, JRH);
                __syncthreads();
            }
            const uint8_t *jb = JR + (iny - jr_y0) * JRW + (inx - jr_x0);
            int s1 = 0, s2 = 0;
            unsigned a1 = 0, a2 = 0;
            {
                Walk wk;
                wk.init(tid, NT, w);
                for (int idx = tid; idx < w * h; idx += NT, wk.step()) {
                    const uint8_t *p = jb + wk.y * JRW + wk.x;
                    const int jv = PSN_DESCALE(p[0] * iw00 + p[1] * iw01 + p[JRW] * iw10 + p[JRW + 1] * iw11, 9);
                    const int diff = jv - Iw[idx];
                    const short2 d = Dw[idx];
                    const int t1 = diff * d.x, t2 = diff * d.y;
                    s1 += t1;
                    s2 += t2;
                    a1 = sat_add(a1, (unsigned)abs(t1));
                    a2 = sat_add(a2, (unsigned)abs(t2));
                }
            }
            block_reduce4<NT, false>(s1, s2, a1, a2, REDI);
            float b1, b2;
            if (sums_exact(a1, s1) && sums_exact(a2, s2)) {  // subset-sum bound (see sums_exact)
                b1 = (float)s1;
                b2 = (float)s2;
            } else {
                float bacc = 0.f;
                for (int r0 = 0; r0 < h; r0 += TR) {
                    const int th = min(TR, h - r0);
                    const ChainB C(w, th, sse);
                    __syncthreads();  // chain lanes done with the previous tile / reduce scratch
                    Walk wk;
                    wk.init(tid, NT, w);
                    for (int idx = tid; idx < th * w; idx += NT, wk.step()) {
                        const int y = r0 + wk.y;
                        const uint8_t *p = jb + y * JRW + wk.x;
                        const int jv = PSN_DESCALE(p[0] * iw00 + p[1] * iw01 + p[JRW] * iw10 + p[JRW + 1] * iw11, 9);
                        const int diff = jv - Iw[y * w + wk.x];
                        const short2 d = Dw[y * w + wk.x];
                        const int pos = C.pos(wk.y, wk.x);
                        Prod[pos] = (float)(diff * d.x);
                        Prod[C.P + pos] = (float)(diff * d.y);
                    }
                    __syncthreads();
                    if (tid < 10) {
                        const int ch = tid % 5, s = tid / 5;
                        const int base = ch < 4 ? ch * C.SB : 4 * C.SB;
                        const int len = ch < 4 ? th * 2 * C.nB : th * C.tB;
                        bacc = chain_sum(Prod + s * C.P + base, len, bacc);
                    }
                }
                if (tid < 10) RED[16 + tid] = bacc;
                __syncthreads();
                combine_b10([&](int i) { return RED[16 + i]; }, sse, b1, b2);
                __syncthreads();  // RED read by all before any later write
            }
            float dx, dy;
            const double dd = lk_update(S.A11, S.A12, S.A22, S.invD, b1, b2, hwx, hwy, nx, ny, NPx, NPy, dx, dy);
            if (lk_stop(dd, Q.eps2, j, dx, dy, pdx, pdy, NPx, NPy)) break;
        }

        if (level == 0 && status && A.err && (flags & PSN_LK_GET_MIN_EIGENVALS) == 0) {
            const float qx = __fsub_rn(NPx, hwx), qy = __fsub_rn(NPy, hwy);
            const int iqx = cv_floor(qx), iqy = cv_floor(qy);
            if (iqx < -w || iqx >= cols || iqy < -h || iqy >= rows) {
                status = 0;
                __syncthreads();
                continue;
            }
            if (flags & PSN_LK_ERR_STATUS_ONLY) {  // the re-check was all: err[] = 0
                __syncthreads();
                continue;
            }
            bilin_weights(__fsub_rn(qx, (float)iqx), __fsub_rn(qy, (float)iqy), iw00, iw01, iw10, iw11);
            if (!(jr_valid && jr_covers(iqx, iqy, w, h, jr_x0, jr_y0, JRW, JRH))) {
                jr_x0 = iqx - kJMargin;
                jr_y0 = iqy - kJMargin;
                jr_valid = true;
                __syncthreads();
                stage_one<NT>(JR, J, jr_y0, jr_x0, JRW, JRH);
                __syncthreads();
            }
            const uint8_t *jb = JR + (iqy - jr_y0) * JRW + (iqx - jr_x0);
            int e0 = 0, e1 = 0;
            unsigned e2 = 0, e3 = 0;
            {
                Walk wk;
                wk.init(tid, NT, w);
                for (int idx = tid; idx < w * h; idx += NT, wk.step()) {
                    const uint8_t *p = jb + wk.y * JRW + wk.x;
                    const int jv = PSN_DESCALE(p[0] * iw00 + p[1] * iw01 + p[JRW] * iw10 + p[JRW + 1] * iw11, 9);
                    e2 = sat_add(e2, (unsigned)abs(jv - Iw[idx]));
                }
            }
            block_reduce4<NT, false>(e0, e1, e2, e3, REDI);
            float errval;
            if (e2 <= (unsigned)kExact) {
                // every partial sum of errval += |diff| is an integer <= 2^24: exact
                errval = (float)e2;
            } else {
                float eacc = 0.f;
                for (int r0 = 0; r0 < h; r0 += TR) {
                    const int th = min(TR, h - r0);
                    __syncthreads();
                    Walk wk;
                    wk.init(tid, NT, w);
                    for (int idx = tid; idx < th * w; idx += NT, wk.step()) {
                        const int y = r0 + wk.y;
                        const uint8_t *p = jb + y * JRW + wk.x;
                        const int jv = PSN_DESCALE(p[0] * iw00 + p[1] * iw01 + p[JRW] * iw10 + p[JRW + 1] * iw11, 9);
                        Prod[idx] = (float)abs(jv - Iw[y * w + wk.x]);
                    }
                    __syncthreads();
                    if (tid == 0) eacc = chain_sum(Prod, th * w, eacc);
                }
                if (tid == 0) RED[32] = eacc;
                __syncthreads();
                errval = RED[32];
            }
            errv = lk_err(errval, w * h);
        }
        __syncthreads();  // LDS reuse by the next level
    }

    if (tid == 0) {
        A.next[2 * pi] = NPx;
        A.next[2 * pi + 1] = NPy;
        A.status[pi] = (uint8_t)status;
        if (A.err) A.err[pi] = errv;
    }
}

hipError_t launch_lk(const LkLaunchArgs &a, int total_wgs, int threads, int lds_bytes, hipStream_t s) {
    if (total_wgs <= 0) return hipSuccess;
    const dim3 grid(total_wgs);
    switch (threads) {
        case 64: hipLaunchKernelGGL(lk_kernel<64>, grid, dim3(64), lds_bytes, s, a); break;
        case 128: hipLaunchKernelGGL(lk_kernel<128>, grid, dim3(128), lds_bytes, s, a); break;
        default: hipLaunchKernelGGL(lk_kernel<256>, grid, dim3(256), lds_bytes, s, a); break;
    }
    return hipGetLastError();
}

hipError_t lk_kernels_init() {
    const void *fns[] = {(const void *)lk_kernel<64>, (const void *)lk_kernel<128>, (const void *)lk_kernel<256>,
                         (const void *)pyramid_kernel};
    hipError_t e;
    for (const void *f : fns)
        if ((e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes)) != hipSuccess)
            return e;
    // the other families' lists live in their own units
    if ((e = st_kernels_init()) != hipSuccess) return e;
    if ((e = bx_kernels_init()) != hipSuccess) return e;
    if ((e = lg_kernels_init()) != hipSuccess) return e;
    return gridfast_kernels_init();
}

}  // namespace psn
