// The per-point solver arithmetic of LKTrackerInvoker (OpenCV 2.4.6), once.
//
// This header is the ONE place that restates the invoker's scalar float steps;
// every LK kernel (lk_kernel in psn_lk_kernels.hip, lk_kernel_st in psn_lk_st.hip,
// lk_kernel_bx in psn_lk_bx.hip, lk_kernel_lg in psn_lk_large.hip) calls it and differs only in how the sums
// are produced and where the window lives. The bit-exactness of every GPU test
// against the oracle rests on these lines; oracle/lk_oracle.c pins them
// (minEig at :725, the D test at :729).
//
// Every function is pure arithmetic: no barriers, no LDS, no control flow out
// of the caller's loops, no stamps. The __f*_rn / __d*_rn calls keep each
// operation separately rounded whatever the build's contraction flags.
// Internal, not installed.
#pragma once

#include <float.h>

namespace psn {

// FLT_SCALE of the invoker: applied to the raw A sums and to b1 / b2.
constexpr float kFltScale = 1.f / (1 << 20);

// The window at integer top-left (ix, iy) has left the level's image
// (cols x rows) by more than its own size: the point is lost at this level.
// (returns int, not bool: as a bool function the compiler folds the four tests
// differently from the in-place `||` chain and every LK kernel gains VGPRs)
__device__ __forceinline__ int win_outside(int ix, int iy, int w, int h, int cols, int rows) {
    return (ix < -w || ix >= cols || iy < -h || iy >= rows) ? 1 : 0;
}

// The staged J region (origin jr_x0, jr_y0; JRW x JRH) still covers the
// (w + 1) x (h + 1) pixels the bilinear window at (ix, iy) reads.
__device__ __forceinline__ bool jr_covers(int ix, int iy, int w, int h, int jr_x0, int jr_y0, int JRW, int JRH) {
    return ix >= jr_x0 && iy >= jr_y0 && ix + w + 1 <= jr_x0 + JRW && iy + h + 1 <= jr_y0 + JRH;
}

// The guess a level starts from: at the coarsest level the initial flow (or the
// previous point) scaled to it, below it twice the level above's result.
struct Guess {
    float x, y;
};
__device__ __forceinline__ Guess level_guess(int level, int maxL, int flags, float px0, float py0, float NPx, float NPy) {
    Guess gs;
    const float scale = ldexpf(1.f, -level);
    if (level == maxL) {
        if (flags & PSN_LK_USE_INITIAL_FLOW) {
            gs.x = __fmul_rn(NPx, scale);
            gs.y = __fmul_rn(NPy, scale);
        } else {
            gs.x = __fmul_rn(px0, scale);
            gs.y = __fmul_rn(py0, scale);
        }
    } else {
        gs.x = __fmul_rn(NPx, 2.f);
        gs.y = __fmul_rn(NPy, 2.f);
    }
    return gs;
}

// SSE2-order combination of the 5 ordered chain sums of A sum s (chains
// 5s..5s+3 the lanes of the __m128 accumulator, 5s+4 the scalar tail):
// tail + (((q0 + q1) + q2) + q3); the scalar build has the tail chain only.
// get(i) returns chain i.
template <typename Get>
__device__ __forceinline__ float combine_a5(Get get, int s, bool sse) {
    float t = get(5 * s + 4);
    if (sse) t = __fadd_rn(t, __fadd_rn(__fadd_rn(__fadd_rn(get(5 * s), get(5 * s + 1)), get(5 * s + 2)), get(5 * s + 3)));
    return t;
}

// The same for the 10 b chains (0-3 the lanes of b1's two accumulators, 4 its
// tail; 5-9 b2's): bbuf = qb0 + qb1; b1 += bbuf[0] + bbuf[2]; b2 += bbuf[1] + bbuf[3].
template <typename Get>
__device__ __forceinline__ void combine_b10(Get get, bool sse, float &b1, float &b2) {
    b1 = get(4);
    b2 = get(9);
    if (sse) {
        const float bb0 = __fadd_rn(get(0), get(2));
        const float bb2 = __fadd_rn(get(1), get(3));
        const float bb1 = __fadd_rn(get(5), get(7));
        const float bb3 = __fadd_rn(get(6), get(8));
        b1 = __fadd_rn(b1, __fadd_rn(bb0, bb2));
        b2 = __fadd_rn(b2, __fadd_rn(bb1, bb3));
    }
}

// Structure tensor of one level from the three raw float sums: the scaled
// A11, A12, A22, the minimum eigenvalue per window pixel, the reject test
// (minEig < minEigThreshold || D < FLT_EPSILON) and 1 / D (of use when ok).
struct LkSolve {
    float A11, A12, A22, invD, minEig;
    bool ok;
};
__device__ __forceinline__ LkSolve lk_solve(float s11, float s12, float s22, int wh, float min_eig) {
    LkSolve r;
    r.A11 = __fmul_rn(s11, kFltScale);
    r.A12 = __fmul_rn(s12, kFltScale);
    r.A22 = __fmul_rn(s22, kFltScale);
    const float D = __fsub_rn(__fmul_rn(r.A11, r.A22), __fmul_rn(r.A12, r.A12));
    const float dd = __fsub_rn(r.A11, r.A22);
    const float t = __fadd_rn(__fmul_rn(dd, dd), __fmul_rn(__fmul_rn(4.f, r.A12), r.A12));
    r.minEig = __fdiv_rn(__fsub_rn(__fadd_rn(r.A22, r.A11), sqrtf(t)), (float)(2 * wh));
    r.ok = !(r.minEig < min_eig || D < FLT_EPSILON);
    r.invD = __fdiv_rn(1.f, D);
    return r;
}

// One iteration's update from the raw b sums: delta = A^-1 b (b scaled by
// FLT_SCALE), the window corner (nx, ny) and the point NP = n + halfWin
// advance by it. Returns |delta|^2 as the invoker's double.
__device__ __forceinline__ double lk_update(float A11, float A12, float A22, float invD, float b1, float b2, float hwx,
                                            float hwy, float &nx, float &ny, float &NPx, float &NPy, float &dx,
                                            float &dy) {
    b1 = __fmul_rn(b1, kFltScale);
    b2 = __fmul_rn(b2, kFltScale);
    dx = __fmul_rn(__fsub_rn(__fmul_rn(A12, b2), __fmul_rn(A22, b1)), invD);
    dy = __fmul_rn(__fsub_rn(__fmul_rn(A12, b1), __fmul_rn(A11, b2)), invD);
    nx = __fadd_rn(nx, dx);
    ny = __fadd_rn(ny, dy);
    NPx = __fadd_rn(nx, hwx);
    NPy = __fadd_rn(ny, hwy);
    return __dadd_rn(__dmul_rn((double)dx, (double)dx), __dmul_rn((double)dy, (double)dy));
}

// End of the iterations: converged (|delta|^2 <= epsilon^2), or iteration j
// undid the previous one (the point oscillates: it takes half the step back).
// Otherwise the step becomes the previous one.
__device__ __forceinline__ bool lk_stop(double dd, double eps2, int j, float dx, float dy, float &pdx, float &pdy,
                                        float &NPx, float &NPy) {
    if (dd <= eps2) return true;
    if (j > 0 && (double)fabsf(__fadd_rn(dx, pdx)) < 0.01 && (double)fabsf(__fadd_rn(dy, pdy)) < 0.01) {
        NPx = __fsub_rn(NPx, __fmul_rn(dx, 0.5f));
        NPy = __fsub_rn(NPy, __fmul_rn(dy, 0.5f));
        return true;
    }
    pdx = dx;
    pdy = dy;
    return false;
}

// err of a tracked point: the sum of |J - I| over the window, per pixel, in
// the units of the 5 fractional bits of the interpolated values.
__device__ __forceinline__ float lk_err(float errval, int wh) {
    return __fdiv_rn(__fmul_rn(errval, 1.f), (float)(32 * wh));
}

}  // namespace psn
