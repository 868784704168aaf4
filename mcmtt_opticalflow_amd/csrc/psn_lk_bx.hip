// The box-window LK kernel of libpsn_lk.so (gfx950): lk_kernel_bx and its forward
// entry lk_kernel_fw, their instantiation lists PSN_BX_KERNELS / PSN_FW_KERNELS,
// launch_lk_bx and bx_kernels_init. The kernel body is psn_lk_bx_body.inc, its
// device helpers are in psn_lk_bx.h (shared with psn_lk_large.hip).
//
// lk_kernel_bx -- box windows (Tracker2D: (int)box.w x (int)box.w backward,
// PSNWhere_Tracker2D.cpp:776-782; box w x h forward, :871-877) above the
// single-tile kernel's size. Workgroup = one point, 4 waves (2 in the two-wave
// build, NT = kBxNT2). The window is cut
// into units of 4 pixels (row y, quad q) in row-major order and thread t owns
// the CONTIGUOUS units [t*UPT, t*UPT + UPT): for every SSE2 lane chain (x & 3,
// pixels below the 8- resp. 4-pixel-step bound) and the scalar tail chain the
// thread's terms are one contiguous run of the chain, in chain order. Window
// values (256 - 512 I, Ix, Iy) stay in registers for the whole level; the I
// patch and the J region are LDS bytes (J pairs for the packed-dot bilinear are
// formed with v_perm from two dwords per row).
// Exactness of every float sum (A11, A12, A22 per level; b1, b2 per iteration),
// decided per chain: a run's total and its maximum / minimum prefix go through
// a block scan (DPP within a wave, one LDS record per wave, ONE barrier); when
// every prefix of every chain is an integer of magnitude <= 2^24 and every term
// is exact, each chain's float sum IS its integer sum and the chains combine in
// float in the SSE2 build's order. Otherwise the ordered float chains: terms
// chain-major into LDS planes, row tile by row tile, one lane per chain.
#include <type_traits>

#include "psn_lk_bx.h"

namespace psn {

// Diagnostic phase clocks (PSN_LK_STAMPS, psn_lk_stamps.h; thread 0's view):
// accumulated s_memtime ticks per phase in bx_acc, written as stamps[wg][0..15]
// at the end. stamps[wg][19..30]: per fallback tile, the chain lane's time split
// (tools/bx_stamps.py) -- A fallback 19 its wave's next-tile write, 20 geometry +
// pad, 21 chain sums, 22 barrier wait, 23 tiles, 24 first-block wait (inside 21);
// b fallback, flag loop 25 flag wait, 26 geometry + pad, 27 chain sums, 28 tiles;
// barrier loop 29 chain sums (inside 12); 30 first-block wait of either loop;
// 31 / 32 the flag wait and the count of the FIRST tile of each flag-loop pass
// (inside 25 / 28). stamps[wg][33]: the err pass of level 0, from after its bounds
// re-check to the end (0 when it did not run: no err, PSN_LK_ERR_STATUS_ONLY).
// NT: the workgroup size. kBxNT2 is the two-wave build (QT below): the same
// kernel with two waves' records, err partials and staging strides, and fallback
// tiles of a quarter wave (kBxTile2 threads), each written by its whole wave.
//
// The body (psn_lk_bx_body.inc) has two kernel entries. POL picks, at compile
// time, where the entries differ: BxBasePolicy is lk_kernel_bx, whose
// <4 / 8 / 10, true> builds are held to their register counts; BxFwPolicy is
// lk_kernel_fw, the forward windows' entry, which is free to move.
struct BxBasePolicy {
    // the half-wave tile writers (writeA_nt, write_tile_nt) take the division-free
    // tile geometry of the no-tail builds
    static constexpr bool kShortWriterGeo = false;
    // PSN_LK_ERR_STATUS_ONLY ends level 0 after the bounds re-check (no err pass).
    // Off here: the pinned builds keep their code; the two-wave build takes the
    // flag through its own condition (QT in the body)
    static constexpr bool kErrStatusOnly = false;
    // the chain lanes' tile step (chain_sum_nt, psn_lk_bx.h): full no-tail tiles
    // summed by the straight-line chain_sum_nt with the tile geometry taken once
    // per fallback. Off here: the pinned builds and the two-wave build keep
    // chain_sum_pl and their loops
    static constexpr bool kChainNT = false;
};
struct BxFwPolicy {
    static constexpr bool kShortWriterGeo = true;
    static constexpr bool kErrStatusOnly = true;
    static constexpr bool kChainNT = true;
};

template <int UPT, bool NOTAIL, int NT = kBxNT>
__global__ __launch_bounds__(NT, bx_waves_per_simd(UPT, NOTAIL, NT)) void lk_kernel_bx(LkLaunchArgs A) {
    using POL = BxBasePolicy;
#include "psn_lk_bx_body.inc"
}

// The forward windows' entry (Tracker2D's box w x h, 64 x 160 at 1080p): the same
// body, launch bounds and LDS plan as lk_kernel_bx<UPT, NOTAIL, NT> under
// BxFwPolicy. Its name keeps it out of the lk_kernel_bx family, whose register
// counts are pinned.
template <int UPT, bool NOTAIL, int NT = kBxNT>
__global__ __launch_bounds__(NT, bx_waves_per_simd(UPT, NOTAIL, NT)) void lk_kernel_fw(LkLaunchArgs A) {
    using POL = BxFwPolicy;
#include "psn_lk_bx_body.inc"
}

// The instantiations of lk_kernel_bx, written ONCE: the launch dispatch and the
// dynamic-LDS attribute loop of bx_kernels_init are both generated from this
// list, so a variant cannot launch without its attribute.
// X(UPT units per thread, NOTAIL, NT workgroup size).
#define PSN_BX_KERNELS(X)                                                              \
    X(4, true, kBxNT) X(4, false, kBxNT) X(8, true, kBxNT) X(8, false, kBxNT)          \
    X(10, true, kBxNT) X(10, false, kBxNT) X(12, true, kBxNT) X(12, false, kBxNT)      \
    X(16, true, kBxNT) X(16, false, kBxNT) X(kBxUPT2, true, kBxNT2)
// ... and of lk_kernel_fw (the same fields): the build the planner's forward
// entry stands in for (kBxFwUPT).
#define PSN_FW_KERNELS(X) X(kBxFwUPT, true, kBxNT)

hipError_t launch_lk_bx(const LkLaunchArgs &a0, int total_wgs, int upt, bool notail, int nt, bool fw, int planned_lds,
                        bool pack, hipStream_t s) {
    if (total_wgs <= 0) return hipSuccess;
    const dim3 grid(total_wgs);
    // The request in CU slots (psn_lk_kernels.h): the kernels lay their window out
    // from its size alone, so the bytes past the plan are never touched -- POISON_LDS
    // fills them too, which is how the tests hold that.
    const int lds_bytes = bx_lds_request(planned_lds, nt, fw, pack);
    LkLaunchArgs a = a0;
    if (a.poison_lds) a.poison_lds = lds_bytes;
#define PSN_BX_LAUNCH(U, NOTAIL, NT)                                                            \
    if (!fw && upt == U && notail == NOTAIL && nt == NT) {                                      \
        hipLaunchKernelGGL((lk_kernel_bx<U, NOTAIL, NT>), grid, dim3(NT), lds_bytes, s, a);     \
        return hipGetLastError();                                                               \
    }
    PSN_BX_KERNELS(PSN_BX_LAUNCH)
#undef PSN_BX_LAUNCH
#define PSN_FW_LAUNCH(U, NOTAIL, NT)                                                            \
    if (fw && upt == U && notail == NOTAIL && nt == NT) {                                       \
        hipLaunchKernelGGL((lk_kernel_fw<U, NOTAIL, NT>), grid, dim3(NT), lds_bytes, s, a);     \
        return hipGetLastError();                                                               \
    }
    PSN_FW_KERNELS(PSN_FW_LAUNCH)
#undef PSN_FW_LAUNCH
    return hipErrorInvalidValue;  // (a missing instantiation is an error, never another kernel)
}

hipError_t bx_kernels_init() {
#define PSN_BX_FN(U, NOTAIL, NT) (const void *)lk_kernel_bx<U, NOTAIL, NT>,
#define PSN_FW_FN(U, NOTAIL, NT) (const void *)lk_kernel_fw<U, NOTAIL, NT>,
    const void *fns[] = {PSN_BX_KERNELS(PSN_BX_FN) PSN_FW_KERNELS(PSN_FW_FN)};
#undef PSN_BX_FN
#undef PSN_FW_FN
    for (const void *f : fns) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace psn
