// lk_kernel_lg: LKTrackerInvoker (OpenCV 2.4.6, reached from
// PSNWhere_Tracker2D.cpp:776-782 backward and :871-877 forward) for the box
// windows the box kernel cannot hold in registers -- Tracker2D windows of any
// size (forward w x h, backward w x w; PETS-scale 100x250 at 1080p, 128x320 at
// 4K).
//
// The structure of lk_kernel_bx (psn_lk_bx.hip) with the window values
// streamed instead of register-resident. One workgroup (4 waves) per point, the
// grid striding over the launch's points. The window is cut into quads (row y,
// 4 pixels) in row-major order; thread t owns the CONTIGUOUS quads [t*K, t*K+K),
// so for every SSE2 lane chain and the scalar tail chain its terms form one
// contiguous run of the chain. Per level the A phase writes every quad's window
// values -- (I*, Ix*, Iy*) of 4 pixels as packed 16-bit pairs, 24 B -- into the
// workgroup's HBM slot (laid out [j][t], so thread t's j-th quads are one
// coalesced load), and every iteration streams them back (L2 / MALL resident)
// with the quad's J rows as two aligned dwords per row (packed-dot bilinear as
// in lk_kernel_bx). Exactness of each float sum per chain by the run records
// (total, maximum / minimum prefix) through one block scan; otherwise the
// ordered chains from the first inexact half wave on, over tiles of consecutive
// quads whose products are written chain-major into double-buffered LDS planes
// while wave 0's chain lanes sum the previous tile. LDS holds only the tiles
// (and, in the A phase, one row band of the I patch and its Scharr plane), so
// several workgroups share a CU and hide each other's serial chains.
//
// One helper per phase beside the kernel: lg_slot_index (the slot layout), lg_walk
// (A runs, main pass, err pass), lg_runs_exact (run records -> block check),
// lg_tiles / lg_store_quad / lg_ordered (ordered chains -> uniform result); the
// level's guess is level_guess (psn_lk_solve.h); instantiations: PSN_LG_KERNELS.
//
// Bit-identical to oracle/lk_oracle.c (the SSE2 build's summation order, or the
// scalar build's with PSN_LK_ACCUM_SCALAR).
#include "psn_lk_bx.h"

namespace psn {

// pair selector: bytes (s, s + 1) of a row's 8-byte window -> J[x] | J[x+1] << 16
__device__ __forceinline__ unsigned lg_sel(int s) { return 0x0c000c00u | ((unsigned)(s + 1) << 16) | (unsigned)s; }

// Window geometry: quads per row, quads, quads per thread; the SSE2 chain split
// of the b sums (8-pixel steps: nB2 quads per row, n8 pixels, tB tail pixels)
// and of the A sums (4-pixel steps: nA quads, tA tail pixels).
struct LgGeo {
    int w, h, QW, NQ, K;
    int nB2, n8, tB, nA, tA;
    float rQW, rK;  // 1 / QW, 1 / K (lg_div)
};
// n / d for 0 <= n < 2^24 (quad indices; the planner keeps windows below 2^22
// quads) by the float reciprocal r = 1 / d and one correction step
__device__ __forceinline__ int lg_div(int n, int d, float r) {
    int t = (int)__fmul_rn((float)n, r);
    const int m = n - t * d;
    t += m < 0 ? -1 : (m >= d ? 1 : 0);
    return t;
}
__device__ __forceinline__ LgGeo lg_geo(int w, int h, bool sse) {
    LgGeo g;
    g.w = w;
    g.h = h;
    g.QW = (w + 3) >> 2;
    g.NQ = h * g.QW;
    g.K = (g.NQ + kLgNT - 1) / kLgNT;
    g.nB2 = sse ? 2 * (w / 8) : 0;
    g.n8 = 4 * g.nB2;
    g.tB = w - g.n8;
    g.nA = sse ? w / 4 : 0;
    g.tA = w - 4 * g.nA;
    g.rQW = __fdiv_rn(1.f, (float)g.QW);
    g.rK = __fdiv_rn(1.f, (float)g.K);
    return g;
}
// row y and quad column qx of quad q
struct LgRC {
    int y, qx;
};
__device__ __forceinline__ LgRC lg_rc(const LgGeo &g, int q) {
    const int y = lg_div(q, g.QW, g.rQW);
    return {y, q - y * g.QW};
}
// terms of the SSE chains (one per SSE quad) and of the tail chain before quad q
__device__ __forceinline__ int lg_sse_before(const LgGeo &g, int q, int nS) {
    const LgRC r = lg_rc(g, q);
    return r.y * nS + min(r.qx, nS);
}
__device__ __forceinline__ int lg_tail_before(const LgGeo &g, int q, int nS, int t) {
    const LgRC r = lg_rc(g, q);
    return r.y * t + min(max(4 * (r.qx - nS), 0), t);
}

// The workgroup's HBM slot: the window values of every quad, three planes (I*,
// Ix*, Iy*; 4 pixels as packed 16-bit pairs) laid out [j][t]: quad q = t * K + j
// (thread t's j-th) at j * NT + t, so the j-th quads of a wave are one coalesced load.
struct LgSlot {
    uint2 *ip, *xp, *yp;
};
__device__ __forceinline__ int lg_slot_index(const LgGeo &g, int q) {
    const int t = lg_div(q, g.K, g.rK);
    return (q - t * g.K) * kLgNT + t;
}
// One quad's window values; a pass loads the planes it reads (LI, LX, LY).
struct LgQ {
    uint2 ip, xp, yp;
};
template <bool LI, bool LX, bool LY>
__device__ __forceinline__ LgQ lg_load(const LgSlot &S, int idx) {
    LgQ v{};
    if constexpr (LI) v.ip = S.ip[idx];
    if constexpr (LX) v.xp = S.xp[idx];
    if constexpr (LY) v.yp = S.yp[idx];
    return v;
}
// the 4 pixels of a packed plane value
__device__ __forceinline__ void lg_unpack4(const uint2 &p, int (&v)[4]) {
    v[0] = lo16(p.x), v[1] = hi16(p.x), v[2] = lo16(p.y), v[3] = hi16(p.y);
}

// One quad's J - I* (4 pixels) at window row y, quad column qx: from the LDS copy
// of the J region (lds), or from the level (in: every tap inside it).
struct LgJ {
    const uint32_t *jl;  // lds: the region's dword holding the window origin
    const uint8_t *jb;   // in: J at the window origin aligned down to a dword
    LevelDev J;
    int inx, iny, pitch, jrp4;
    unsigned W0, W1, s[4];
    int w00, w01, w10, w11;
    bool lds, in;
};
__device__ __forceinline__ LgJ lg_j(const LevelDev &J, int inx, int iny, int w, int h, int w00, int w01, int w10,
                                    int w11, const uint32_t *jr, int jrp4, int jr_x0, int jr_y0) {
    LgJ r;
    r.J = J;
    r.inx = inx;
    r.iny = iny;
    r.pitch = J.pitch;
    r.jrp4 = jrp4;
    r.w00 = w00;
    r.w01 = w01;
    r.w10 = w10;
    r.w11 = w11;
    r.W0 = pack_w(w00, w01);
    r.W1 = pack_w(w10, w11);
    r.lds = jr != nullptr;
    // every tap of the window (columns inx .. inx + w, rows iny .. iny + h) inside the level
    r.in = inx >= 0 && iny >= 0 && inx + w + 1 <= J.w && iny + h + 1 <= J.h;
    int sh = r.in ? (inx & 3) : 0;
    if (r.lds) {
        const int ox = inx - jr_x0;
        sh = ox & 3;
        r.jl = jr + (iny - jr_y0) * jrp4 + (ox >> 2);
    } else {
        r.jl = nullptr;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) r.s[i] = lg_sel(sh + i);
    r.jb = r.in ? J.p + (long long)iny * J.pitch + (inx - sh) : J.p;
    return r;
}
// d[i] = DESCALE(bilinear J, 9) - I of the quad's pixels (ip: I* as packed pairs);
// the diff is folded into the dot product's accumulator: (v + 256 - 512 I) >> 9.
// Taps outside the level take their reflect-101 source (the padded J buffer of
// calcOpticalFlowPyrLK: copyMakeBorder(..., BORDER_REFLECT_101)); the LDS copy
// holds them already (dma_patch).
__device__ __forceinline__ void lg_diffs(const LgJ &J, int y, int qx, const uint2 &ip, int (&d)[4]) {
    int I[4];
    lg_unpack4(ip, I);
    if (J.lds || J.in) {
        uint32_t a0, a1, b0, b1;
        if (J.lds) {
            const uint32_t *r0 = J.jl + y * J.jrp4 + qx;
            a0 = r0[0];
            a1 = r0[1];
            b0 = r0[J.jrp4];
            b1 = r0[J.jrp4 + 1];
        } else {
            const uint32_t *r0 = (const uint32_t *)(J.jb + (long long)y * J.pitch + 4 * qx);
            const uint32_t *r1 = (const uint32_t *)((const uint8_t *)r0 + J.pitch);
            a0 = r0[0];
            a1 = r0[1];
            b0 = r1[0];
            b1 = r1[1];
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
            d[i] = sdot2(__builtin_amdgcn_perm(b1, b0, J.s[i]), J.W1,
                         sdot2(__builtin_amdgcn_perm(a1, a0, J.s[i]), J.W0, 256 - 512 * I[i])) >> 9;
    } else {  // a window reaching past the level: reflect-101 taps, pixel by pixel
        const uint8_t *r0 = J.J.p + (long long)refl101(J.iny + y, J.J.h) * J.pitch;
        const uint8_t *r1 = J.J.p + (long long)refl101(J.iny + y + 1, J.J.h) * J.pitch;
#pragma unroll 1
        for (int i = 0; i < 4; i++) {
            const int xa = refl101(J.inx + 4 * qx + i, J.J.w), xb = refl101(J.inx + 4 * qx + i + 1, J.J.w);
            d[i] = PSN_DESCALE(r0[xa] * J.w00 + r0[xb] * J.w01 + r1[xa] * J.w10 + r1[xb] * J.w11, 9) - I[i];
        }
    }
}

// LDS tile planes of the ordered-chain fallbacks (psn_lk_kernels.h): per plane 4
// SSE chain regions of up to TQ terms and a tail region of up to 4*TQ terms
// (16-float blocks + 4: conflict-free across the chain lanes' 16-B reads)

// Ordered chains from quad qs on, tile by tile: waves 1-3 write a tile's products
// (one quad per thread: `load(q)` fetches quad q's window values, `store(v, q,
// tile start, buffer)` writes its products), chain lanes (wave 0, lanes < NCH)
// sum the previous tile meanwhile; double-buffered, one barrier per tile, each
// writer's loads for tile g+2 in flight while tile g is summed. `before(q, s, t)`
// gives the SSE / tail chain terms before quad q (uniform); a chain lane zeroes
// the 16-float block holding the end of its region for tile g+2 right after
// summing tile g from the same buffer (the writers fill the block's front a
// barrier later). Returns acc (chain lanes: their chain's sum onto its base).
template <int NPL, int TQ, typename Load, typename Store, typename Before, typename Mark>
__device__ __forceinline__ float lg_tiles(int qs, int NQ, float *buf, int nch, float acc, Load load, Store store,
                                          Before before, Mark mark) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int PL = lg_plane(TQ), SR = lg_sreg(TQ);
    const bool chl = tid < nch;
    const int cs = lane / 5, cc = lane - 5 * cs;
    const int ntiles = (NQ - qs + TQ - 1) / TQ;
    if (ntiles <= 0) return acc;
    auto region = [&](float *b) { return b + cs * PL + (cc < 4 ? cc * SR : 4 * SR); };
    // chain terms before tile boundaries g .. g+3 (uniform), rolled per tile
    int bs[4], bt[4];
#pragma unroll
    for (int i = 0; i < 4; i++) before(min(qs + i * TQ, NQ), bs[i], bt[i]);
    auto pad = [&](int i0, float *b) {  // the tile between boundaries i0, i0 + 1
        if (!chl) return;
        const int len = cc < 4 ? bs[i0 + 1] - bs[i0] : bt[i0 + 1] - bt[i0];
        if (len & 15) {
            float4 *z = (float4 *)(region(b) + (len & ~15));
            const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
            z[0] = zero;
            z[1] = zero;
            z[2] = zero;
            z[3] = zero;
        }
    };
    // writer thread tid (waves 1-3) takes quad tid - 64 of each tile
    auto quad_of = [&](int g) { return tid >= 64 && tid - 64 < TQ ? qs + g * TQ + tid - 64 : NQ; };
    pad(0, buf);
    if (ntiles > 1) pad(1, buf + NPL * PL);
    __syncthreads();
    LgQ v{};
    int q = quad_of(0);
    if (q < NQ) store(load(q), q, qs, buf);
    q = quad_of(1);
    if (q < NQ) v = load(q);
    __syncthreads();
    for (int g = 0; g < ntiles; g++) {
        float *cur = buf + (g & 1) * NPL * PL, *nxt = buf + ((g + 1) & 1) * NPL * PL;
        if (g + 1 < ntiles) {
            if (q < NQ) store(v, q, qs + (g + 1) * TQ, nxt);
            q = quad_of(g + 2);
            if (q < NQ) v = load(q);
        }
        if (tid < 64) {
            const int ns = bs[1] - bs[0], nt = bt[1] - bt[0];
            const int len = chl ? (cc < 4 ? ns : nt) : 0;
            const int nbmax = (max(ns, nt) + 15) >> 4;
            mark(2);
            if (chl) acc = chain_sum_pl<false>(region(cur), len, nbmax, acc);
            mark(3);
            if (g + 2 < ntiles) pad(2, cur);
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            bs[i] = bs[i + 1];
            bt[i] = bt[i + 1];
        }
        before(min(qs + (g + 4) * TQ, NQ), bs[3], bt[3]);
        mark(0);
        __syncthreads();
        mark(1);
    }
    return acc;
}

// The fallback tile writer (lg_tiles' `store`): quad q's terms of NPL sums into the
// tile starting at quad a, planes at buf. Chains split at quad column nS: pixel i
// of an SSE2 quad is a term of lane chain i, the pixels of the later quads are
// tail chain terms in order (tT per row, cut at the window's width). term(i, t)
// gives pixel i's NPL terms.
template <int NPL, int TQ, typename Term>
__device__ __forceinline__ void lg_store_quad(const LgGeo &G, int nS, int tT, int q, int qx, int a, float *buf,
                                              Term term) {
    constexpr int PLN = lg_plane(TQ), SR = lg_sreg(TQ);
    auto put = [&](float *p, int i) {
        float t[NPL];
        term(i, t);
#pragma unroll
        for (int s = 0; s < NPL; s++) p[s * PLN] = t[s];
    };
    if (qx < nS) {
        const int pos = lg_sse_before(G, q, nS) - lg_sse_before(G, a, nS);
#pragma unroll
        for (int i = 0; i < 4; i++) put(buf + i * SR + pos, i);
    } else {
        const int pos = lg_tail_before(G, q, nS, tT) - lg_tail_before(G, a, nS, tT);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (4 * qx + i >= G.w) break;
            put(buf + 4 * SR + pos + i, i);
        }
    }
}

// Ordered chains to a uniform result: the 5 * NPL chains of NPL sums (3: A11,
// A12, A22; 2: b1, b2) from quad qs on, chain lanes starting from `base`
// (lg_tiles over the planes at PL); wave 0 combines its chain lanes in the SSE2
// build's order and all threads read r[] back from RS[0 .. NPL) after one
// barrier. The writers load the X and Y planes (and I with LI); terms(v, y, qx)
// returns the per-pixel term callable of a quad (lg_store_quad). mark(0 .. 3) as
// in lg_tiles, mark(4) once the tiles are summed.
template <int NPL, int TQ, bool LI, typename Terms, typename Mark>
__device__ __forceinline__ void lg_ordered(const LgGeo &G, int nS, int tT, const LgSlot &S, int qs, float base,
                                           float *PL, float *RS, bool sse, Terms terms, Mark mark, float (&r)[NPL]) {
    static_assert(NPL == 2 || NPL == 3, "b1, b2 or A11, A12, A22");
    auto before = [&](int q, int &bs, int &bt) {
        bs = lg_sse_before(G, q, nS);
        bt = lg_tail_before(G, q, nS, tT);
    };
    auto load = [&](int q) { return lg_load<LI, true, true>(S, lg_slot_index(G, q)); };
    auto store = [&](const LgQ &v, int q, int a, float *buf) {
        const LgRC rc = lg_rc(G, q);
        lg_store_quad<NPL, TQ>(G, nS, tT, q, rc.qx, a, buf, terms(v, rc.y, rc.qx));
    };
    const float acc = lg_tiles<NPL, TQ>(qs, G.NQ, PL, 5 * NPL, base, load, store, before, mark);
    mark(4);
    if (threadIdx.x < 64) {  // wave 0 combines in the SSE2 build's order
        auto chain = [&](int i) { return readlane_f(acc, i); };
        float t[NPL];
        if constexpr (NPL == 3) {
#pragma unroll
            for (int s = 0; s < 3; s++) t[s] = combine_a5(chain, s, sse);
        } else {
            combine_b10(chain, sse, t[0], t[1]);
        }
        if (threadIdx.x == 0) {
#pragma unroll
            for (int s = 0; s < NPL; s++) RS[s] = t[s];
        }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NPL; s++) r[s] = RS[s];
}

// The walk over a thread's quads [q0, q0 + cnt), q0 at row y0, quad column x0, in
// order: body(v, y, qx) per quad with the planes LI / LX / LY of its window
// values. Batches of kLgMB quads have their slot loads in flight together.
constexpr int kLgMB = 4;
template <bool LI, bool LX, bool LY, typename Body>
__device__ __forceinline__ void lg_walk(const LgSlot &S, int cnt, int y0, int x0, int QW, Body body) {
    const int tid = threadIdx.x;
    int y = y0, qx = x0;
    auto quad = [&](const LgQ &v) {
        body(v, y, qx);
        if (++qx == QW) {
            qx = 0;
            y++;
        }
    };
    int k = 0;
    for (; k + kLgMB <= cnt; k += kLgMB) {
        // (one array per plane, not LgQ[kLgMB]: from an array of structs the compiler
        // issues the loads plane-major and the third quad waits for the whole batch,
        // s_waitcnt vmcnt 11, 7, 4, 0 in place of 11, 7, 6, 5, 3, 2, 0)
        uint2 ip[kLgMB] = {}, xp[kLgMB] = {}, yp[kLgMB] = {};
#pragma unroll
        for (int u = 0; u < kLgMB; u++) {
            const int ix = (k + u) * kLgNT + tid;
            if constexpr (LI) ip[u] = S.ip[ix];
            if constexpr (LX) xp[u] = S.xp[ix];
            if constexpr (LY) yp[u] = S.yp[ix];
        }
#pragma unroll
        for (int u = 0; u < kLgMB; u++) quad(LgQ{ip[u], xp[u], yp[u]});
    }
    for (; k < cnt; k++) quad(lg_load<LI, LX, LY>(S, k * kLgNT + tid));
}

// The block's exactness check of a thread's run records of N = 5 x sums chains
// (chain 5 s + c: sum s, c 0-3 the SSE2 lanes, 4 the tail; T, M, m: total,
// maximum and minimum prefix of the thread's contiguous run of each chain) by
// bx_publish / bx_check_t / bx_eval_t on the records of parity par, two
// barriers: true when every chain's float sum is its integer total (lane c:
// tot), else the first failing thread h0 and, on lane c, chain c's exact prefix
// base0 before that thread's run. bad: the thread's terms are not all exact
// floats. T becomes the wave-exclusive prefix (bx_publish).
template <int N>
__device__ __forceinline__ bool lg_runs_exact(int (&T)[N], const int (&M)[N], const int (&m)[N], bool bad, int *X,
                                              int &par, bool no_tail, int &tot, int &h0, int &base0) {
    // a run whose own prefix leaves [-2^25, 2^25] cannot stay exact after any
    // exact start (|start| <= 2^24): flag it (terms < 2^26 are seen before any
    // wrap; the saturating A11 / A22 runs never wrap)
#pragma unroll
    for (int c = 0; c < N; c++) bad |= M[c] > (1 << 25) || m[c] < -(1 << 25);
    int *rec = X + par * 4 * kBxRecInts;
    par ^= 1;
    bx_publish<N>(T, rec, no_tail);
    __syncthreads();
    bx_check_t<N>(T, M, m, bad, rec, no_tail);
    __syncthreads();
    return bx_eval_t<N>(rec, tot, h0, base0);
}

// Diagnostic phase clocks (PSN_LK_STAMPS build, psn_lk_stamps.h; tools/lg_stamps.py):
// accumulated s_memtime ticks per phase of each point in lg_acc, thread 0's view,
// written as stamps[point][0..23] at the end.

// TQ: quads per ordered-chain tile (kLgTQs; the planner's choice per query).
// Minimum waves per SIMD 1: asking for more workgroups per CU was measured slower.
template <int TQ>
__global__ __launch_bounds__(kLgNT, 1) void lk_kernel_lg(LkLaunchArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int NT = kLgNT;
    const int tid = threadIdx.x, lane = tid & 63;
    if (A.poison_lds) lds_poison<NT>(smem, A.poison_lds);
    int *X = (int *)smem;                 // chain-check records, two parities
    float *RS = (float *)(X + kBxXInts);  // results (wave 0 -> all), err partials
    int *EP = (int *)(RS + 16);
    uint8_t *U = smem + lg_scr_bytes();   // band staging | tile planes
    float *PL = (float *)U;
    uint32_t *JR = (uint32_t *)(U + lg_tiles_b_bytes(TQ));  // J region (lg_jr), after the b tiles
    uint8_t *const slot = (uint8_t *)A.lg_ws + (long long)blockIdx.x * A.lg_slot * 8;
    int par = 0;

    for (int gi = blockIdx.x; gi < A.lk_wgs; gi += gridDim.x) {
        const int g = gi;
        int qi = 0;
        while (qi + 1 < A.nq && g >= A.q[qi + 1].wg_begin) qi++;
        const LkQueryDev &Q = A.q[qi];
        const int pi = lk_query_point(Q, A.counts, A.count_stride, g);
        if (pi < 0) continue;  // past the query's device count
        const int w = Q.win_w, h = Q.win_h, TR = Q.tile_rows;
        const int maxL = Q.max_level, flags = Q.flags;
        const bool sse = (flags & PSN_LK_ACCUM_SCALAR) == 0;
        const LgGeo G = lg_geo(w, h, sse);
        const int K = G.K, QW = G.QW, NQ = G.NQ;
        // (each plane from the one before: with all three as offsets of `slot` the A runs'
        // batch waits for all its loads at once and the kernel takes 151 VGPRs, not 149)
        uint2 *const IPs = (uint2 *)slot, *const XPs = IPs + NT * K;
        const LgSlot SL = {IPs, XPs, XPs + NT * K};
        const int q0 = min(tid * K, NQ), cnt = min(NQ - q0, K);  // this thread's quads [q0, q0 + cnt)
        const int y0 = q0 / QW, x0 = q0 - y0 * QW;
        const int PM = bx_pm(w);  // I patch dwords per row
        const bool jrm = Q.lg_jr != 0;
        const int JRW = st_jreg_w(w), JRH = st_jreg_h(h), JRP4 = bx_jrp(w) >> 2;
        uint8_t *Pimg = U;

        const float hwx = __fmul_rn((float)(w - 1), 0.5f), hwy = __fmul_rn((float)(h - 1), 0.5f);
        const float px0 = A.prev[2 * pi], py0 = A.prev[2 * pi + 1];
        float NPx = 0.f, NPy = 0.f;
        if (flags & PSN_LK_USE_INITIAL_FLOW) {
            NPx = A.next[2 * pi];
            NPy = A.next[2 * pi + 1];
        }
        int status = 1;
        float errv = 0.f;
        unsigned nwin = 0;  // window passes (A phase + iterations): the sample count / (w*h)
#ifdef PSN_LK_STAMPS
        unsigned long long lg_acc[24] = {}, lg_t = 0, lg_t0 = 0;
        PSN_CLK_ORDERED(lg_t0);
        lg_t = lg_t0;
#endif

        for (int level = maxL; level >= 0; level--) {
            const LevelDev I = ring_level_u(A.ring, Q.prev_slot, level);
            const LevelDev J = ring_level_u(A.ring, Q.next_slot, level);
            const int cols = I.w, rows = I.h;
            // the LDS copy of the J region around the window (lg_jr): restaged when the
            // window at (inx, iny) leaves it (the A phase's bands and tiles reuse its LDS)
            bool jr_valid = false;
            int jr_x0 = 0, jr_y0 = 0;
            auto window_j = [&](int inx, int iny, int w00, int w01, int w10, int w11) {
                if (jrm && !(jr_valid && jr_covers(inx, iny, w, h, jr_x0, jr_y0, JRW, JRH))) {
                    // every reader of the previous copy passed a barrier since
                    jr_x0 = (inx - kStJMargin) & ~3;
                    jr_y0 = iny - kStJMargin;
                    dma_patch<NT>((uint8_t *)JR, J, jr_y0, jr_x0, JRW, JRH, JRP4, Q.dv_bxjr);
                    dma_wait();
                    __syncthreads();
                    jr_valid = true;
                }
                return lg_j(J, inx, iny, w, h, w00, w01, w10, w11, jrm ? JR : nullptr, JRP4, jr_x0, jr_y0);
            };
            const Guess gs = level_guess(level, maxL, flags, px0, py0, NPx, NPy);
            NPx = gs.x;
            NPy = gs.y;
            const float scale = ldexpf(1.f, -level);
            const float px = __fsub_rn(__fmul_rn(px0, scale), hwx), py = __fsub_rn(__fmul_rn(py0, scale), hwy);
            const int ipx = cv_floor(px), ipy = cv_floor(py);
            if (win_outside(ipx, ipy, w, h, cols, rows)) {
                if (level == 0) {
                    status = 0;
                    errv = 0.f;
                }
                continue;
            }
            int iw00, iw01, iw10, iw11;
            bilin_weights(__fsub_rn(px, (float)ipx), __fsub_rn(py, (float)ipy), iw00, iw01, iw10, iw11);
            float nx = __fsub_rn(gs.x, hwx), ny = __fsub_rn(gs.y, hwy);
            nwin++;

            // ---- A phase (1): window values, band by band: the band's I patch rows
            // by LDS-DMA, then each quad's Scharr + bilinear values (bx_unit) into
            // the slot ----
            {
                const int sh = (ipx - 1) & 3;
                const bool interior = ipx >= 0 && ipy >= 0 && ipx + 4 * QW + 2 <= cols && ipy + h + 1 <= rows;
                const int c256 = 1 << 8, c8192 = 1 << 13;
                const uint32_t *P32 = (const uint32_t *)Pimg;
                int gdum0 = 0, gdum1 = 0;  // (the A runs below track the gradients)
                auto band = [&](auto inner) {
                    constexpr bool IN = decltype(inner)::value;
                    for (int r0 = 0; r0 < h; r0 += TR) {
                        const int th = min(TR, h - r0);
                        __syncthreads();  // the previous band's (tile's, level's, point's) LDS readers are done
                        dma_rows<NT>(Pimg, I, ipy + r0 - 1, ipx - 1, w + 3, th + 3, PM);
                        dma_wait();
                        __syncthreads();
                        PSN_PH_MARK(lg_acc, lg_t, 7);  // band staging
                        Walk wk;
                        wk.init(tid, NT, QW);
                        for (int qb = tid; qb < th * QW; qb += NT, wk.step()) {
                            unsigned ip[2], xp[2], yp[2];
                            bx_unit<IN, false>(P32, PM, sh, wk.y, wk.x, true, w, ipx, ipy + r0, cols, rows, iw00, iw01,
                                               iw10, iw11, c256, c8192, ip, xp, yp, gdum0, gdum1);
                            const int idx = lg_slot_index(G, (r0 + wk.y) * QW + wk.x);
                            SL.ip[idx] = make_uint2(ip[0], ip[1]);
                            SL.xp[idx] = make_uint2(xp[0], xp[1]);
                            SL.yp[idx] = make_uint2(yp[0], yp[1]);
                        }
                        PSN_PH_MARK(lg_acc, lg_t, 9);  // band quads
                    }
                };
                if (interior)
                    band(std::true_type());
                else
                    band(std::false_type());
            }
            __syncthreads();  // the window values of every band for every thread
            PSN_PH_MARK(lg_acc, lg_t, 0);  // A phase: window values

            // ---- A phase (2): the 15 A chains (sum x class) as runs over the
            // thread's quads, the block check, ordered chains if inexact ----
            float s3[3];   // the raw A11, A12, A22 sums
            int gmax = 0;  // max |Ix|, |Iy| of the thread's pixels (exactness of the b terms)
            {
                int T[15] = {}, M[15] = {}, m[15] = {};  // run records; chains 0-4: A11, 5-9: A12, 10-14: A22
                lg_walk<false, true, true>(SL, cnt, y0, x0, QW, [&](const LgQ &v, int, int qx) {
                    int gx[4], gy[4];
                    lg_unpack4(v.xp, gx);
                    lg_unpack4(v.yp, gy);
                    // (A11 / A22 runs saturate at 2^30: a long run never wraps; a run past 2^25
                    // fails the check below, as it must)
                    auto term = [&](int c, int i) {
                        T[c] = (int)sat_add((unsigned)T[c], (unsigned)(gx[i] * gx[i]));
                        T[10 + c] = (int)sat_add((unsigned)T[10 + c], (unsigned)(gy[i] * gy[i]));
                        run_add(T[5 + c], M[5 + c], m[5 + c], gx[i] * gy[i]);
                    };
                    if (qx < G.nA) {  // SSE2 quad: pixel i feeds lane chain i
#pragma unroll
                        for (int i = 0; i < 4; i++) term(i, i);
                    } else {  // the tail chain, in order (pixels past w carry zero gradients)
#pragma unroll
                        for (int i = 0; i < 4; i++) term(4, i);
                    }
#pragma unroll
                    for (int i = 0; i < 4; i++) gmax = max(gmax, max(abs(gx[i]), abs(gy[i])));
                });
                // A11 / A22 terms are >= 0: the maximum prefix is the total
#pragma unroll
                for (int c = 0; c < 5; c++) M[c] = T[c], M[10 + c] = T[10 + c];
                int tot, h0, base0;
                if (lg_runs_exact(T, M, m, false, X, par, G.tA == 0, tot, h0, base0)) {
#pragma unroll
                    for (int s = 0; s < 3; s++) s3[s] = combine_a5([&](int i) { return rl_f(tot, i); }, s, sse);
                } else {
                    // ordered chains from thread h0's run on (every earlier prefix is an
                    // exact integer: the chain lanes start from base0)
                    lg_ordered<3, TQ, false>(
                        G, G.nA, G.tA, SL, min(h0 * K, NQ), (float)base0, PL, RS, sse,
                        [&](const LgQ &v, int, int) {
                            int gx[4], gy[4];
                            lg_unpack4(v.xp, gx);
                            lg_unpack4(v.yp, gy);
                            return [=](int i, float(&t)[3]) {
                                t[0] = (float)(gx[i] * gx[i]);
                                t[1] = (float)(gx[i] * gy[i]);
                                t[2] = (float)(gy[i] * gy[i]);
                            };
                        },
                        [&](int) {}, s3);
                }
            }
            PSN_PH_MARK(lg_acc, lg_t, 1);  // A chains
            const LkSolve S = lk_solve(s3[0], s3[1], s3[2], w * h, Q.min_eig);
            if (flags & PSN_LK_GET_MIN_EIGENVALS) errv = S.minEig;
            if (!S.ok) {
                if (level == 0) status = 0;
                continue;
            }

            float pdx = 0.f, pdy = 0.f;
            for (int j = 0; j < Q.max_count; j++) {
                const int inx = cv_floor(nx), iny = cv_floor(ny);
                if (win_outside(inx, iny, w, h, cols, rows)) {
                    if (level == 0) status = 0;
                    break;
                }
                nwin++;
                int w00, w01, w10, w11;
                bilin_weights(__fsub_rn(nx, (float)inx), __fsub_rn(ny, (float)iny), w00, w01, w10, w11);
                const LgJ JJ = window_j(inx, iny, w00, w01, w10, w11);
                // ---- main pass: the thread's quads in order, the 10 b chains as runs ----
                int T[10] = {}, M[10] = {}, m[10] = {};  // run records; chains 0-4: b1, 5-9: b2
                int dmax = 0;
                // a quad's diffs J - I* and gradients (the main pass and the fallback writers)
                auto b_quad = [&](const LgQ &v, int y, int qx, int(&d)[4], int(&gx)[4], int(&gy)[4]) {
                    lg_diffs(JJ, y, qx, v.ip, d);
                    lg_unpack4(v.xp, gx);
                    lg_unpack4(v.yp, gy);
                };
                lg_walk<true, true, true>(SL, cnt, y0, x0, QW, [&](const LgQ &v, int y, int qx) {
                    int d[4], gx[4], gy[4];
                    b_quad(v, y, qx, d, gx, gy);
                    auto term = [&](int c, int i) {
                        run_add(T[c], M[c], m[c], __mul24(d[i], gx[i]));
                        run_add(T[5 + c], M[5 + c], m[5 + c], __mul24(d[i], gy[i]));
                    };
                    if (qx < G.nB2) {  // SSE2 quad: pixel i feeds lane chain i
#pragma unroll
                        for (int i = 0; i < 4; i++) term(i, i);
                    } else {  // the tail chain, in order (pixels past w: zero gradients)
#pragma unroll
                        for (int i = 0; i < 4; i++) term(4, i);
                    }
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (4 * qx + i < w) dmax = max(dmax, abs(d[i]));
                });
                PSN_PH_MARK(lg_acc, lg_t, 2);  // main pass
                PSN_PH_COUNT(lg_acc, 10);
                // every term is an exact float unless |d| * |g| > 2^24
                const bool bad = (long long)dmax * gmax > (long long)kExact;
                int tot, h0, base0;
                const bool bex = lg_runs_exact(T, M, m, bad, X, par, G.tB == 0, tot, h0, base0);
                PSN_PH_MARK(lg_acc, lg_t, 3);  // publish / check / eval
                float b[2];
                if (bex) {
                    combine_b10([&](int i) { return rl_f(tot, i); }, sse, b[0], b[1]);
                } else {
                    PSN_PH_COUNT(lg_acc, 11);
                    PSN_PH_MARK(lg_acc, lg_t, 4);
                    // 18: pads of the next tile (14: tiles), 13: barrier wait, 16: writes, loads, tile
                    // geometry, 17: chain sums, 5: ordered b chains
                    auto markB = [&](int i) {
                        PSN_PH_MARK(lg_acc, lg_t, i == 0 ? 18 : i == 1 ? 13 : i == 2 ? 16 : i == 3 ? 17 : 5);
                        if (i == 0) PSN_PH_COUNT(lg_acc, 14);
                    };
                    // ordered float chains from thread h0's run on (chain lanes: wave 0,
                    // lanes 0-9, from their exact prefixes base0), tiles of TQ quads
                    lg_ordered<2, TQ, true>(
                        G, G.nB2, G.tB, SL, min(h0 * K, NQ), (float)base0, PL, RS + 4, sse,
                        [&](const LgQ &v, int y, int qx) {
                            int d[4], gx[4], gy[4];
                            b_quad(v, y, qx, d, gx, gy);
                            return [=](int i, float(&t)[2]) {
                                t[0] = (float)__mul24(d[i], gx[i]);
                                t[1] = (float)__mul24(d[i], gy[i]);
                            };
                        },
                        markB, b);
                }
                PSN_PH_MARK(lg_acc, lg_t, 6);  // results
                float dx, dy;
                const double dd = lk_update(S.A11, S.A12, S.A22, S.invD, b[0], b[1], hwx, hwy, nx, ny, NPx, NPy, dx, dy);
                if (lk_stop(dd, Q.eps2, j, dx, dy, pdx, pdy, NPx, NPy)) break;
            }

            if (level == 0 && status && A.err && (flags & PSN_LK_GET_MIN_EIGENVALS) == 0) {
                const float qxf = __fsub_rn(NPx, hwx), qyf = __fsub_rn(NPy, hwy);
                const int iqx = cv_floor(qxf), iqy = cv_floor(qyf);
                if (win_outside(iqx, iqy, w, h, cols, rows)) {
                    status = 0;
                    continue;
                }
                if (flags & PSN_LK_ERR_STATUS_ONLY) continue;  // the re-check was all: err[] = 0
                int w00, w01, w10, w11;
                bilin_weights(__fsub_rn(qxf, (float)iqx), __fsub_rn(qyf, (float)iqy), w00, w01, w10, w11);
                const LgJ JJ = window_j(iqx, iqy, w00, w01, w10, w11);
                unsigned e = 0;
                lg_walk<true, false, false>(SL, cnt, y0, x0, QW, [&](const LgQ &v, int y, int qx) {
                    int d[4];
                    lg_diffs(JJ, y, qx, v.ip, d);
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (4 * qx + i < w) e = sat_add(e, (unsigned)abs(d[i]));
                });
                e = wave_sum_sat(e);
                if (lane == 0) EP[tid >> 6] = (int)e;
                __syncthreads();
                const unsigned et = sat_add(sat_add((unsigned)EP[0], (unsigned)EP[1]), sat_add((unsigned)EP[2], (unsigned)EP[3]));
                float errval;
                if (et <= (unsigned)kExact) {
                    errval = (float)et;  // every partial sum of errval += |diff| is an exact integer
                } else {  // row-major order, one lane, tiles of kLgTQE quads
                    float acc = 0.f;
                    auto pixel_of = [&](int q) {  // row-major pixel index of quad q
                        const LgRC rc = lg_rc(G, q);
                        return rc.y * w + 4 * rc.qx;
                    };
                    for (int a = 0; a < NQ; a += kLgTQE) {
                        const int b = min(a + kLgTQE, NQ);
                        const int pa = pixel_of(a);
                        __syncthreads();
                        const int q = a + tid;
                        if (q < b) {
                            const LgRC rc = lg_rc(G, q);
                            int d[4];
                            lg_diffs(JJ, rc.y, rc.qx, SL.ip[lg_slot_index(G, q)], d);
#pragma unroll
                            for (int i = 0; i < 4; i++)
                                if (4 * rc.qx + i < w) PL[rc.y * w + 4 * rc.qx + i - pa] = (float)abs(d[i]);
                        }
                        __syncthreads();
                        const int pb = b < NQ ? pixel_of(b) : w * h;
                        if (tid == 0) acc = chain_sum(PL, pb - pa, acc);
                    }
                    if (tid == 0) RS[8] = acc;
                    __syncthreads();
                    errval = RS[8];
                }
                errv = lk_err(errval, w * h);
            }
        }

#ifdef PSN_LK_STAMPS
        {
            unsigned long long t_end;
            PSN_CLK_ORDERED(t_end);
            lg_acc[15] = t_end - lg_t0;
            if (tid == 0 && A.stamps)
                for (int i = 0; i < 24; i++) A.stamps[(size_t)g * 64 + i] = lg_acc[i];
        }
#endif
        if (tid == 0) {
            A.next[2 * pi] = NPx;
            A.next[2 * pi + 1] = NPy;
            A.status[pi] = (uint8_t)status;
            if (A.err) A.err[pi] = errv;
            if (A.samples) atomicAdd(A.samples, (unsigned long long)nwin * (unsigned)(w * h));
        }
        __syncthreads();  // the next point reuses the slot, the LDS and the records
    }
}

// The instantiations of lk_kernel_lg, written ONCE: the launch dispatch and the
// dynamic-LDS attribute loop of lg_kernels_init are both generated from this
// list, so a tile size cannot launch without its attribute. X(TQ): the
// planner's tile sizes kLgTQs, in its order.
#define PSN_LG_KERNELS(X) X(192) X(128)
constexpr bool lg_kernels_are_tqs() {
#define PSN_LG_TQ(TQ) TQ,
    constexpr int tqs[] = {PSN_LG_KERNELS(PSN_LG_TQ)};
#undef PSN_LG_TQ
    if (sizeof(tqs) != sizeof(kLgTQs)) return false;
    for (size_t i = 0; i < sizeof(tqs) / sizeof(tqs[0]); i++)
        if (tqs[i] != kLgTQs[i]) return false;
    return true;
}
static_assert(lg_kernels_are_tqs(), "PSN_LG_KERNELS must list exactly kLgTQs");

hipError_t launch_lk_lg(const LkLaunchArgs &a, int grid, int lds_bytes, int tq, hipStream_t s) {
    if (grid <= 0 || a.lk_wgs <= 0) return hipSuccess;
    if (!a.lg_ws || a.lg_slot <= 0 || lds_bytes > kMaxLdsBytes) return hipErrorInvalidValue;
#define PSN_LG_LAUNCH(TQ)                                                                   \
    if (tq == TQ) {                                                                         \
        hipLaunchKernelGGL(lk_kernel_lg<TQ>, dim3(grid), dim3(kLgNT), lds_bytes, s, a);     \
        return hipGetLastError();                                                           \
    }
    PSN_LG_KERNELS(PSN_LG_LAUNCH)
#undef PSN_LG_LAUNCH
    return hipErrorInvalidValue;  // (a missing instantiation is an error, never another kernel)
}

hipError_t lg_kernels_init() {
#define PSN_LG_FN(TQ) (const void *)lk_kernel_lg<TQ>,
    const void *fns[] = {PSN_LG_KERNELS(PSN_LG_FN)};
#undef PSN_LG_FN
    for (const void *f : fns) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace psn
