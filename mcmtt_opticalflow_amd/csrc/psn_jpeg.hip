// JPEG frame ingest on the device (include/psn_jpeg.h): the libjpeg baseline
// decode behind cv::imread (psn_where/main.cpp:144), restated for gfx950.
//
//   host   markers -> quantisation tables (natural order), Huffman tables
//          (canonical maxcode/valoffset + a 9-bit lookahead table), component
//          geometry, restart-segment byte offsets (RSTn positions); one pinned
//          staging block [tables | segment offsets | entropy bytes] -> one H2D
//   K1     jpeg_entropy_kernel: one thread per restart segment decodes its MCUs
//          (jdhuff.c: fill with 0xFF00 unstuffing, a marker feeds zeros; DC
//          prediction reset per segment) into int16 coefficient blocks
//   K1p    a plain stream without restart intervals takes four kernels in K1's
//          place (the symbol step they share with the CPU model is
//          psn_jpeg_entropy.h):
//          jpeg_sync_kernel   one thread per subsequence of S bytes, 256 to a
//                             workgroup: decode from a cold state, then take the
//                             predecessor's exit state and decode again until no
//                             exit state of the workgroup changes
//          jpeg_chain_kernel  one workgroup, one thread per 256-subsequence
//                             sequence: carry the exit states across sequences to
//                             the fixed point, then the exclusive prefix sum of
//                             the blocks completed per subsequence
//          jpeg_emit_kernel   one thread per subsequence decodes from its true
//                             entry state and writes coefficients (DC: the
//                             difference)
//          jpeg_dc_kernel     one workgroup per component: inclusive scan of the
//                             DC differences in scan order
//   K2     jpeg_idct_kernel: one thread per 8x8 block, dequantise + islow IDCT
//          (jidctint.c, 64-bit intermediates as libjpeg-turbo's JLONG) + the
//          post-IDCT range-limit table -> component planes (u8)
//   K3     jpeg_color_kernel: one thread per pixel: fancy upsampling (jdsample.c
//          h2v1 / h2v2, edges replicated at the downsampled size), YCbCr->RGB
//          (jdcolor.c, SCALEBITS 16), BGR out
// Bit-identical to oracle/jpeg_oracle.c, which is pinned to libjpeg-turbo.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "psn_jpeg.h"
#include "psn_jpeg_entropy.h"  // HuffDev, the symbol step of the parallel path
#include "psn_lk.h"

namespace psn {
namespace {

constexpr int kJpegMaxComp = 3;

struct Tables {             // device copy per frame
    uint16_t qt[4][64];     // natural order
    HuffDev dc[4], ac[4];
};

struct CompGeo {
    int h, v, tq, td, ta;   // sampling factors, table selectors
    int bw, bh;             // blocks across / down (plane = bw*8 x bh*8)
    int dw, dh;             // downsampled size (edges of the fancy upsampler)
    int blk0;               // first coefficient block
    int plane0;             // byte offset of the plane
};

struct JpegArgs {
    int W, H, nc, hmax, vmax, mcux, nmcu, ri, nseg, data_len;
    CompGeo c[kJpegMaxComp];
    const Tables *tab;
    const int *seg;          // byte offset of each segment's first entropy byte
    const uint8_t *data;     // entropy-coded bytes
    int16_t *coef;           // [blocks][64], natural order
    uint8_t *planes;
    uint8_t *out;
    int out_stride;
    int nblocks;
};

__constant__ int kNatural[64 + 16] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
    63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};

// Bit reader of one segment (jdhuff.c fill_bit_buffer semantics).
struct BitReader {
    const uint8_t *p;
    int pos, end;
    unsigned long long buf;
    int n;
    bool marker;
    __device__ void fill() {
        while (n <= 56) {
            unsigned c = 0;
            if (!marker && pos < end) {
                c = p[pos];
                if (c == 0xFF) {
                    int q = pos + 1;
                    while (q < end && p[q] == 0xFF) q++;  // fill bytes
                    if (q < end && p[q] == 0) {
                        pos = q + 1;  // stuffed zero: a 0xFF data byte
                    } else {
                        marker = true;  // a marker: zeros from here on
                        c = 0;
                    }
                } else {
                    pos++;
                }
            }
            buf |= (unsigned long long)c << (56 - n);
            n += 8;
        }
    }
    __device__ unsigned peek(int k) {
        if (n < k) fill();
        return (unsigned)(buf >> (64 - k));
    }
    __device__ void skip(int k) {
        buf <<= k;
        n -= k;
    }
    __device__ int bits(int k) {
        if (k == 0) return 0;
        const unsigned v = peek(k);
        skip(k);
        return (int)v;
    }
    __device__ int decode(const HuffDev &h) {
        const unsigned look = peek(16);
        const unsigned f = h.fast[look >> 7];
        if (f) {
            skip((int)(f >> 8));
            return (int)(f & 255);
        }
        for (int l = 10; l <= 16; l++) {
            const int code = (int)(look >> (16 - l));
            if (code <= h.maxcode[l]) {
                skip(l);
                return h.vals[(code + h.valoff[l]) & 255];
            }
        }
        (void)peek(17);  // corrupt data: libjpeg has read a 17th bit when it warns and yields 0
        skip(17);
        return 0;
    }
};

__device__ __forceinline__ int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(JpegArgs A) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= A.nseg) return;
    const Tables &T = *A.tab;
    BitReader br;
    br.p = A.data;
    br.pos = A.seg[s];
    br.end = s + 1 < A.nseg ? A.seg[s + 1] : A.data_len;
    br.buf = 0;
    br.n = 0;
    br.marker = false;
    const int m0 = A.ri ? s * A.ri : 0, m1 = A.ri ? min(m0 + A.ri, A.nmcu) : A.nmcu;
    int last_dc[kJpegMaxComp] = {0, 0, 0};
    for (int mcu = m0; mcu < m1; mcu++) {
        const int mx = mcu % A.mcux, my = mcu / A.mcux;
        for (int ci = 0; ci < A.nc; ci++) {
            const CompGeo &g = A.c[ci];
            const int bh = A.nc == 1 ? 1 : g.h, bv = A.nc == 1 ? 1 : g.v;
            for (int by = 0; by < bv; by++)
                for (int bx = 0; bx < bh; bx++) {
                    int16_t *blk = A.coef + (size_t)(g.blk0 + (my * bv + by) * g.bw + mx * bh + bx) * 64;
                    const int sz = br.decode(T.dc[g.td]);
                    const int diff = sz ? extend(br.bits(sz), sz) : 0;
                    last_dc[ci] += diff;
                    blk[0] = (int16_t)last_dc[ci];
                    for (int k = 1; k < 64; k++) {
                        const int rs = br.decode(T.ac[g.ta]);
                        const int r = rs >> 4, sv = rs & 15;
                        if (sv) {
                            k += r;
                            blk[kNatural[k]] = (int16_t)extend(br.bits(sv), sv);
                        } else {
                            if (r != 15) break;
                            k += 15;
                        }
                    }
                }
        }
    }
}

// ---------------------------------------------------------------- parallel path
// Subsequence i owns the bits [i * 8S, (i + 1) * 8S) of the entropy bytes: its
// thread decodes the symbols that start there, and its exit state is the state at
// the first symbol boundary at or past its end.

struct DevStats {           // written by the kernels, read by psn_jpeg_last_stats
    int sync_rounds, chain_rounds, blocks, pad;
};

struct EntArgs {
    const Tables *tab;
    const uint8_t *data;     // entropy bytes (readable 16 bytes past len)
    long long len;
    int S;                   // subsequence bytes
    int nsub, nseq;          // subsequences, sequences of jent::kSeqLen
    int stage;               // 1: the workgroup's bytes are staged in LDS
    int nb0, bpm, nmcu;
    int td[kJpegMaxComp], ta[kJpegMaxComp];
    jent::Geo geo;
    unsigned long long *st;  // [nsub] exit state
    unsigned *cnt;           // [nsub] blocks completed inside the subsequence
    unsigned *pre;           // [nsub] exclusive prefix sum of cnt
    int *seq_rounds;         // [nseq] rounds of jpeg_sync_kernel's workgroup
    DevStats *stats;
    int16_t *coef;
};

struct LdsTabs {            // the scan's tables by component (lookups are divergent)
    HuffDev dc[kJpegMaxComp], ac[kJpegMaxComp];
};
static_assert(sizeof(LdsTabs) % 16 == 0, "LDS carve offsets stay 16-byte aligned");
constexpr int kNaturalLds = 96;  // jpeg_emit_kernel's LDS copy of the natural-order table (80 bytes, carve stays 16-aligned)
constexpr int kStageSlack = 64;  // bytes staged past the workgroup's last subsequence (a symbol may span its end)

__device__ __forceinline__ void stage_tables(const EntArgs &E, LdsTabs &L) {
    constexpr int nd = (int)(sizeof(HuffDev) / 4);
    for (int c = 0; c < E.geo.nc; c++) {
        const uint32_t *sd = (const uint32_t *)&E.tab->dc[E.td[c]], *sa = (const uint32_t *)&E.tab->ac[E.ta[c]];
        uint32_t *dd = (uint32_t *)&L.dc[c], *da = (uint32_t *)&L.ac[c];
        for (int k = threadIdx.x; k < nd; k += blockDim.x) {
            dd[k] = sd[k];
            da[k] = sa[k];
        }
    }
}

// Bytes by index: the staged window [w0, w1) from LDS, the rest from global
// memory, zeros from len on.
struct DevBytes {
    const uint8_t *lds;
    long long w0, w1;
    const uint8_t *g;
    long long len;
    __device__ __forceinline__ unsigned operator()(long long i) const {
        if (i >= w0 && i < w1) return lds[i - w0];
        return i < len ? g[i] : 0u;
    }
};

// Stage the bytes of the workgroup's kSeqLen subsequences (plus slack) as dwords.
__device__ __forceinline__ DevBytes stage_bytes(const EntArgs &E, uint8_t *sb) {
    DevBytes src{sb, 0, 0, E.data, E.len};
    if (E.stage) {
        src.w0 = (long long)blockIdx.x * jent::kSeqLen * E.S;
        src.w1 = min(src.w0 + (long long)jent::kSeqLen * E.S + kStageSlack, E.len);
        const int nd = (int)((src.w1 - src.w0 + 3) / 4);  // the last dword may read past len: inside the blob's slack
        const uint32_t *s = (const uint32_t *)(E.data + src.w0);
        for (int k = threadIdx.x; k < nd; k += blockDim.x) ((uint32_t *)sb)[k] = s[k];
    }
    return src;
}

__global__ __launch_bounds__(256) void jpeg_sync_kernel(EntArgs E) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    LdsTabs &L = *(LdsTabs *)smem;
    unsigned long long *sx = (unsigned long long *)(smem + sizeof(LdsTabs));  // exit state per thread
    stage_tables(E, L);
    const DevBytes src = stage_bytes(E, smem + sizeof(LdsTabs) + jent::kSeqLen * 8);
    __syncthreads();
    const jent::Tabs T{L.dc, L.ac, E.nb0, E.bpm};
    const int t = threadIdx.x;
    const long long i = (long long)blockIdx.x * jent::kSeqLen + t;
    const bool active = i < E.nsub;
    const long long subbits = 8LL * E.S;
    const unsigned long long end = (unsigned long long)((i + 1) * subbits);
    unsigned long long entry = 0, ex = 0;
    unsigned cnt = 0;
    if (active) {  // round 0: from cold (the stream's first thread from the true state)
        entry = i ? jent::cold_state(src, i * E.S) : jent::pack(0, 0, 0);
        jent::CountSink cs;
        ex = jent::run(src, T, entry, end, subbits + 1, cs);
        cnt = cs.blocks;
    }
    sx[t] = ex;
    int rounds = 1;
    __syncthreads();
    for (int r = 1; r < jent::kSeqLen; r++) {  // thread r is final after round r
        const unsigned long long pred = t ? sx[t - 1] : entry;
        __syncthreads();
        int changed = 0;
        if (active && t && pred != entry) {
            entry = pred;
            jent::CountSink cs;
            const unsigned long long e = jent::run(src, T, entry, end, subbits + 1, cs);
            cnt = cs.blocks;
            if (e != ex) {
                ex = e;
                sx[t] = e;
                changed = 1;
            }
        }
        rounds++;
        if (!__syncthreads_or(changed)) break;
    }
    if (active) {
        E.st[i] = ex;
        E.cnt[i] = cnt;
    }
    if (t == 0) E.seq_rounds[blockIdx.x] = rounds;
}

// Inclusive scan over the workgroup (any multiple of 64 threads up to 1024);
// `ws` holds one word per wave. Every thread calls it.
__device__ __forceinline__ unsigned block_scan_incl(unsigned v, unsigned *ws, unsigned *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    __syncthreads();  // the previous call's reads of ws are done
    if (lane == 63) ws[w] = v;
    __syncthreads();
    unsigned off = 0, tot = 0;
    for (int k = 0; k < nw; k++) {
        const unsigned x = ws[k];
        if (k < w) off += x;
        tot += x;
    }
    *total = tot;
    return v + off;
}

__global__ __launch_bounds__(1024) void jpeg_chain_kernel(EntArgs E) {
    __shared__ LdsTabs L;
    __shared__ unsigned long long sx[jent::kChainLen];  // last exit state of each sequence of the pass
    __shared__ unsigned ws[16];
    __shared__ int smax;
    const int tid = threadIdx.x;
    stage_tables(E, L);
    if (tid == 0) smax = 0;
    __syncthreads();
    const jent::Tabs T{L.dc, L.ac, E.nb0, E.bpm};
    const DevBytes src{nullptr, 0, 0, E.data, E.len};
    const long long subbits = 8LL * E.S;
    int rounds = 0;
    unsigned long long carry = jent::pack(0, 0, 0);  // the state entering the pass's first sequence
    for (int c0 = 0; c0 < E.nseq; c0 += jent::kChainLen) {
        const int j = c0 + tid, npass = min(jent::kChainLen, E.nseq - c0);
        const bool active = j < E.nseq;
        const long long first = (long long)j * jent::kSeqLen, last = min(first + jent::kSeqLen, (long long)E.nsub) - 1;
        if (active) sx[tid] = E.st[last];
        unsigned long long walked = ~0ULL;  // the entry state the sequence's stored states follow from
        __syncthreads();
        for (int r = 0; r < npass; r++) {  // the pass's sequence r is final after round r
            const unsigned long long entry = tid ? sx[active ? tid - 1 : 0] : carry;
            __syncthreads();
            int changed = 0;
            if (active && j > 0 && entry != walked) {
                // sequence 0 was decoded from the true state; every other one from a cold
                // state: walk it from its entry until the walk meets the stored states
                unsigned long long cur = entry;
                bool met = false;
                for (long long i = first; i <= last && !met; i++) {
                    jent::CountSink cs;
                    cur = jent::run(src, T, cur, (unsigned long long)((i + 1) * subbits), subbits + 1, cs);
                    met = cur == E.st[i];
                    E.st[i] = cur;
                    E.cnt[i] = cs.blocks;
                }
                if (!met && cur != sx[tid]) {
                    sx[tid] = cur;
                    changed = 1;
                }
                walked = entry;
            }
            rounds++;
            if (!__syncthreads_or(changed)) break;
        }
        __syncthreads();
        carry = sx[npass - 1];
        __syncthreads();
    }
    // exclusive prefix sum of the blocks per subsequence
    unsigned run_sum = 0;
    for (long long base = 0; base < E.nsub; base += blockDim.x) {
        const long long i = base + tid;
        const unsigned v = i < E.nsub ? E.cnt[i] : 0u;
        unsigned tot;
        const unsigned incl = block_scan_incl(v, ws, &tot);
        if (i < E.nsub) E.pre[i] = run_sum + incl - v;
        run_sum += tot;
    }
    int m = 0;
    for (int k = tid; k < E.nseq; k += blockDim.x) m = max(m, E.seq_rounds[k]);
    atomicMax(&smax, m);
    __syncthreads();
    if (tid == 0) {
        E.stats->sync_rounds = smax;
        E.stats->chain_rounds = rounds;
    }
}

__global__ __launch_bounds__(256) void jpeg_emit_kernel(EntArgs E) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    LdsTabs &L = *(LdsTabs *)smem;
    uint8_t *snat = smem + sizeof(LdsTabs);  // the natural-order table: a divergent lookup per coefficient
    stage_tables(E, L);
    if (threadIdx.x < 64 + 16) snat[threadIdx.x] = jent::kNaturalDev[threadIdx.x];
    const DevBytes src = stage_bytes(E, smem + sizeof(LdsTabs) + kNaturalLds);
    __syncthreads();
    const long long i = (long long)blockIdx.x * jent::kSeqLen + threadIdx.x;
    if (i >= E.nsub) return;
    const jent::Tabs T{L.dc, L.ac, E.nb0, E.bpm};
    const long long subbits = 8LL * E.S, total = E.geo.total;
    const bool last = i == E.nsub - 1;
    const long long g0 = E.pre[i];
    jent::EmitSink sink(E.geo, T, E.coef, snat, g0);
    // the last thread goes on past its end, and past the data (zeros), to the scan's
    // last block, as the serial reader does for a truncated file: at most 64 symbols a block
    const unsigned long long end = last ? ~0ULL >> 16 : (unsigned long long)((i + 1) * subbits);
    const long long bound = subbits + 1 + (last ? (total - min(g0, total) + 1) * 64 : 0);
    jent::run(src, T, i ? E.st[i - 1] : jent::pack(0, 0, 0), end, bound, sink);
    if (last) E.stats->blocks = (int)min(sink.g, total);
}

__global__ __launch_bounds__(1024) void jpeg_dc_kernel(EntArgs E) {
    __shared__ unsigned ws[16];
    const int ci = blockIdx.x;
    const long long n = (long long)E.nmcu * E.geo.c[ci].h * E.geo.c[ci].v;
    unsigned last_dc = 0;  // the serial kernel's last_dc[ci], modulo 2^32
    for (long long base = 0; base < n; base += blockDim.x) {
        const long long e = base + threadIdx.x;
        long long blk = e < n ? jent::dc_block(E.geo, ci, e) : -1;
        if (blk >= E.geo.nblocks) blk = -1;
        const unsigned v = blk >= 0 ? (unsigned)(int)E.coef[blk * 64] : 0u;
        unsigned tot;
        const unsigned incl = block_scan_incl(v, ws, &tot);
        if (blk >= 0) E.coef[blk * 64] = (int16_t)(int)(last_dc + incl);
        last_dc += tot;
    }
}

__device__ __forceinline__ long long desc(long long x, int n) { return (x + (1LL << (n - 1))) >> n; }
__device__ __forceinline__ uint8_t range_limit(long long v) {
    const int idx = (int)(v & 1023);
    return (uint8_t)(idx < 128 ? idx + 128 : idx < 512 ? 255 : idx < 896 ? 0 : idx - 896);
}

// jidctint.c: one 1-D pass over 8 values (even part: rotator sqrt(2)*c(-6);
// odd part per figure 8), shared by columns and rows.
__device__ __forceinline__ void idct8(const long long (&d)[8], long long (&o)[8]) {
    const long long z1 = (d[2] + d[6]) * 4433;
    const long long t2 = z1 + d[6] * -15137, t3 = z1 + d[2] * 6270;
    const long long t0 = (d[0] + d[4]) * 8192, t1 = (d[0] - d[4]) * 8192;
    const long long t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    long long a0 = d[7], a1 = d[5], a2 = d[3], a3 = d[1];
    long long z1o = a0 + a3, z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const long long z5 = (z3 + z4) * 9633;
    a0 *= 2446;
    a1 *= 16819;
    a2 *= 25172;
    a3 *= 12299;
    z1o *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    a0 += z1o + z3;
    a1 += z2 + z4;
    a2 += z2 + z3;
    a3 += z1o + z4;
    o[0] = t10 + a3;
    o[7] = t10 - a3;
    o[1] = t11 + a2;
    o[6] = t11 - a2;
    o[2] = t12 + a1;
    o[5] = t12 - a1;
    o[3] = t13 + a0;
    o[4] = t13 - a0;
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(JpegArgs A) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= A.nblocks) return;
    int ci = 0;
    while (ci + 1 < A.nc && b >= A.c[ci + 1].blk0) ci++;
    const CompGeo &g = A.c[ci];
    const int lb = b - g.blk0, bx = lb % g.bw, by = lb / g.bw;
    const uint16_t *q = A.tab->qt[g.tq];
    const int16_t *blk = A.coef + (size_t)b * 64;
    int ws[64];
    for (int c = 0; c < 8; c++) {  // pass 1: columns, scaled by 2^PASS1_BITS
        long long d[8], o[8];
        for (int r = 0; r < 8; r++) d[r] = (long long)blk[8 * r + c] * q[8 * r + c];
        idct8(d, o);
        for (int r = 0; r < 8; r++) ws[8 * r + c] = (int)desc(o[r], 13 - 2);
    }
    uint8_t *dst = A.planes + g.plane0 + (size_t)(by * 8) * (g.bw * 8) + bx * 8;
    for (int r = 0; r < 8; r++) {  // pass 2: rows, descaled by 8 and 2^PASS1_BITS
        long long d[8], o[8];
        for (int k = 0; k < 8; k++) d[k] = ws[8 * r + k];
        idct8(d, o);
        uint32_t lo = 0, hi = 0;
        for (int k = 0; k < 4; k++) {
            lo |= (uint32_t)range_limit(desc(o[k], 13 + 2 + 3)) << (8 * k);
            hi |= (uint32_t)range_limit(desc(o[k + 4], 13 + 2 + 3)) << (8 * k);
        }
        uint32_t *row = (uint32_t *)(dst + (size_t)r * (g.bw * 8));
        row[0] = lo;
        row[1] = hi;
    }
}

// One fancy-upsampled chroma sample at full-resolution (x, y).
__device__ __forceinline__ int chroma(const JpegArgs &A, const CompGeo &g, int x, int y) {
    const uint8_t *pl = A.planes + g.plane0;
    const int pw = g.bw * 8;
    const int sx = A.hmax / g.h, sy = A.vmax / g.v;
    if (sx == 1 && sy == 1) return pl[(size_t)y * pw + x];
    const int i = x >> 1;
    if (sy == 1) {  // h2v1_fancy_upsample
        const uint8_t *row = pl + (size_t)y * pw;
        const int cur = row[i];
        if (g.dw == 1) return cur;
        if ((x & 1) == 0) return i == 0 ? cur : (cur * 3 + row[i - 1] + 1) >> 2;
        return i == g.dw - 1 ? cur : (cur * 3 + row[i + 1] + 2) >> 2;
    }
    const int j = y >> 1;  // h2v2_fancy_upsample
    const int jn = (y & 1) ? min(j + 1, g.dh - 1) : max(j - 1, 0);
    const uint8_t *r0 = pl + (size_t)j * pw, *r1 = pl + (size_t)jn * pw;
    const int cs = r0[i] * 3 + r1[i];
    if (g.dw == 1) return (cs * 4 + ((x & 1) ? 7 : 8)) >> 4;
    if ((x & 1) == 0) return i == 0 ? (cs * 4 + 8) >> 4 : (cs * 3 + r0[i - 1] * 3 + r1[i - 1] + 8) >> 4;
    return i == g.dw - 1 ? (cs * 4 + 7) >> 4 : (cs * 3 + r0[i + 1] * 3 + r1[i + 1] + 7) >> 4;
}

__device__ __forceinline__ uint8_t clamp255(int v) { return (uint8_t)min(max(v, 0), 255); }

__global__ __launch_bounds__(256) void jpeg_color_kernel(JpegArgs A) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= A.W) return;
    const CompGeo &gy = A.c[0];
    const int Y = A.planes[gy.plane0 + (size_t)y * (gy.bw * 8) + x];
    uint8_t *o = A.out + (size_t)y * A.out_stride + 3 * x;
    if (A.nc == 1) {
        o[0] = o[1] = o[2] = (uint8_t)Y;
        return;
    }
    const int cb = chroma(A, A.c[1], x, y) - 128, cr = chroma(A, A.c[2], x, y) - 128;
    // jdcolor.c build_ycc_rgb_table: FIX(1.402) 91881, FIX(1.772) 116130, FIX(0.71414) 46802, FIX(0.34414) 22554
    const int r = (91881 * cr + 32768) >> 16, b = (116130 * cb + 32768) >> 16;
    const int gsum = (-22554 * cb + 32768) + (-46802 * cr);
    o[0] = clamp255(Y + b);
    o[1] = clamp255(Y + (gsum >> 16));
    o[2] = clamp255(Y + r);
}

int rd16(const uint8_t *p) { return (p[0] << 8) | p[1]; }

// jdhuff.c jpeg_make_d_derived_tbl: false for a table libjpeg rejects with
// JERR_BAD_HUFF_TABLE -- more codes of a length than fit after the shorter ones
// (the canonical code would overflow its length; the all-ones code is not
// allowed), or a DC symbol above 15. Checked before any table entry is written.
bool build_huff(const uint8_t *bits, const uint8_t *vals, int nvals, bool dc, HuffDev &h) {
    for (int l = 1, code = 0; l <= 16; l++) {
        code += bits[l - 1];
        if (code >= (1 << l)) return false;
        code <<= 1;
    }
    if (dc)
        for (int i = 0; i < nvals; i++)
            if (vals[i] > 15) return false;
    memset(&h, 0, sizeof h);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; l++) {
        h.valoff[l] = k - code;
        const int n = bits[l - 1];
        for (int i = 0; i < n && l <= 9; i++) {  // lookahead entries of the codes of length <= 9
            const int c = code + i, span = 1 << (9 - l);
            for (int j = 0; j < span; j++) h.fast[(c << (9 - l)) | j] = (uint16_t)((l << 8) | vals[(k + i) & 255]);
        }
        code += n;
        k += n;
        h.maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    for (int i = 0; i < 256; i++) h.vals[i] = i < nvals ? vals[i] : 0;
    return true;
}

}  // namespace
}  // namespace psn

struct psn_jpeg_ctx {
    int device = 0;
    hipStream_t own = nullptr, stream = nullptr;
    uint8_t *d_blob = nullptr, *h_blob = nullptr;  // [Tables | segment offsets | entropy bytes]
    size_t blob_cap = 0;
    int16_t *d_coef = nullptr;
    size_t coef_cap = 0;
    uint8_t *d_planes = nullptr;
    size_t planes_cap = 0;
    hipEvent_t blob_free = nullptr;  // the previous frame's kernels have read the staging blob
    bool blob_pending = false;
    uint8_t *d_out = nullptr;  // psn_jpeg_decode's device BGR buffer
    size_t out_cap = 0;
    int ent_mode = 0, ent_sub = 0;  // psn_jpeg_debug_set_entropy
    uint8_t *d_par = nullptr;       // parallel path: [DevStats | states | counts | prefix sums | rounds]
    size_t par_cap = 0;
    psn_jpeg_stats last{};          // the last decode (host part; the kernels' counters are in d_par)
    bool decoded = false;
    int last_nblocks = 0;           // coefficient blocks of the last decode (psn_jpeg_debug_read_coefficients)
    std::string err;
};

namespace {

const int kNaturalHost[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                              12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                              35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                              58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

int jerr(psn_jpeg_ctx *c, int code, const char *fmt, ...) {
    if (c) {
        char b[256];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(b, sizeof b, fmt, ap);
        va_end(ap);
        c->err = b;
    }
    return code;
}

// A parsed frame: tables, geometry, entropy segments.
struct Parsed {
    psn::Tables tab;
    psn::JpegArgs a{};
    std::vector<int> seg;
    size_t ent0 = 0, ent1 = 0;  // entropy bytes [ent0, ent1) of the file
    // every 0xFF in [ent0, ent1) is followed by 0x00 and the last byte is not 0xFF:
    // no fill bytes, no embedded marker (psn_jpeg_entropy.h reads such streams)
    bool plain = true;
    // per Huffman slot (class tc, index th): 0 never defined, 1 valid, -1 the last
    // definition is one jpeg_make_d_derived_tbl rejects -- an error only for a table
    // the scan uses (libjpeg builds the derived tables of the scan's components)
    int hstate[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
};

int parse(const uint8_t *d, size_t n, Parsed &P, std::string &why) {
    memset(&P.tab, 0, sizeof P.tab);
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return why = "not a JPEG (no SOI)", PSN_LK_ERR_ARG;
    int ids[psn::kJpegMaxComp] = {0, 0, 0};
    bool sof = false;
    size_t p = 2;
    while (p + 4 <= n) {
        if (d[p] != 0xFF) return why = "marker expected", PSN_LK_ERR_ARG;
        const int m = d[p + 1];
        if (m == 0xFF) {
            p++;
            continue;
        }
        const int len = psn::rd16(d + p + 2);
        if (len < 2 || p + 2 + (size_t)len > n) return why = "truncated segment", PSN_LK_ERR_ARG;
        const uint8_t *s = d + p + 4;
        const int sl = len - 2;
        if (m == 0xDB) {
            for (int o = 0; o < sl;) {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                if (tq > 3 || o + 1 + (pq ? 128 : 64) > sl) return why = "bad DQT", PSN_LK_ERR_ARG;
                for (int i = 0; i < 64; i++)
                    P.tab.qt[tq][kNaturalHost[i]] = (uint16_t)(pq ? psn::rd16(s + o + 1 + 2 * i) : s[o + 1 + i]);
                o += 1 + (pq ? 128 : 64);
            }
        } else if (m == 0xC4) {
            for (int o = 0; o < sl;) {
                const int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3 || o + 17 > sl) return why = "bad DHT", PSN_LK_ERR_ARG;
                int cnt = 0;
                for (int l = 0; l < 16; l++) cnt += s[o + 1 + l];
                if (cnt > 256 || o + 17 + cnt > sl) return why = "bad DHT", PSN_LK_ERR_ARG;
                P.hstate[tc][th] = psn::build_huff(s + o + 1, s + o + 17, cnt, tc == 0, tc ? P.tab.ac[th] : P.tab.dc[th]) ? 1 : -1;
                o += 17 + cnt;
            }
        } else if (m == 0xC0 || m == 0xC1) {
            if (sl < 6 || s[0] != 8) return why = "not 8-bit", PSN_LK_ERR_UNSUPPORTED;
            P.a.H = psn::rd16(s + 1);
            P.a.W = psn::rd16(s + 3);
            P.a.nc = s[5];
            if ((P.a.nc != 1 && P.a.nc != 3) || sl < 6 + 3 * P.a.nc || !P.a.W || !P.a.H)
                return why = "unsupported component count", PSN_LK_ERR_UNSUPPORTED;
            for (int c = 0; c < P.a.nc; c++) {
                ids[c] = s[6 + 3 * c];
                P.a.c[c].h = s[7 + 3 * c] >> 4;
                P.a.c[c].v = s[7 + 3 * c] & 15;
                P.a.c[c].tq = s[8 + 3 * c] & 3;
                if (P.a.c[c].h < 1 || P.a.c[c].h > 2 || P.a.c[c].v < 1 || P.a.c[c].v > 2)
                    return why = "unsupported sampling", PSN_LK_ERR_UNSUPPORTED;
            }
            sof = true;
        } else if ((m >= 0xC2 && m <= 0xCF) && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            return why = "not baseline sequential Huffman", PSN_LK_ERR_UNSUPPORTED;
        } else if (m == 0xDD) {
            P.a.ri = sl >= 2 ? psn::rd16(s) : 0;
        } else if (m == 0xDA) {
            if (!sof || sl < 1 || s[0] != P.a.nc) return why = "unsupported scan", PSN_LK_ERR_UNSUPPORTED;
            for (int i = 0; i < P.a.nc; i++)
                for (int c = 0; c < P.a.nc; c++)
                    if (ids[c] == s[1 + 2 * i]) {
                        P.a.c[c].td = (s[2 + 2 * i] >> 4) & 3;
                        P.a.c[c].ta = s[2 + 2 * i] & 3;
                    }
            // the scan's tables (jdhuff.c start_pass_huff_decoder -> jpeg_make_d_derived_tbl:
            // JERR_NO_HUFF_TABLE, JERR_BAD_HUFF_TABLE)
            for (int c = 0; c < P.a.nc; c++)
                for (int tc = 0; tc < 2; tc++) {
                    const int st = P.hstate[tc][tc ? P.a.c[c].ta : P.a.c[c].td];
                    if (st == 0) return why = "Huffman table not defined", PSN_LK_ERR_ARG;
                    if (st < 0) return why = "bad DHT (code lengths or DC symbols)", PSN_LK_ERR_ARG;
                }
            P.ent0 = p + 2 + (size_t)len;
            break;
        }
        p += 2 + (size_t)len;
    }
    if (!sof || !P.ent0) return why = "no frame / scan header", PSN_LK_ERR_ARG;
    psn::JpegArgs &a = P.a;
    a.hmax = a.vmax = 1;
    for (int c = 0; c < a.nc; c++) {
        a.hmax = std::max(a.hmax, a.c[c].h);
        a.vmax = std::max(a.vmax, a.c[c].v);
    }
    // 4:4:4, 4:2:2 (h2v1) and 4:2:0 (h2v2) chroma; 4:4:0 (luma 1x2: a vertical-only
    // upsample, h1v2) has no path in jpeg_color_kernel's chroma() and is refused
    if (a.nc == 3 && (a.c[0].h != a.hmax || a.c[0].v != a.vmax || a.c[1].h != 1 || a.c[1].v != 1 || a.c[2].h != 1 ||
                      a.c[2].v != 1 || (a.hmax == 1 && a.vmax == 2)))
        return why = "unsupported sampling", PSN_LK_ERR_UNSUPPORTED;
    const int mcux = (a.W + 8 * a.hmax - 1) / (8 * a.hmax), mcuy = (a.H + 8 * a.vmax - 1) / (8 * a.vmax);
    int blk = 0, plane = 0;
    for (int c = 0; c < a.nc; c++) {
        psn::CompGeo &g = a.c[c];
        g.bw = a.nc == 1 ? (a.W + 7) / 8 : mcux * g.h;
        g.bh = a.nc == 1 ? (a.H + 7) / 8 : mcuy * g.v;
        g.dw = (int)(((long long)a.W * g.h + a.hmax - 1) / a.hmax);
        g.dh = (int)(((long long)a.H * g.v + a.vmax - 1) / a.vmax);
        g.blk0 = blk;
        g.plane0 = plane;
        blk += g.bw * g.bh;
        plane += g.bw * g.bh * 64;
    }
    a.nblocks = blk;
    a.mcux = a.nc == 1 ? a.c[0].bw : mcux;
    a.nmcu = a.nc == 1 ? a.c[0].bw * a.c[0].bh : mcux * mcuy;
    // entropy data runs to EOI (or the end); restart segments start after each RSTn
    P.seg.assign(1, 0);
    size_t q = P.ent0;
    while (q + 1 < n) {
        if (d[q] == 0xFF && d[q + 1] != 0x00 && d[q + 1] != 0xFF) {
            const int mk = d[q + 1];
            if (mk >= 0xD0 && mk <= 0xD7) {
                if (a.ri) P.seg.push_back((int)(q + 2 - P.ent0));
                P.plain = false;  // a marker inside the entropy bytes
                q += 2;
                continue;
            }
            break;  // EOI or another marker ends the scan
        }
        if (d[q] == 0xFF && d[q + 1] == 0xFF) P.plain = false;  // a fill byte
        q++;
    }
    P.ent1 = q;
    if (P.ent1 > P.ent0 && d[P.ent1 - 1] == 0xFF) P.plain = false;
    const int want = a.ri ? (a.nmcu + a.ri - 1) / a.ri : 1;
    if ((int)P.seg.size() < want) return why = "missing restart markers", PSN_LK_ERR_ARG;
    P.seg.resize((size_t)want);
    a.nseg = want;
    a.data_len = (int)(P.ent1 - P.ent0);
    return PSN_LK_OK;
}

namespace jent = psn::jent;

// Bytes of a workgroup's subsequences are staged in LDS up to this subsequence
// size (256 subsequences + tables + states stay under 64 KiB); larger ones are
// read from global memory.
#ifndef PSN_JPEG_STAGE_MAX_SUB
#define PSN_JPEG_STAGE_MAX_SUB 128
#endif

bool valid_entropy_request(int mode, int sub) {
    return mode >= 0 && mode <= 2 && (sub == 0 || (sub >= jent::kMinSub && sub <= jent::kMaxSub && sub % 4 == 0));
}

// The planner: the parallel path is legal for a plain stream without restart
// intervals, and it is the planner's choice wherever it is legal.
void plan_entropy(const Parsed &P, int mode, int sub, psn_jpeg_plan &pl) {
    memset(&pl, 0, sizeof pl);
    pl.segments = P.a.nseg;
    pl.plain = P.plain ? 1 : 0;
    pl.entropy_bytes = P.a.data_len;
    const bool legal = P.a.ri == 0 && P.plain && P.a.data_len > 0;
    pl.path = mode != 1 && legal ? PSN_JPEG_PATH_PARALLEL : PSN_JPEG_PATH_SERIAL;
    if (pl.path == PSN_JPEG_PATH_PARALLEL) {
        pl.sub_bytes = sub ? sub : PSN_JPEG_DEFAULT_SUB_BYTES;
        pl.subsequences = (P.a.data_len + pl.sub_bytes - 1) / pl.sub_bytes;
        pl.sequences = (pl.subsequences + jent::kSeqLen - 1) / jent::kSeqLen;
    }
}

// The scan's block layout as the symbol step's sinks address it.
void entropy_geometry(const Parsed &P, jent::Geo &G, int &nb0, int &bpm) {
    const psn::JpegArgs &a = P.a;
    memset(&G, 0, sizeof G);
    G.nc = a.nc;
    G.mcux = a.mcux;
    G.nblocks = a.nblocks;
    for (int c = 0; c < a.nc; c++) {
        G.c[c].h = a.nc == 1 ? 1 : a.c[c].h;
        G.c[c].v = a.nc == 1 ? 1 : a.c[c].v;
        G.c[c].bw = a.c[c].bw;
        G.c[c].blk0 = a.c[c].blk0;
    }
    nb0 = G.c[0].h * G.c[0].v;
    bpm = a.nc == 1 ? 1 : nb0 + a.nc - 1;  // chroma is 1x1 (parse())
    G.total = a.nmcu * bpm;
}

// psn_jpeg_entropy_model's decode: the kernels' passes, one after the other.
void model_decode(const Parsed &P, const uint8_t *ent, const psn_jpeg_plan &pl, int16_t *coef, psn_jpeg_stats &S) {
    jent::Geo G;
    int nb0, bpm;
    entropy_geometry(P, G, nb0, bpm);
    std::vector<psn::HuffDev> dc(psn::kJpegMaxComp), ac(psn::kJpegMaxComp);
    for (int c = 0; c < P.a.nc; c++) {
        dc[c] = P.tab.dc[P.a.c[c].td];
        ac[c] = P.tab.ac[P.a.c[c].ta];
    }
    const jent::Tabs T{dc.data(), ac.data(), nb0, bpm};
    const jent::HostBytes src{ent, P.a.data_len};
    const long long total = G.total;
    const unsigned long long kNoEnd = ~0ULL >> 16, kStart = jent::pack(0, 0, 0);
    memset(coef, 0, (size_t)G.nblocks * 64 * sizeof(int16_t));
    if (pl.path == PSN_JPEG_PATH_SERIAL) {
        jent::EmitSink sink(G, T, coef, jent::kNaturalHost, 0);
        jent::run(src, T, kStart, kNoEnd, (total + 1) * 64, sink);
        S.blocks = (int)std::min(sink.g, total);
    } else {
        const int nsub = pl.subsequences, nseq = pl.sequences, K = jent::kSeqLen;
        const long long subbits = 8LL * pl.sub_bytes;
        std::vector<unsigned long long> st((size_t)nsub);
        std::vector<unsigned> cnt((size_t)nsub);
        auto sub = [&](long long i, unsigned long long from, unsigned &blocks) {
            jent::CountSink cs;
            const unsigned long long e = jent::run(src, T, from, (unsigned long long)((i + 1) * subbits), subbits + 1, cs);
            blocks = cs.blocks;
            return e;
        };
        // jpeg_sync_kernel: every thread of a round sees the previous round's exit states
        for (int q = 0; q < nseq; q++) {
            const long long i0 = (long long)q * K;
            const int n = (int)std::min<long long>(K, nsub - i0);
            std::vector<unsigned long long> entry((size_t)n), ex((size_t)n);
            for (int t = 0; t < n; t++) {
                entry[t] = i0 + t ? jent::cold_state(src, (i0 + t) * pl.sub_bytes) : kStart;
                ex[t] = sub(i0 + t, entry[t], cnt[i0 + t]);
            }
            int rounds = 1;
            for (int r = 1; r < K; r++) {
                const std::vector<unsigned long long> prev = ex;
                bool changed = false;
                for (int t = 1; t < n; t++)
                    if (prev[t - 1] != entry[t]) {
                        entry[t] = prev[t - 1];
                        const unsigned long long e = sub(i0 + t, entry[t], cnt[i0 + t]);
                        changed |= e != ex[t];
                        ex[t] = e;
                    }
                rounds++;
                if (!changed) break;
            }
            std::copy(ex.begin(), ex.end(), st.begin() + i0);
            S.sync_rounds = std::max(S.sync_rounds, rounds);
        }
        // jpeg_chain_kernel
        unsigned long long carry = kStart;
        for (int c0 = 0; c0 < nseq; c0 += jent::kChainLen) {
            const int npass = std::min(jent::kChainLen, nseq - c0);
            std::vector<unsigned long long> sx((size_t)npass), walked((size_t)npass, ~0ULL);
            auto last_of = [&](int j) { return std::min<long long>((long long)(j + 1) * K, nsub) - 1; };
            for (int t = 0; t < npass; t++) sx[t] = st[last_of(c0 + t)];
            for (int r = 0; r < npass; r++) {
                const std::vector<unsigned long long> prev = sx;
                bool changed = false;
                for (int t = 0; t < npass; t++) {
                    const int j = c0 + t;
                    const unsigned long long entry = t ? prev[t - 1] : carry;
                    if (j == 0 || entry == walked[t]) continue;
                    unsigned long long cur = entry;
                    bool met = false;
                    for (long long i = (long long)j * K; i <= last_of(j) && !met; i++) {
                        unsigned blocks;
                        cur = sub(i, cur, blocks);
                        met = cur == st[i];
                        st[i] = cur;
                        cnt[i] = blocks;
                    }
                    if (!met && cur != sx[t]) {
                        sx[t] = cur;
                        changed = true;
                    }
                    walked[t] = entry;
                }
                S.chain_rounds++;
                if (!changed) break;
            }
            carry = sx[npass - 1];
        }
        // prefix sum, jpeg_emit_kernel
        long long g0 = 0;
        for (long long i = 0; i < nsub; i++) {
            const bool last = i == nsub - 1;
            jent::EmitSink sink(G, T, coef, jent::kNaturalHost, g0);
            const long long bound = subbits + 1 + (last ? (total - std::min(g0, total) + 1) * 64 : 0);
            jent::run(src, T, i ? st[i - 1] : kStart, last ? kNoEnd : (unsigned long long)((i + 1) * subbits), bound, sink);
            if (last) S.blocks = (int)std::min(sink.g, total);
            g0 += cnt[i];
        }
    }
    // jpeg_dc_kernel: the serial kernel's last_dc[ci] += diff; blk[0] = (int16_t)last_dc[ci]
    for (int c = 0; c < P.a.nc; c++) {
        const long long n = (long long)P.a.nmcu * G.c[c].h * G.c[c].v;
        unsigned last_dc = 0;
        for (long long e = 0; e < n; e++) {
            int16_t &d0 = coef[jent::dc_block(G, c, e) * 64];
            last_dc += (unsigned)(int)d0;
            d0 = (int16_t)(int)last_dc;
        }
    }
}

}  // namespace

extern "C" {

int psn_jpeg_info(const uint8_t *data, size_t len, int *w, int *h, int *comps) {
    if (!data || !w || !h) return PSN_LK_ERR_ARG;
    Parsed P;
    std::string why;
    const int rc = parse(data, len, P, why);
    if (rc) return rc;
    *w = P.a.W;
    *h = P.a.H;
    if (comps) *comps = P.a.nc;
    return PSN_LK_OK;
}

int psn_jpeg_create(int device, psn_jpeg_ctx **out) {
    if (!out) return PSN_LK_ERR_ARG;
    *out = nullptr;
    psn_jpeg_ctx *c = new (std::nothrow) psn_jpeg_ctx();
    if (!c) return PSN_LK_ERR_NOMEM;
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->blob_free, hipEventDisableTiming) != hipSuccess) {
        psn_jpeg_destroy(c);
        return PSN_LK_ERR_HIP;
    }
    c->stream = c->own;
    *out = c;
    return PSN_LK_OK;
}

void psn_jpeg_destroy(psn_jpeg_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (void *p : {(void *)c->d_blob, (void *)c->d_coef, (void *)c->d_planes, (void *)c->d_out, (void *)c->d_par})
        if (p) (void)hipFree(p);
    if (c->h_blob) (void)hipHostFree(c->h_blob);
    if (c->blob_free) (void)hipEventDestroy(c->blob_free);
    if (c->own) (void)hipStreamDestroy(c->own);
    delete c;
}

const char *psn_jpeg_last_error(psn_jpeg_ctx *c) { return c ? c->err.c_str() : "null context"; }

int psn_jpeg_set_stream(psn_jpeg_ctx *c, void *s) {
    if (!c) return PSN_LK_ERR_ARG;
    c->stream = s ? (hipStream_t)s : c->own;
    return PSN_LK_OK;
}

#define JCHK(c, e)                                                                                      \
    do {                                                                                                \
        hipError_t e_ = (e);                                                                            \
        if (e_ != hipSuccess) return jerr((c), PSN_LK_ERR_HIP, "%s: %s", #e, hipGetErrorString(e_));   \
    } while (0)

int psn_jpeg_decode_device(psn_jpeg_ctx *c, const uint8_t *data, size_t len, uint8_t *d_bgr, int stride) {
    if (!c || !data || !d_bgr) return PSN_LK_ERR_ARG;
    Parsed P;
    std::string why;
    int rc = parse(data, len, P, why);
    if (rc) return jerr(c, rc, "%s", why.c_str());
    psn::JpegArgs &a = P.a;
    if (stride < 3 * a.W) return jerr(c, PSN_LK_ERR_ARG, "stride %d < 3 * width %d", stride, a.W);
    JCHK(c, hipSetDevice(c->device));
    const size_t off_seg = (sizeof(psn::Tables) + 15) & ~(size_t)15;
    const size_t off_data = (off_seg + 4 * P.seg.size() + 15) & ~(size_t)15;
    const size_t blob = off_data + (size_t)a.data_len + 16;
    if (c->blob_pending) {  // the staging blob is reused: the previous frame's H2D must be done
        JCHK(c, hipEventSynchronize(c->blob_free));
        c->blob_pending = false;
    }
    if (c->blob_cap < blob) {
        JCHK(c, hipStreamSynchronize(c->stream));
        if (c->d_blob) (void)hipFree(c->d_blob);
        if (c->h_blob) (void)hipHostFree(c->h_blob);
        c->d_blob = c->h_blob = nullptr;
        c->blob_cap = 0;
        const size_t cap = blob + blob / 2;
        JCHK(c, hipMalloc(&c->d_blob, cap));
        JCHK(c, hipHostMalloc(&c->h_blob, cap, hipHostMallocDefault));
        c->blob_cap = cap;
    }
    const size_t coef = (size_t)a.nblocks * 64 * sizeof(int16_t), planes = (size_t)a.nblocks * 64;
    if (c->coef_cap < coef || c->planes_cap < planes) {
        JCHK(c, hipStreamSynchronize(c->stream));
        if (c->d_coef) (void)hipFree(c->d_coef);
        if (c->d_planes) (void)hipFree(c->d_planes);
        c->d_coef = nullptr;
        c->d_planes = nullptr;
        c->coef_cap = c->planes_cap = 0;
        JCHK(c, hipMalloc(&c->d_coef, coef));
        JCHK(c, hipMalloc(&c->d_planes, planes));
        c->coef_cap = coef;
        c->planes_cap = planes;
    }
    memcpy(c->h_blob, &P.tab, sizeof(psn::Tables));
    memcpy(c->h_blob + off_seg, P.seg.data(), 4 * P.seg.size());
    memcpy(c->h_blob + off_data, data + P.ent0, (size_t)a.data_len);
    JCHK(c, hipMemcpyAsync(c->d_blob, c->h_blob, blob, hipMemcpyHostToDevice, c->stream));
    JCHK(c, hipEventRecord(c->blob_free, c->stream));
    c->blob_pending = true;
    JCHK(c, hipMemsetAsync(c->d_coef, 0, coef, c->stream));
    a.tab = (const psn::Tables *)c->d_blob;
    a.seg = (const int *)(c->d_blob + off_seg);
    a.data = c->d_blob + off_data;
    a.coef = c->d_coef;
    a.planes = c->d_planes;
    a.out = d_bgr;
    a.out_stride = stride;
    psn_jpeg_plan pl;
    plan_entropy(P, c->ent_mode, c->ent_sub, pl);
    c->last = psn_jpeg_stats{pl.path, pl.segments, pl.sub_bytes, pl.subsequences, pl.sequences, 0, 0, 0};
    c->decoded = true;
    c->last_nblocks = a.nblocks;
    if (pl.path == PSN_JPEG_PATH_PARALLEL) {
        const size_t nsub = (size_t)pl.subsequences, nseq = (size_t)pl.sequences;
        auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
        const size_t off_st = up16(sizeof(psn::DevStats)), off_cnt = off_st + up16(8 * nsub), off_pre = off_cnt + up16(4 * nsub),
                     off_rounds = off_pre + up16(4 * nsub), par = off_rounds + up16(4 * nseq);
        if (c->par_cap < par) {
            JCHK(c, hipStreamSynchronize(c->stream));
            if (c->d_par) (void)hipFree(c->d_par);
            c->d_par = nullptr;
            c->par_cap = 0;
            JCHK(c, hipMalloc(&c->d_par, par + par / 2));
            c->par_cap = par + par / 2;
        }
        psn::EntArgs e{};
        e.tab = a.tab;
        e.data = a.data;
        e.len = a.data_len;
        e.S = pl.sub_bytes;
        e.nsub = pl.subsequences;
        e.nseq = pl.sequences;
        e.stage = pl.sub_bytes <= PSN_JPEG_STAGE_MAX_SUB ? 1 : 0;
        entropy_geometry(P, e.geo, e.nb0, e.bpm);
        e.nmcu = a.nmcu;
        for (int i = 0; i < a.nc; i++) {
            e.td[i] = a.c[i].td;
            e.ta[i] = a.c[i].ta;
        }
        e.stats = (psn::DevStats *)c->d_par;
        e.st = (unsigned long long *)(c->d_par + off_st);
        e.cnt = (unsigned *)(c->d_par + off_cnt);
        e.pre = (unsigned *)(c->d_par + off_pre);
        e.seq_rounds = (int *)(c->d_par + off_rounds);
        e.coef = a.coef;
        const size_t staged = e.stage ? (size_t)jent::kSeqLen * e.S + psn::kStageSlack : 0;
        const size_t lds_sync = sizeof(psn::LdsTabs) + jent::kSeqLen * 8 + staged, lds_emit = sizeof(psn::LdsTabs) + psn::kNaturalLds + staged;
        hipLaunchKernelGGL(psn::jpeg_sync_kernel, dim3(e.nseq), dim3(jent::kSeqLen), lds_sync, c->stream, e);
        JCHK(c, hipGetLastError());
        hipLaunchKernelGGL(psn::jpeg_chain_kernel, dim3(1), dim3(1024), 0, c->stream, e);
        JCHK(c, hipGetLastError());
        hipLaunchKernelGGL(psn::jpeg_emit_kernel, dim3(e.nseq), dim3(jent::kSeqLen), lds_emit, c->stream, e);
        JCHK(c, hipGetLastError());
        hipLaunchKernelGGL(psn::jpeg_dc_kernel, dim3(a.nc), dim3(1024), 0, c->stream, e);
        JCHK(c, hipGetLastError());
    } else {
        c->last.blocks = a.nblocks;  // the serial kernel decodes every block of the scan
        hipLaunchKernelGGL(psn::jpeg_entropy_kernel, dim3((a.nseg + 63) / 64), dim3(64), 0, c->stream, a);
        JCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(psn::jpeg_idct_kernel, dim3((a.nblocks + 255) / 256), dim3(256), 0, c->stream, a);
    JCHK(c, hipGetLastError());
    hipLaunchKernelGGL(psn::jpeg_color_kernel, dim3((a.W + 255) / 256, a.H), dim3(256), 0, c->stream, a);
    JCHK(c, hipGetLastError());
    return PSN_LK_OK;
}

int psn_jpeg_decode(psn_jpeg_ctx *c, const uint8_t *data, size_t len, uint8_t *bgr, int stride) {
    if (!c || !data || !bgr) return PSN_LK_ERR_ARG;
    int w = 0, h = 0;
    int rc = psn_jpeg_info(data, len, &w, &h, nullptr);
    if (rc) return jerr(c, rc, "bad JPEG headers");
    if (stride < 3 * w) return jerr(c, PSN_LK_ERR_ARG, "stride %d < 3 * width %d", stride, w);
    JCHK(c, hipSetDevice(c->device));
    const size_t need = (size_t)w * 3 * h;
    if (c->out_cap < need) {
        JCHK(c, hipStreamSynchronize(c->stream));
        if (c->d_out) (void)hipFree(c->d_out);
        c->d_out = nullptr;
        c->out_cap = 0;
        JCHK(c, hipMalloc(&c->d_out, need));
        c->out_cap = need;
    }
    rc = psn_jpeg_decode_device(c, data, len, c->d_out, 3 * w);
    if (rc) return rc;
    JCHK(c, hipMemcpy2DAsync(bgr, stride, c->d_out, 3 * (size_t)w, 3 * (size_t)w, h, hipMemcpyDeviceToHost, c->stream));
    JCHK(c, hipStreamSynchronize(c->stream));
    return PSN_LK_OK;
}

int psn_jpeg_entropy_plan(const uint8_t *data, size_t len, psn_jpeg_plan *out) {
    if (!data || !out) return PSN_LK_ERR_ARG;
    Parsed P;
    std::string why;
    const int rc = parse(data, len, P, why);
    if (rc) return rc;
    plan_entropy(P, 0, 0, *out);
    return PSN_LK_OK;
}

int psn_jpeg_debug_set_entropy(psn_jpeg_ctx *c, int mode, int sub_bytes) {
    if (!c) return PSN_LK_ERR_ARG;
    if (!valid_entropy_request(mode, sub_bytes))
        return jerr(c, PSN_LK_ERR_ARG, "entropy mode %d (0..2), sub_bytes %d (0 or a multiple of 4 in [4, 1024])", mode, sub_bytes);
    c->ent_mode = mode;
    c->ent_sub = sub_bytes;
    return PSN_LK_OK;
}

int psn_jpeg_debug_read_coefficients(psn_jpeg_ctx *c, int16_t *out, size_t count) {
    if (!c || !out) return PSN_LK_ERR_ARG;
    if (!c->decoded) return jerr(c, PSN_LK_ERR_ARG, "nothing decoded yet");
    if (count != (size_t)c->last_nblocks * 64)
        return jerr(c, PSN_LK_ERR_ARG, "count %zu is not %d blocks * 64", count, c->last_nblocks);
    JCHK(c, hipSetDevice(c->device));
    JCHK(c, hipMemcpyAsync(out, c->d_coef, count * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
    JCHK(c, hipStreamSynchronize(c->stream));
    return PSN_LK_OK;
}

int psn_jpeg_last_stats(psn_jpeg_ctx *c, psn_jpeg_stats *out) {
    if (!c || !out) return PSN_LK_ERR_ARG;
    if (!c->decoded) return jerr(c, PSN_LK_ERR_ARG, "nothing decoded yet");
    JCHK(c, hipSetDevice(c->device));
    JCHK(c, hipStreamSynchronize(c->stream));
    *out = c->last;
    if (c->last.path == PSN_JPEG_PATH_PARALLEL) {
        psn::DevStats d;
        JCHK(c, hipMemcpy(&d, c->d_par, sizeof d, hipMemcpyDeviceToHost));
        out->sync_rounds = d.sync_rounds;
        out->chain_rounds = d.chain_rounds;
        out->blocks = d.blocks;
    }
    return PSN_LK_OK;
}

int psn_jpeg_entropy_model(const uint8_t *data, size_t len, int mode, int sub_bytes, int16_t *coef, psn_jpeg_stats *stats) {
    if (!data || !stats || !valid_entropy_request(mode, sub_bytes)) return PSN_LK_ERR_ARG;
    Parsed P;
    std::string why;
    const int rc = parse(data, len, P, why);
    if (rc) return rc;
    if (P.a.ri != 0 || !P.plain) return PSN_LK_ERR_UNSUPPORTED;
    psn_jpeg_plan pl;
    plan_entropy(P, mode, sub_bytes, pl);
    *stats = psn_jpeg_stats{pl.path, pl.segments, pl.sub_bytes, pl.subsequences, pl.sequences, 0, 0, P.a.nblocks};
    if (!coef) return PSN_LK_OK;
    stats->blocks = 0;
    model_decode(P, data + P.ent0, pl, coef, *stats);
    return PSN_LK_OK;
}

}  // extern "C"
