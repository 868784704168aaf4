// JPEG frame ingest on the device (include/psn_jpeg.h): the libjpeg baseline
// decode behind cv::imread (psn_where/main.cpp:144), restated for gfx950.
//
//   host   markers -> quantisation tables (natural order), Huffman tables
//          (canonical maxcode/valoffset + a 9-bit lookahead table), component
//          geometry, restart-segment byte offsets (RSTn positions); one pinned
//          staging block (its layout: "items" below) -> one H2D
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
//   items  every decode is a batch (psn_jpeg_decode_batch_device; a single image,
//          psn_jpeg_decode_device, is a batch of one): each kernel has one entry,
//          which reads its item's arguments from a device table, the item index
//          in the grid; one blob
//          [per item: tables | segment offsets | entropy bytes + 16 zeroed bytes]
//          [EntArgs table | JpegArgs table | parallel list | serial list], one
//          H2D, one memset, one launch per kernel whatever the item count
// Bit-identical to oracle/jpeg_oracle.c, which is pinned to libjpeg-turbo.
//
// This unit: the kernels with their device-only structs, the decoder context,
// the launches and the entries of the ABI that touch the device. The host side
// that needs no device is plain C++ beside it: psn_jpeg_parse.h / .cpp (marker
// parser, Huffman table builder, entropy planner, the kernels' argument structs;
// psn_jpeg_info, psn_jpeg_entropy_plan) and psn_jpeg_model.cpp (the CPU model of
// the parallel path, psn_jpeg_entropy_model).
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

#include "psn_jpeg_parse.h"  // Tables, CompGeo, JpegArgs, Parsed, parse(), the planner

namespace psn {
namespace {

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

// Every kernel's body is a device function over one item's argument struct and
// the item's own indices; the entry (the end of the namespace) passes it the
// item's arguments from a device table.
__device__ __forceinline__ void entropy_body(const JpegArgs &A, int group) {
    const int s = group * blockDim.x + threadIdx.x;
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
// the first symbol boundary at or past its end. (EntArgs, DevStats: psn_jpeg_parse.h.)

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
__device__ __forceinline__ DevBytes stage_bytes(const EntArgs &E, int seq, uint8_t *sb) {
    DevBytes src{sb, 0, 0, E.data, E.len};
    if (E.stage) {
        src.w0 = (long long)seq * jent::kSeqLen * E.S;
        src.w1 = min(src.w0 + (long long)jent::kSeqLen * E.S + kStageSlack, E.len);
        const int nd = (int)((src.w1 - src.w0 + 3) / 4);  // the last dword may read past len: inside the item's own slack
        const uint32_t *s = (const uint32_t *)(E.data + src.w0);
        for (int k = threadIdx.x; k < nd; k += blockDim.x) ((uint32_t *)sb)[k] = s[k];
    }
    return src;
}

__device__ __forceinline__ void sync_body(const EntArgs &E, int seq, uint8_t *smem) {
    LdsTabs &L = *(LdsTabs *)smem;
    unsigned long long *sx = (unsigned long long *)(smem + sizeof(LdsTabs));  // exit state per thread
    stage_tables(E, L);
    const DevBytes src = stage_bytes(E, seq, smem + sizeof(LdsTabs) + jent::kSeqLen * 8);
    __syncthreads();
    const jent::Tabs T{L.dc, L.ac, E.nb0, E.bpm};
    const int t = threadIdx.x;
    const long long i = (long long)seq * jent::kSeqLen + t;
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
    if (t == 0) E.seq_rounds[seq] = rounds;
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

__device__ __forceinline__ void chain_body(const EntArgs &E) {
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

__device__ __forceinline__ void emit_body(const EntArgs &E, int seq, uint8_t *smem) {
    LdsTabs &L = *(LdsTabs *)smem;
    uint8_t *snat = smem + sizeof(LdsTabs);  // the natural-order table: a divergent lookup per coefficient
    stage_tables(E, L);
    if (threadIdx.x < 64 + 16) snat[threadIdx.x] = jent::kNaturalDev[threadIdx.x];
    const DevBytes src = stage_bytes(E, seq, smem + sizeof(LdsTabs) + kNaturalLds);
    __syncthreads();
    const long long i = (long long)seq * jent::kSeqLen + threadIdx.x;
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

__device__ __forceinline__ void dc_body(const EntArgs &E, int ci) {
    __shared__ unsigned ws[16];
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

__device__ __forceinline__ void idct_body(const JpegArgs &A, int group) {
    const int b = group * blockDim.x + threadIdx.x;
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

__device__ __forceinline__ void color_body(const JpegArgs &A, int group, int y) {
    const int x = group * blockDim.x + threadIdx.x;
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

// ---------------------------------------------------------------- entries
// One launch per kernel for all items of a decode. The item is blockIdx.y
// (blockIdx.z for the colour kernel, whose y is the row); the entropy kernels take
// it through the index list of their path. The item's arguments are read from a
// device table -- the index is uniform, so these are scalar loads, as
// kernel-argument loads are. The grid is the maximum over the items: a workgroup
// past its own item's extent returns whole, before any barrier of the body (with
// one item the grid is that item's extent).

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const JpegArgs *__restrict__ tab, const int *__restrict__ list) {
    const JpegArgs &A = tab[list[blockIdx.y]];
    if ((int)blockIdx.x >= (A.nseg + 63) / 64) return;
    entropy_body(A, blockIdx.x);
}

__global__ __launch_bounds__(256) void jpeg_sync_kernel(const EntArgs *__restrict__ tab, const int *__restrict__ list) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const EntArgs &E = tab[list[blockIdx.y]];
    if ((int)blockIdx.x >= E.nseq) return;
    sync_body(E, blockIdx.x, smem);
}

__global__ __launch_bounds__(1024) void jpeg_chain_kernel(const EntArgs *__restrict__ tab, const int *__restrict__ list) {
    chain_body(tab[list[blockIdx.y]]);  // one workgroup per item
}

__global__ __launch_bounds__(256) void jpeg_emit_kernel(const EntArgs *__restrict__ tab, const int *__restrict__ list) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const EntArgs &E = tab[list[blockIdx.y]];
    if ((int)blockIdx.x >= E.nseq) return;
    emit_body(E, blockIdx.x, smem);
}

__global__ __launch_bounds__(1024) void jpeg_dc_kernel(const EntArgs *__restrict__ tab, const int *__restrict__ list) {
    const EntArgs &E = tab[list[blockIdx.y]];
    if ((int)blockIdx.x >= E.geo.nc) return;
    dc_body(E, blockIdx.x);  // one workgroup per item and component
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpegArgs *__restrict__ tab) {
    const JpegArgs &A = tab[blockIdx.y];
    if ((int)blockIdx.x >= (A.nblocks + 255) / 256) return;
    idct_body(A, blockIdx.x);
}

__global__ __launch_bounds__(256) void jpeg_color_kernel(const JpegArgs *__restrict__ tab) {
    const JpegArgs &A = tab[blockIdx.z];
    if ((int)blockIdx.x >= (A.W + 255) / 256 || (int)blockIdx.y >= A.H) return;
    color_body(A, blockIdx.x, blockIdx.y);
}

}  // namespace
}  // namespace psn

struct psn_jpeg_ctx {
    int device = 0;
    hipStream_t own = nullptr, stream = nullptr;
    uint8_t *d_blob = nullptr, *h_blob = nullptr;  // the staging blob (psn::plan_batch lays it out)
    size_t blob_cap = 0;
    int16_t *d_coef = nullptr;
    size_t coef_cap = 0;
    uint8_t *d_planes = nullptr;
    size_t planes_cap = 0;
    hipEvent_t blob_free = nullptr;  // the previous decode's H2D has read the staging blob
    bool blob_pending = false;
    uint8_t *d_out = nullptr;  // psn_jpeg_decode's device BGR buffer
    size_t out_cap = 0;
    int ent_mode = 0, ent_sub = 0;  // psn_jpeg_debug_set_entropy
    uint8_t *d_par = nullptr;       // per item: [DevStats | states | counts | prefix sums | rounds]
    size_t par_cap = 0;
    struct BatchItem {              // one item of the last decode (the stats and coefficient readers)
        psn_jpeg_stats st;          // host part; a parallel item's counters are its DevStats in d_par
        int nblocks;
        size_t stats_off, coef_off;  // its DevStats in d_par, its coefficients in d_coef (bytes)
    };
    std::vector<BatchItem> items;    // the last decode; empty: nothing decoded yet
    bool batch = false;             // it came in through psn_jpeg_decode_batch_device
    std::string err;
};

namespace {

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

#define JCHK(c, e)                                                                                      \
    do {                                                                                                \
        hipError_t e_ = (e);                                                                            \
        if (e_ != hipSuccess) return jerr((c), PSN_LK_ERR_HIP, "%s: %s", #e, hipGetErrorString(e_));   \
    } while (0)

// A device buffer of the context (with its pinned twin, if it has one) grown to
// `to` bytes where it holds fewer than `need`: waits for the stream's work on the
// old buffer first. After a failed allocation the pointer is null, the capacity 0.
template <class T>
int grow(psn_jpeg_ctx *c, T *&buf, size_t &cap, size_t need, size_t to, T **pinned = nullptr) {
    if (cap >= need) return PSN_LK_OK;
    JCHK(c, hipStreamSynchronize(c->stream));
    if (buf) (void)hipFree(buf);
    if (pinned && *pinned) (void)hipHostFree(*pinned);
    buf = nullptr;
    if (pinned) *pinned = nullptr;
    cap = 0;
    JCHK(c, hipMalloc(&buf, to));
    if (pinned) JCHK(c, hipHostMalloc(pinned, to, hipHostMallocDefault));
    cap = to;
    return PSN_LK_OK;
}

namespace jent = psn::jent;

// The one decode: psn_jpeg_decode_batch_device's items, or psn_jpeg_decode_device's
// image as a batch of one (`batch` false: its errors name no item).
int decode_items(psn_jpeg_ctx *c, const psn_jpeg_item *items, int n, bool batch) {
    psn::Batch B;
    std::string why;
    int rc = psn::plan_batch(items, n, c->ent_mode, c->ent_sub, B, why);  // every item, before anything is enqueued
    if (rc && batch && B.L.bad_item >= 0) return jerr(c, rc, "item %d: %s", B.L.bad_item, why.c_str());
    if (rc) return jerr(c, rc, "%s", why.c_str());
    const psn_jpeg_batch_layout &L = B.L;
    JCHK(c, hipSetDevice(c->device));
    if (c->blob_pending) {  // the staging blob is reused: the previous decode's H2D must be done
        JCHK(c, hipEventSynchronize(c->blob_free));
        c->blob_pending = false;
    }
    if ((rc = grow(c, c->d_blob, c->blob_cap, L.blob_size, L.blob_size + L.blob_size / 2, &c->h_blob))) return rc;
    if ((rc = grow(c, c->d_coef, c->coef_cap, L.coef_size, L.coef_size))) return rc;
    if ((rc = grow(c, c->d_planes, c->planes_cap, L.planes_size, L.planes_size))) return rc;
    if ((rc = grow(c, c->d_par, c->par_cap, L.scratch_size, L.scratch_size + L.scratch_size / 2))) return rc;
    psn::EntArgs *he = (psn::EntArgs *)(c->h_blob + L.ent_args);
    psn::JpegArgs *ha = (psn::JpegArgs *)(c->h_blob + L.jpeg_args);
    int *hl = (int *)(c->h_blob + L.lists);
    std::vector<psn_jpeg_ctx::BatchItem> rec((size_t)n);
    int sub = 0;  // the parallel items' subsequence size: one per context
    for (int i = 0; i < n; i++) {
        const psn::Parsed &P = B.P[(size_t)i];
        const psn_jpeg_batch_item_layout &it = L.item[i];
        const psn_jpeg_plan &pl = B.plans[(size_t)i];
        memcpy(c->h_blob + it.tables, &P.tab, sizeof(psn::Tables));
        memcpy(c->h_blob + it.segments, P.seg.data(), 4 * P.seg.size());
        memcpy(c->h_blob + it.bytes, items[i].data + P.ent0, (size_t)P.a.data_len);
        memset(c->h_blob + it.bytes + P.a.data_len, 0, it.bytes_size - (size_t)P.a.data_len);  // the item's slack
        psn::batch_args(B, i, items[i], c->d_blob, c->d_par, (uint8_t *)c->d_coef, c->d_planes, ha[i], he[i]);
        rec[(size_t)i] = {psn_jpeg_stats{pl.path, pl.segments, pl.sub_bytes, pl.subsequences, pl.sequences, 0, 0,
                                         pl.path == PSN_JPEG_PATH_PARALLEL ? 0 : P.a.nblocks},
                          P.a.nblocks, it.stats, it.coef};
        if (pl.path == PSN_JPEG_PATH_PARALLEL) sub = pl.sub_bytes;
    }
    for (int k = 0; k < L.n_parallel; k++) hl[k] = L.parallel[k];
    for (int k = 0; k < L.n_serial; k++) hl[n + k] = L.serial[k];
    JCHK(c, hipMemcpyAsync(c->d_blob, c->h_blob, L.blob_size, hipMemcpyHostToDevice, c->stream));
    JCHK(c, hipEventRecord(c->blob_free, c->stream));
    c->blob_pending = true;
    JCHK(c, hipMemsetAsync(c->d_coef, 0, L.coef_size, c->stream));
    c->items = rec;  // a call refused above left the records of the last decode as they were
    c->batch = batch;
    const psn::EntArgs *de = (const psn::EntArgs *)(c->d_blob + L.ent_args);
    const psn::JpegArgs *da = (const psn::JpegArgs *)(c->d_blob + L.jpeg_args);
    const int *dl = (const int *)(c->d_blob + L.lists);
    if (L.n_parallel) {
        const size_t staged = sub <= PSN_JPEG_STAGE_MAX_SUB ? (size_t)jent::kSeqLen * sub + psn::kStageSlack : 0;
        const size_t lds_sync = sizeof(psn::LdsTabs) + jent::kSeqLen * 8 + staged, lds_emit = sizeof(psn::LdsTabs) + psn::kNaturalLds + staged;
        const dim3 seqs(L.max_sequences, L.n_parallel);
        hipLaunchKernelGGL(psn::jpeg_sync_kernel, seqs, dim3(jent::kSeqLen), lds_sync, c->stream, de, dl);
        JCHK(c, hipGetLastError());
        hipLaunchKernelGGL(psn::jpeg_chain_kernel, dim3(1, L.n_parallel), dim3(1024), 0, c->stream, de, dl);
        JCHK(c, hipGetLastError());
        hipLaunchKernelGGL(psn::jpeg_emit_kernel, seqs, dim3(jent::kSeqLen), lds_emit, c->stream, de, dl);
        JCHK(c, hipGetLastError());
        hipLaunchKernelGGL(psn::jpeg_dc_kernel, dim3(L.max_parallel_components, L.n_parallel), dim3(1024), 0, c->stream, de, dl);
        JCHK(c, hipGetLastError());
    }
    if (L.n_serial) {
        hipLaunchKernelGGL(psn::jpeg_entropy_kernel, dim3(L.max_segment_groups, L.n_serial), dim3(64), 0, c->stream, da, dl + n);
        JCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(psn::jpeg_idct_kernel, dim3(L.max_block_groups, n), dim3(256), 0, c->stream, da);
    JCHK(c, hipGetLastError());
    hipLaunchKernelGGL(psn::jpeg_color_kernel, dim3((L.max_width + 255) / 256, L.max_height, n), dim3(256), 0, c->stream, da);
    JCHK(c, hipGetLastError());
    return PSN_LK_OK;
}

// Item `item` of the last decode where that was a batch; else null, the reason in the context.
const psn_jpeg_ctx::BatchItem *batch_item(psn_jpeg_ctx *c, int item) {
    const size_t n = c->batch ? c->items.size() : 0;
    if (item >= 0 && (size_t)item < n) return &c->items[(size_t)item];
    jerr(c, PSN_LK_ERR_ARG, "item %d: the last decode was %s", item, n ? "a smaller batch" : "not a batch");
    return nullptr;
}

int item_stats(psn_jpeg_ctx *c, const psn_jpeg_ctx::BatchItem &b, psn_jpeg_stats *out) {
    JCHK(c, hipSetDevice(c->device));
    JCHK(c, hipStreamSynchronize(c->stream));
    *out = b.st;
    if (b.st.path == PSN_JPEG_PATH_PARALLEL) {
        psn::DevStats d;
        JCHK(c, hipMemcpy(&d, c->d_par + b.stats_off, sizeof d, hipMemcpyDeviceToHost));
        out->sync_rounds = d.sync_rounds;
        out->chain_rounds = d.chain_rounds;
        out->blocks = d.blocks;
    }
    return PSN_LK_OK;
}

int item_coefficients(psn_jpeg_ctx *c, const psn_jpeg_ctx::BatchItem &b, int16_t *out, size_t count) {
    if (count != (size_t)b.nblocks * 64) return jerr(c, PSN_LK_ERR_ARG, "count %zu is not %d blocks * 64", count, b.nblocks);
    JCHK(c, hipSetDevice(c->device));
    JCHK(c, hipMemcpyAsync(out, (const uint8_t *)c->d_coef + b.coef_off, count * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
    JCHK(c, hipStreamSynchronize(c->stream));
    return PSN_LK_OK;
}

}  // namespace

extern "C" {

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

int psn_jpeg_decode_device(psn_jpeg_ctx *c, const uint8_t *data, size_t len, uint8_t *d_bgr, int stride) {
    if (!c || !data || !d_bgr) return PSN_LK_ERR_ARG;
    const psn_jpeg_item item{data, len, d_bgr, stride};
    return decode_items(c, &item, 1, false);
}

int psn_jpeg_decode(psn_jpeg_ctx *c, const uint8_t *data, size_t len, uint8_t *bgr, int stride) {
    if (!c || !data || !bgr) return PSN_LK_ERR_ARG;
    int w = 0, h = 0;
    int rc = psn_jpeg_info(data, len, &w, &h, nullptr);
    if (rc) return jerr(c, rc, "bad JPEG headers");
    if (stride < 3 * w) return jerr(c, PSN_LK_ERR_ARG, "stride %d < 3 * width %d", stride, w);
    JCHK(c, hipSetDevice(c->device));
    const size_t need = (size_t)w * 3 * h;
    if ((rc = grow(c, c->d_out, c->out_cap, need, need))) return rc;
    rc = psn_jpeg_decode_device(c, data, len, c->d_out, 3 * w);
    if (rc) return rc;
    JCHK(c, hipMemcpy2DAsync(bgr, stride, c->d_out, 3 * (size_t)w, 3 * (size_t)w, h, hipMemcpyDeviceToHost, c->stream));
    JCHK(c, hipStreamSynchronize(c->stream));
    return PSN_LK_OK;
}

int psn_jpeg_decode_batch_device(psn_jpeg_ctx *c, const psn_jpeg_item *items, int n) {
    if (!c) return PSN_LK_ERR_ARG;
    return decode_items(c, items, n, true);
}

int psn_jpeg_batch_stats(psn_jpeg_ctx *c, int item, psn_jpeg_stats *out) {
    if (!c || !out) return PSN_LK_ERR_ARG;
    const psn_jpeg_ctx::BatchItem *b = batch_item(c, item);
    return b ? item_stats(c, *b, out) : PSN_LK_ERR_ARG;
}

int psn_jpeg_debug_read_batch_coefficients(psn_jpeg_ctx *c, int item, int16_t *out, size_t count) {
    if (!c || !out) return PSN_LK_ERR_ARG;
    const psn_jpeg_ctx::BatchItem *b = batch_item(c, item);
    return b ? item_coefficients(c, *b, out, count) : PSN_LK_ERR_ARG;
}

int psn_jpeg_debug_set_entropy(psn_jpeg_ctx *c, int mode, int sub_bytes) {
    if (!c) return PSN_LK_ERR_ARG;
    if (!psn::valid_entropy_request(mode, sub_bytes))
        return jerr(c, PSN_LK_ERR_ARG, "entropy mode %d (0..2), sub_bytes %d (0 or a multiple of 4 in [4, 1024])", mode, sub_bytes);
    c->ent_mode = mode;
    c->ent_sub = sub_bytes;
    return PSN_LK_OK;
}

int psn_jpeg_debug_read_coefficients(psn_jpeg_ctx *c, int16_t *out, size_t count) {
    if (!c || !out) return PSN_LK_ERR_ARG;
    if (c->items.empty()) return jerr(c, PSN_LK_ERR_ARG, "nothing decoded yet");
    return item_coefficients(c, c->items.back(), out, count);
}

int psn_jpeg_last_stats(psn_jpeg_ctx *c, psn_jpeg_stats *out) {
    if (!c || !out) return PSN_LK_ERR_ARG;
    if (c->items.empty()) return jerr(c, PSN_LK_ERR_ARG, "nothing decoded yet");
    return item_stats(c, c->items.back(), out);
}

}  // extern "C"
