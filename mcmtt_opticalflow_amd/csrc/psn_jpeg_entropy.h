// One symbol of the baseline-JPEG entropy decode, written once for the host and
// the device: the CPU model (psn_jpeg_entropy_model, psn_jpeg_model.cpp) and the
// parallel kernels of psn_jpeg.hip (jpeg_sync_kernel, jpeg_chain_kernel,
// jpeg_emit_kernel) run these functions, so a state the model reaches is the
// state a kernel reaches.
//
// They read a *plain* stream: inside the entropy bytes every 0xFF is followed by
// 0x00 and the last byte is not 0xFF -- no fill bytes, no embedded marker. A 0x00
// after a 0xFF is then always stuffing, so a reader can start at any byte offset
// (it skips a leading stuffed zero by looking one byte back), and on such a
// stream the reader below yields the bits of jpeg_entropy_kernel's BitReader.
//
// Decoder state: (pos, b, zz) packed into one 64-bit word.
//   pos  bit position from the first entropy byte, in the stuffed stream; never
//        inside a stuffed zero (leaving a 0xFF byte skips the zero after it)
//   b    block index within the MCU (selects the component's DC / AC tables)
//   zz   coefficient index; 0: the next symbol is a DC size
// One symbol is a pure function of that state and the bytes. Past the end of the
// data the reader feeds zeros, as the serial reader does for a truncated file.
#ifndef PSN_JPEG_ENTROPY_H
#define PSN_JPEG_ENTROPY_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PSN_JENT_HD __host__ __device__
#else
#define PSN_JENT_HD
#endif

namespace psn {

struct HuffDev {            // one Huffman table (jdhuff.c d_derived_tbl)
    int maxcode[18];        // largest code of length l, -1 if none; [17] sentinel
    int valoff[18];         // vals index = code + valoff[l]
    uint16_t fast[512];     // 9-bit lookahead: (len << 8) | value, 0 = longer code
    uint8_t vals[256];
};

namespace jent {

constexpr int kMaxComp = 3;
constexpr int kSeqLen = 256;      // subsequences per sequence (one jpeg_sync_kernel workgroup)
constexpr int kChainLen = 1024;   // sequences per jpeg_chain_kernel pass
constexpr int kMinSub = 4, kMaxSub = 1024;  // subsequence bytes, a multiple of 4

// zigzag -> natural order, with the 16 guard entries a run past 63 lands in
#define PSN_JENT_NATURAL_INIT                                                                       \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,       \
     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,       \
     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,               \
     63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63}
#if defined(__HIPCC__)
static __constant__ uint8_t kNaturalDev[64 + 16] = PSN_JENT_NATURAL_INIT;  // the kernels copy it into LDS
#endif
static const uint8_t kNaturalHost[64 + 16] = PSN_JENT_NATURAL_INIT;

// The compiler builtin for host and device: HIP's __popcll wraps the same builtin,
// and a unit that includes no HIP header has no __popcll when it is built as HIP.
PSN_JENT_HD inline int popc64(uint64_t x) { return __builtin_popcountll(x); }

PSN_JENT_HD inline uint64_t pack(uint64_t pos, int b, int zz) { return (pos << 16) | ((uint64_t)b << 8) | (uint64_t)zz; }
PSN_JENT_HD inline uint64_t state_pos(uint64_t s) { return s >> 16; }
PSN_JENT_HD inline int state_b(uint64_t s) { return (int)((s >> 8) & 255); }
PSN_JENT_HD inline int state_zz(uint64_t s) { return (int)(s & 255); }

// The scan's tables by component and the MCU's block layout: blocks 0..nb0-1 of an
// MCU are component 0's, each later block is one further component's (parse() of
// psn_jpeg_parse.cpp admits 1x1 chroma only; a one-component scan has one block
// per MCU).
struct Tabs {
    const HuffDev *dc, *ac;   // [component]
    int nb0, bpm;             // component 0's blocks per MCU, all blocks per MCU
};
PSN_JENT_HD inline int comp_of_block(const Tabs &T, int b) { return b < T.nb0 ? 0 : b - T.nb0 + 1; }

// Bytes of the stream by index, zeros from `len` on.
struct HostBytes {
    const uint8_t *p;
    long long len;
    PSN_JENT_HD unsigned operator()(long long i) const { return i < len ? p[i] : 0u; }
};

// Bit reader of a plain stream. `buf` holds unstuffed bits, `mk` one mark per
// buffered 0xFF byte (at its last bit), `rp` the next byte to load; the position
// of the next unread bit in the stuffed stream follows from the three.
template <class Src>
struct Reader {
    const Src &src;
    unsigned long long buf, mk;
    long long rp;
    int n;
    PSN_JENT_HD explicit Reader(const Src &s) : src(s), buf(0), mk(0), rp(0), n(0) {}
    PSN_JENT_HD void fill() {
        while (n <= 56) {
            const unsigned c = src(rp);
            rp++;
            unsigned long long m = 0;
            if (c == 0xFF) {  // plain stream: the next byte is its stuffed zero
                rp++;
                m = 1;
            }
            buf |= (unsigned long long)c << (56 - n);
            mk |= m << (56 - n);
            n += 8;
        }
    }
    PSN_JENT_HD void init(uint64_t pos) {
        buf = mk = 0;
        n = 0;
        rp = (long long)(pos >> 3);
        fill();
        skip((int)(pos & 7));
    }
    PSN_JENT_HD uint64_t pos() const { return (uint64_t)(rp * 8 - n - 8 * popc64(mk)); }
    // step() fills once per symbol: a symbol reads at most 16 + 15 (a code no length accepts: 17) of the >= 57 bits
    PSN_JENT_HD unsigned peek(int k) const { return (unsigned)(buf >> (64 - k)); }
    PSN_JENT_HD void skip(int k) {
        buf <<= k;
        mk <<= k;
        n -= k;
    }
    PSN_JENT_HD int bits(int k) {
        if (k == 0) return 0;
        const unsigned v = peek(k);
        skip(k);
        return (int)v;
    }
    PSN_JENT_HD int decode(const HuffDev &h) {
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
        // a code no length accepts: jpeg_huff_decode has read a 17th bit by the time
        // its sentinel maxcode[17] ends the search; value 0
        skip(17);
        return 0;
    }
};

PSN_JENT_HD inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// The state a decoder starts from at byte offset `o` knowing nothing: block 0 of
// the MCU, DC next, past a stuffed zero.
template <class Src>
PSN_JENT_HD inline uint64_t cold_state(const Src &src, long long o) {
    if (o > 0 && src(o) == 0 && src(o - 1) == 0xFF) o++;
    return pack((uint64_t)o * 8, 0, 0);
}

// One symbol of the block state machine (the body of jpeg_entropy_kernel's block
// loop). sink.coef(k, v) receives coefficient v at zigzag index k (k == 0: the DC
// *difference*; k up to 63 + 15, the guard entries of the natural-order table);
// returns true when the symbol completes its block.
template <class Src, class Sink>
PSN_JENT_HD inline bool step(Reader<Src> &rd, const Tabs &T, int b, int &zz, Sink &sink) {
    // the lanes of a wave sit in different symbols: one fill, one lookup and one
    // bit read for both symbol kinds, so a wave does not run a DC and an AC copy
    const int ci = comp_of_block(T, b);
    const bool dc = zz == 0;
    rd.fill();
    const int sym = rd.decode(dc ? T.dc[ci] : T.ac[ci]);
    const int r = dc ? 0 : sym >> 4, sv = dc ? sym : sym & 15;
    const int v = sv ? extend(rd.bits(sv), sv) : 0;
    if (dc) {
        sink.coef(0, v);
        zz = 1;
        return false;
    }
    if (sv)
        sink.coef(zz + r, v);
    else if (r != 15)
        return true;  // EOB
    zz += r + 1;      // r == 15 without a value: sixteen zeros
    return zz >= 64;
}

// Decode from `state` while the position is before `end` (bits), the sink has room
// and fewer than `bound` symbols are done; a state at or past `end` passes through.
// sink.block_done() is called per completed block. Every symbol consumes at least
// one bit, so `bound` = bits to `end` + 1 never cuts a decode short.
template <class Src, class Sink>
PSN_JENT_HD inline uint64_t run(const Src &src, const Tabs &T, uint64_t state, uint64_t end, long long bound,
                                Sink &sink) {
    if (state_pos(state) >= end || sink.full()) return state;
    Reader<Src> rd(src);
    rd.init(state_pos(state));
    int b = state_b(state), zz = state_zz(state);
    for (long long it = 0; it < bound; it++) {
        if (rd.pos() >= end || sink.full()) break;
        if (step(rd, T, b, zz, sink)) {
            zz = 0;
            b = b + 1 == T.bpm ? 0 : b + 1;
            sink.block_done();
        }
    }
    return pack(rd.pos(), b, zz);
}

// Counts blocks, writes nothing (synchronisation passes).
struct CountSink {
    unsigned blocks = 0;
    PSN_JENT_HD void coef(int, int) {}
    PSN_JENT_HD void block_done() { blocks++; }
    PSN_JENT_HD bool full() const { return false; }
};

// Where the scan's blocks go: block g of the scan is block g % bpm of MCU g / bpm,
// at the component's blk0 + (my * v + by) * bw + mx * h + bx, as the serial kernel
// addresses it.
struct Geo {
    int nc, mcux, total, nblocks;   // total = nmcu * bpm blocks in the scan
    struct {
        int h, v, bw, blk0;          // h, v as the scan interleaves them (1, 1 for one component)
    } c[kMaxComp];
};

// Writes coefficients, starting in block `g` of the scan; full at `total` blocks.
struct EmitSink {
    const Geo &G;
    const Tabs &T;
    int16_t *coefs;
    const uint8_t *nat;  // zigzag -> natural order, 64 + 16 entries
    long long g;
    int b, mx, my;
    long long blk;   // coefficient block of the block in progress, -1: none
    PSN_JENT_HD EmitSink(const Geo &geo, const Tabs &t, int16_t *c, const uint8_t *natural, long long g0)
        : G(geo), T(t), coefs(c), nat(natural), g(g0) {
        const long long mcu = g0 / T.bpm;
        b = (int)(g0 % T.bpm);
        mx = (int)(mcu % G.mcux);
        my = (int)(mcu / G.mcux);
        place();
    }
    PSN_JENT_HD void place() {
        blk = -1;
        if (g >= G.total) return;
        const int ci = comp_of_block(T, b), lb = ci ? 0 : b;
        const int by = lb / G.c[ci].h, bx = lb % G.c[ci].h;
        const long long at = G.c[ci].blk0 + (long long)(my * G.c[ci].v + by) * G.c[ci].bw + mx * G.c[ci].h + bx;
        if (at >= 0 && at < G.nblocks) blk = at;
    }
    PSN_JENT_HD void coef(int k, int v) {
        if (blk >= 0 && k < 64 + 16) coefs[blk * 64 + (nat[k] & 63)] = (int16_t)v;
    }
    PSN_JENT_HD void block_done() {
        g++;
        if (++b == T.bpm) {
            b = 0;
            if (++mx == G.mcux) {
                mx = 0;
                my++;
            }
        }
        place();
    }
    PSN_JENT_HD bool full() const { return g >= G.total; }
};

// Element e of component ci's DC sequence in scan order -> its coefficient block.
PSN_JENT_HD inline long long dc_block(const Geo &G, int ci, long long e) {
    const int h = G.c[ci].h, v = G.c[ci].v;
    const long long mcu = e / (h * v);
    const int r = (int)(e % (h * v)), by = r / h, bx = r % h;
    const long long mx = mcu % G.mcux, my = mcu / G.mcux;
    return G.c[ci].blk0 + (my * v + by) * G.c[ci].bw + mx * h + bx;
}

}  // namespace jent
}  // namespace psn
#endif  // PSN_JPEG_ENTROPY_H
