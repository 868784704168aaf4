// The host side of the JPEG ingest that touches no device: the marker parser
// (the one place in the library that reads bytes straight from a camera), the
// Huffman table builder and the entropy planner, with the argument structs the
// kernels of psn_jpeg.hip take. Plain C++17, no HIP header: psn_jpeg_parse.cpp
// and psn_jpeg_model.cpp build with a host compiler alone, which is how
// tests/test_jpeg_host.py puts them under the sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "psn_jpeg.h"
#include "psn_jpeg_entropy.h"  // HuffDev, the symbol step of the parallel path
#include "psn_lk.h"

namespace psn {

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

// ---- parallel path: what its kernels take (psn_jpeg.hip) -------------------
struct DevStats {           // written by the kernels, read by psn_jpeg_last_stats / psn_jpeg_batch_stats
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

// Bytes of a workgroup's subsequences are staged in LDS up to this subsequence
// size (256 subsequences + tables + states stay under 64 KiB); larger ones are
// read from global memory.
#ifndef PSN_JPEG_STAGE_MAX_SUB
#define PSN_JPEG_STAGE_MAX_SUB 128
#endif

// A parsed frame: tables, geometry, entropy segments.
struct Parsed {
    Tables tab;
    JpegArgs a{};
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

// Calls between the units of the library, not part of its interface.
#pragma GCC visibility push(hidden)

// The headers and the entropy segments of the `n` bytes at `d`; reads nothing
// outside them. PSN_LK_OK, or PSN_LK_ERR_ARG / PSN_LK_ERR_UNSUPPORTED with the
// reason in `why`.
int parse(const uint8_t *d, size_t n, Parsed &P, std::string &why);

// jdhuff.c jpeg_make_d_derived_tbl: false for a table libjpeg rejects with
// JERR_BAD_HUFF_TABLE -- more codes of a length than fit after the shorter ones
// (the canonical code would overflow its length; the all-ones code is not
// allowed), or a DC symbol above 15. Checked before any table entry is written.
bool build_huff(const uint8_t *bits, const uint8_t *vals, int nvals, bool dc, HuffDev &h);

// psn_jpeg_debug_set_entropy's and psn_jpeg_entropy_model's mode and sub_bytes.
bool valid_entropy_request(int mode, int sub);

// The planner: the parallel path is legal for a plain stream without restart
// intervals, and it is the planner's choice wherever it is legal.
void plan_entropy(const Parsed &P, int mode, int sub, psn_jpeg_plan &pl);

// The scan's block layout as the symbol step's sinks address it.
void entropy_geometry(const Parsed &P, jent::Geo &G, int &nb0, int &bpm);

// A batch (psn_jpeg_decode_batch_device; psn_jpeg_decode_device's image is a batch
// of one): the parsed items, their plans and where each item's tables, bytes,
// scratch, coefficients and planes lie.
struct Batch {
    std::vector<Parsed> P;
    std::vector<psn_jpeg_plan> plans;
    psn_jpeg_batch_layout L;
};

// Checks and parses every item, plans it (mode, sub: psn_jpeg_debug_set_entropy)
// and lays the batch out. On an error B.L.bad_item is the first bad item (-1: the
// call's own arguments) and `why` the bare reason: the caller that has items to
// speak of names the item.
int plan_batch(const psn_jpeg_item *items, int n, int mode, int sub, Batch &B, std::string &why);

// The kernels' arguments of item i of a planned batch, over the base addresses of
// the device blob, the parallel scratch, the coefficients and the planes.
void batch_args(const Batch &B, int i, const psn_jpeg_item &it, uint8_t *blob, uint8_t *par, uint8_t *coef,
                uint8_t *planes, JpegArgs &a, EntArgs &e);

#pragma GCC visibility pop

}  // namespace psn
