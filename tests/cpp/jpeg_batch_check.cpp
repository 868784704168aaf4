// TEST HARNESS: a stand-alone caller of the batch planner (psn_jpeg_batch_plan,
// mcmtt_opticalflow_amd/csrc/psn_jpeg_parse.cpp), compiled together with that unit
// under -fsanitize=address,undefined by tests/test_jpeg_batch_host.py. It reads a
// case file of batches and hands each to psn_jpeg_batch_plan with every stream in
// a malloc block of exactly its length, the item array and the plan array as exact,
// so a read past a stream or past the n-th item ends the run. What the call
// returns is printed for the test to compare with the shared library's answers.
//
// Case file, little endian, repeated to the end:
//   u32 items, i32 n handed to the library, then per item: u32 length, u32 flags, i32 stride, bytes
//   flags bit 0: null data pointer; bit 1: null d_bgr
// Output: one "batch" line (return code, bad item, totals, lists, maxima), then on
// success one "item" line per item (layout fields and the 7 fields of its plan).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "psn_jpeg.h"

static uint32_t u32(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

static int fail(const char *what) {
    std::printf("FAILED: %s\n", what);
    return 2;
}

int main(int argc, char **argv) {
    if (argc != 2) return fail("usage: jpeg_batch_check CASEFILE");
    std::setvbuf(stdout, nullptr, _IOLBF, 0);  // a sanitizer report ends the process without flushing
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return fail("cannot open the case file");
    std::vector<uint8_t> all;
    uint8_t buf[1 << 16];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + got);
    std::fclose(f);
    static uint8_t out_mark[16];  // d_bgr is only checked for null
    size_t idx = 0;
    for (size_t at = 0; at < all.size(); idx++) {
        if (all.size() - at < 8) return fail("case file ends inside a batch header");
        const size_t items = u32(&all[at]);
        const int n = (int)u32(&all[at + 4]);
        at += 8;
        psn_jpeg_item *it = (psn_jpeg_item *)std::malloc(items * sizeof(psn_jpeg_item));
        psn_jpeg_plan *plans = (psn_jpeg_plan *)std::malloc(items * sizeof(psn_jpeg_plan));
        std::vector<uint8_t *> blocks;
        for (size_t i = 0; i < items; i++) {
            if (all.size() - at < 12) return fail("case file ends inside an item header");
            const size_t len = u32(&all[at]);
            const uint32_t flags = u32(&all[at + 4]);
            const int stride = (int)u32(&all[at + 8]);
            at += 12;
            if (all.size() - at < len) return fail("case file ends inside a stream");
            uint8_t *d = (uint8_t *)std::malloc(len);  // malloc(0) is a valid, unreadable pointer
            if (!d) return fail("out of memory");
            if (len) std::memcpy(d, &all[at], len);
            at += len;
            blocks.push_back(d);
            it[i] = psn_jpeg_item{(flags & 1) ? nullptr : d, len, (flags & 2) ? nullptr : out_mark, stride};
        }
        psn_jpeg_batch_layout *L = (psn_jpeg_batch_layout *)std::malloc(sizeof(psn_jpeg_batch_layout));
        if (!L) return fail("out of memory");
        const int rc = psn_jpeg_batch_plan(it, n, L, plans);
        std::printf("batch %zu rc %d bad %d n %d lists %d %d totals %zu %zu %zu %zu %zu %zu %zu maxima %d %d %d %d %d %d par", idx,
                    rc, L->bad_item, L->n, L->n_parallel, L->n_serial, L->ent_args, L->jpeg_args, L->lists, L->blob_size,
                    L->scratch_size, L->coef_size, L->planes_size, L->max_sequences, L->max_parallel_components,
                    L->max_segment_groups, L->max_block_groups, L->max_width, L->max_height);
        for (int k = 0; k < L->n_parallel; k++) std::printf(" %d", L->parallel[k]);
        std::printf(" ser");
        for (int k = 0; k < L->n_serial; k++) std::printf(" %d", L->serial[k]);
        std::printf("\n");
        for (int i = 0; rc == 0 && i < L->n; i++) {
            const psn_jpeg_batch_item_layout &b = L->item[i];
            const psn_jpeg_plan &p = plans[i];
            std::printf("item %zu %d path %d %d blob %zu %zu %zu %zu %zu scratch %zu %zu %zu %zu %zu %zu %zu %zu %zu out %zu %zu %zu %zu "
                        "plan %d %d %d %d %d %d %d\n",
                        idx, i, b.path, b.list_index, b.tables, b.segments, b.bytes, b.segments_size, b.bytes_size, b.stats,
                        b.states, b.counts, b.prefix, b.rounds, b.states_size, b.counts_size, b.prefix_size, b.rounds_size,
                        b.coef, b.coef_size, b.planes, b.planes_size, p.path, p.segments, p.plain, p.entropy_bytes,
                        p.sub_bytes, p.subsequences, p.sequences);
        }
        std::free(L);
        for (uint8_t *d : blocks) std::free(d);
        std::free(plans);
        std::free(it);
    }
    std::printf("jpeg batch check: ok %zu\n", idx);
    return 0;
}
