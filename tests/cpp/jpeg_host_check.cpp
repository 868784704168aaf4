// TEST HARNESS: a stand-alone caller of the JPEG host side
// (mcmtt_opticalflow_amd/csrc/psn_jpeg_parse.cpp and psn_jpeg_model.cpp: the
// marker parser, the planner and the CPU model of the entropy decode), compiled
// together with them under -fsanitize=address,undefined by
// tests/test_jpeg_host.py. It reads a case file of streams and hands each to the
// host entries of include/psn_jpeg.h from a malloc block of exactly the stream's
// length, so the first byte past the stream is poisoned; the coefficient buffer
// is as exact. What every call returns is printed for the test to compare with
// the shared library's answers.
//
// Case file, little endian, repeated to the end:  u32 length, u32 flags, bytes
//   flags bit 0: psn_jpeg_info and psn_jpeg_entropy_plan only
// Output, one line per call group:
//   stream I len N info RC W H COMPS plan RC <the 7 fields of psn_jpeg_plan>
//   model I MODE SUB rc RC [stats <the 8 fields of psn_jpeg_stats> fnv <FNV-1a 64 of the coefficients>]
#include <cinttypes>
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

static void model(size_t idx, const uint8_t *d, size_t n, int mode, int sub) {
    psn_jpeg_stats st;
    std::memset(&st, 0, sizeof st);
    int rc = psn_jpeg_entropy_model(d, n, mode, sub, nullptr, &st);  // blocks: the size of coef
    if (rc) {
        std::printf("model %zu %d %d rc %d\n", idx, mode, sub, rc);
        return;
    }
    const size_t count = (size_t)st.blocks * 64;
    int16_t *coef = (int16_t *)std::malloc(count * sizeof(int16_t));
    if (!coef) std::exit(fail("out of memory"));
    rc = psn_jpeg_entropy_model(d, n, mode, sub, coef, &st);
    uint64_t h = 0xcbf29ce484222325ull;
    const uint8_t *b = (const uint8_t *)coef;
    for (size_t i = 0; rc == 0 && i < count * sizeof(int16_t); i++) h = (h ^ b[i]) * 0x100000001b3ull;
    std::printf("model %zu %d %d rc %d stats %d %d %d %d %d %d %d %d fnv %016" PRIx64 "\n", idx, mode, sub, rc, st.path,
                st.segments, st.sub_bytes, st.subsequences, st.sequences, st.sync_rounds, st.chain_rounds, st.blocks, h);
    std::free(coef);
}

int main(int argc, char **argv) {
    if (argc != 2) return fail("usage: jpeg_host_check CASEFILE");
    std::setvbuf(stdout, nullptr, _IOLBF, 0);  // a sanitizer report ends the process without flushing
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return fail("cannot open the case file");
    std::vector<uint8_t> all;
    uint8_t buf[1 << 16];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + got);
    std::fclose(f);
    size_t idx = 0;
    for (size_t at = 0; at < all.size(); idx++) {
        if (all.size() - at < 8) return fail("case file ends inside a stream's prefix");
        const size_t n = u32(&all[at]);
        const uint32_t flags = u32(&all[at + 4]);
        at += 8;
        if (all.size() - at < n) return fail("case file ends inside a stream");
        uint8_t *d = (uint8_t *)std::malloc(n);  // malloc(0) is a valid, unreadable pointer
        if (!d) return fail("out of memory");
        if (n) std::memcpy(d, &all[at], n);
        at += n;
        int w = 0, h = 0, comps = 0;
        const int info = psn_jpeg_info(d, n, &w, &h, &comps);
        psn_jpeg_plan pl;
        std::memset(&pl, 0, sizeof pl);
        const int plan = psn_jpeg_entropy_plan(d, n, &pl);
        std::printf("stream %zu len %zu info %d %d %d %d plan %d %d %d %d %d %d %d %d\n", idx, n, info, w, h, comps, plan,
                    pl.path, pl.segments, pl.plain, pl.entropy_bytes, pl.sub_bytes, pl.subsequences, pl.sequences);
        if (!(flags & 1)) {
            model(idx, d, n, 1, 0);
            for (int sub : {4, 64, 1024}) model(idx, d, n, 2, sub);
        }
        std::free(d);
    }
    std::printf("jpeg host check: ok %zu\n", idx);
    return 0;
}
