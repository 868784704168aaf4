// The CPU model of the parallel entropy decode (psn_jpeg_entropy_model of
// include/psn_jpeg.h): the symbol step the kernels run (psn_jpeg_entropy.h) with
// the kernels' rounds emulated one after the other. No device, no HIP header.
#include <algorithm>
#include <cstring>
#include <vector>

#include "psn_jpeg_parse.h"

namespace {

using psn::Parsed;
namespace jent = psn::jent;

// psn_jpeg_entropy_model's decode: the kernels' passes, one after the other.
void model_decode(const Parsed &P, const uint8_t *ent, const psn_jpeg_plan &pl, int16_t *coef, psn_jpeg_stats &S) {
    jent::Geo G;
    int nb0, bpm;
    psn::entropy_geometry(P, G, nb0, bpm);
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

extern "C" int psn_jpeg_entropy_model(const uint8_t *data, size_t len, int mode, int sub_bytes, int16_t *coef,
                                      psn_jpeg_stats *stats) {
    if (!data || !stats || !psn::valid_entropy_request(mode, sub_bytes)) return PSN_LK_ERR_ARG;
    Parsed P;
    std::string why;
    const int rc = psn::parse(data, len, P, why);
    if (rc) return rc;
    if (P.a.ri != 0 || !P.plain) return PSN_LK_ERR_UNSUPPORTED;
    psn_jpeg_plan pl;
    psn::plan_entropy(P, mode, sub_bytes, pl);
    *stats = psn_jpeg_stats{pl.path, pl.segments, pl.sub_bytes, pl.subsequences, pl.sequences, 0, 0, P.a.nblocks};
    if (!coef) return PSN_LK_OK;
    stats->blocks = 0;
    model_decode(P, data + P.ent0, pl, coef, *stats);
    return PSN_LK_OK;
}
