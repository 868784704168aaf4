// The JPEG marker parser, the Huffman table builder and the entropy planner
// (psn_jpeg_parse.h), and the two entries of include/psn_jpeg.h that are pure
// parsing: psn_jpeg_info and psn_jpeg_entropy_plan. No device, no HIP header.
#include "psn_jpeg_parse.h"

#include <algorithm>
#include <climits>
#include <cstring>

namespace psn {

static int rd16(const uint8_t *p) { return (p[0] << 8) | p[1]; }

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

int parse(const uint8_t *d, size_t n, Parsed &P, std::string &why) {
    memset(&P.tab, 0, sizeof P.tab);
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return why = "not a JPEG (no SOI)", PSN_LK_ERR_ARG;
    int ids[kJpegMaxComp] = {0, 0, 0};
    bool sof = false;
    size_t p = 2;
    while (p + 4 <= n) {
        if (d[p] != 0xFF) return why = "marker expected", PSN_LK_ERR_ARG;
        const int m = d[p + 1];
        if (m == 0xFF) {
            p++;
            continue;
        }
        const int len = rd16(d + p + 2);
        if (len < 2 || p + 2 + (size_t)len > n) return why = "truncated segment", PSN_LK_ERR_ARG;
        const uint8_t *s = d + p + 4;
        const int sl = len - 2;
        if (m == 0xDB) {
            for (int o = 0; o < sl;) {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                if (tq > 3 || o + 1 + (pq ? 128 : 64) > sl) return why = "bad DQT", PSN_LK_ERR_ARG;
                for (int i = 0; i < 64; i++)
                    P.tab.qt[tq][jent::kNaturalHost[i]] = (uint16_t)(pq ? rd16(s + o + 1 + 2 * i) : s[o + 1 + i]);
                o += 1 + (pq ? 128 : 64);
            }
        } else if (m == 0xC4) {
            for (int o = 0; o < sl;) {
                const int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3 || o + 17 > sl) return why = "bad DHT", PSN_LK_ERR_ARG;
                int cnt = 0;
                for (int l = 0; l < 16; l++) cnt += s[o + 1 + l];
                if (cnt > 256 || o + 17 + cnt > sl) return why = "bad DHT", PSN_LK_ERR_ARG;
                P.hstate[tc][th] = build_huff(s + o + 1, s + o + 17, cnt, tc == 0, tc ? P.tab.ac[th] : P.tab.dc[th]) ? 1 : -1;
                o += 17 + cnt;
            }
        } else if (m == 0xC0 || m == 0xC1) {
            if (sl < 6 || s[0] != 8) return why = "not 8-bit", PSN_LK_ERR_UNSUPPORTED;
            P.a.H = rd16(s + 1);
            P.a.W = rd16(s + 3);
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
            P.a.ri = sl >= 2 ? rd16(s) : 0;
        } else if (m == 0xDA) {
            if (!sof || sl < 1 || s[0] != P.a.nc) return why = "unsupported scan", PSN_LK_ERR_UNSUPPORTED;
            if (sl < 1 + 2 * P.a.nc) return why = "bad SOS", PSN_LK_ERR_ARG;  // the selectors lie inside the segment
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
    JpegArgs &a = P.a;
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
    // CompGeo::plane0 and the kernels' block offsets are int: every plane byte (64 a block) has to fit one
    long long blocks = 0;
    for (int c = 0; c < a.nc; c++)
        blocks += a.nc == 1 ? (long long)((a.W + 7) / 8) * ((a.H + 7) / 8) : (long long)mcux * mcuy * a.c[c].h * a.c[c].v;
    if (blocks * 64 > INT_MAX) return why = "frame too large", PSN_LK_ERR_UNSUPPORTED;
    int blk = 0, plane = 0;
    for (int c = 0; c < a.nc; c++) {
        CompGeo &g = a.c[c];
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

bool valid_entropy_request(int mode, int sub) {
    return mode >= 0 && mode <= 2 && (sub == 0 || (sub >= jent::kMinSub && sub <= jent::kMaxSub && sub % 4 == 0));
}

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

void entropy_geometry(const Parsed &P, jent::Geo &G, int &nb0, int &bpm) {
    const JpegArgs &a = P.a;
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

static size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

int plan_batch(const psn_jpeg_item *items, int n, int mode, int sub, Batch &B, std::string &why) {
    psn_jpeg_batch_layout &L = B.L;
    memset(&L, 0, sizeof L);
    L.bad_item = -1;
    if (!items) return why = "null item list", PSN_LK_ERR_ARG;
    if (n < 1 || n > PSN_JPEG_MAX_BATCH)
        return why = "batch of " + std::to_string(n) + " items (1.." + std::to_string(PSN_JPEG_MAX_BATCH) + ")", PSN_LK_ERR_ARG;
    B.P.assign((size_t)n, Parsed());
    B.plans.assign((size_t)n, psn_jpeg_plan());
    for (int i = 0; i < n; i++) {  // every item is checked before anything is laid out
        L.bad_item = i;
        if (!items[i].data || !items[i].d_bgr) return why = "null pointer", PSN_LK_ERR_ARG;
        const int rc = parse(items[i].data, items[i].len, B.P[(size_t)i], why);
        if (rc) return rc;
        if (items[i].stride < 3 * B.P[(size_t)i].a.W)
            return why = "stride " + std::to_string(items[i].stride) + " < 3 * width " + std::to_string(B.P[(size_t)i].a.W),
                   PSN_LK_ERR_ARG;
        plan_entropy(B.P[(size_t)i], mode, sub, B.plans[(size_t)i]);
    }
    L.n = n;
    size_t blob = 0, par = 0, coef = 0, planes = 0;
    for (int i = 0; i < n; i++) {
        const Parsed &P = B.P[(size_t)i];
        const psn_jpeg_plan &pl = B.plans[(size_t)i];
        psn_jpeg_batch_item_layout &it = L.item[i];
        it.path = pl.path;
        it.tables = blob;
        blob += up16(sizeof(Tables));
        it.segments = blob;
        it.segments_size = up16(4 * P.seg.size());
        blob += it.segments_size;
        it.bytes = blob;
        it.bytes_size = up16((size_t)P.a.data_len) + 16;  // the item's own zeroed slack
        blob += it.bytes_size;
        it.stats = par;
        par += up16(sizeof(DevStats));
        if (pl.path == PSN_JPEG_PATH_PARALLEL) {
            const size_t nsub = (size_t)pl.subsequences, nseq = (size_t)pl.sequences;
            it.list_index = L.n_parallel;
            L.parallel[L.n_parallel++] = i;
            it.states_size = up16(8 * nsub);
            it.counts_size = it.prefix_size = up16(4 * nsub);
            it.rounds_size = up16(4 * nseq);
            L.max_sequences = std::max(L.max_sequences, pl.sequences);
            L.max_parallel_components = std::max(L.max_parallel_components, P.a.nc);
        } else {
            it.list_index = L.n_serial;
            L.serial[L.n_serial++] = i;
            L.max_segment_groups = std::max(L.max_segment_groups, (P.a.nseg + 63) / 64);
        }
        it.states = par;
        par += it.states_size;
        it.counts = par;
        par += it.counts_size;
        it.prefix = par;
        par += it.prefix_size;
        it.rounds = par;
        par += it.rounds_size;
        it.coef = coef;
        it.coef_size = (size_t)P.a.nblocks * 64 * sizeof(int16_t);  // a multiple of 128
        coef += it.coef_size;
        it.planes = planes;
        it.planes_size = (size_t)P.a.nblocks * 64;
        planes += it.planes_size;
        L.max_block_groups = std::max(L.max_block_groups, (P.a.nblocks + 255) / 256);
        L.max_width = std::max(L.max_width, P.a.W);
        L.max_height = std::max(L.max_height, P.a.H);
    }
    L.ent_args = blob;
    blob += up16((size_t)n * sizeof(EntArgs));
    L.jpeg_args = blob;
    blob += up16((size_t)n * sizeof(JpegArgs));
    L.lists = blob;
    blob += up16(2 * (size_t)n * sizeof(int));  // [parallel | serial]
    L.blob_size = blob;
    L.scratch_size = par;
    L.coef_size = coef;
    L.planes_size = planes;
    // one memset and one copy take the totals; the tools that read the buffers index them with int
    if (coef > (size_t)INT_MAX || blob > (size_t)INT_MAX) {
        L.bad_item = -1;
        return why = "frame too large (batch of " + std::to_string(n) + ")", PSN_LK_ERR_UNSUPPORTED;
    }
    L.bad_item = -1;
    return PSN_LK_OK;
}

void batch_args(const Batch &B, int i, const psn_jpeg_item &item, uint8_t *blob, uint8_t *par, uint8_t *coef,
                uint8_t *planes, JpegArgs &a, EntArgs &e) {
    const Parsed &P = B.P[(size_t)i];
    const psn_jpeg_plan &pl = B.plans[(size_t)i];
    const psn_jpeg_batch_item_layout &it = B.L.item[i];
    a = P.a;
    a.tab = (const Tables *)(blob + it.tables);
    a.seg = (const int *)(blob + it.segments);
    a.data = blob + it.bytes;
    a.coef = (int16_t *)(coef + it.coef);
    a.planes = planes + it.planes;
    a.out = item.d_bgr;
    a.out_stride = item.stride;
    memset(&e, 0, sizeof e);
    if (pl.path != PSN_JPEG_PATH_PARALLEL) return;
    e.tab = a.tab;
    e.data = a.data;
    e.len = a.data_len;
    e.S = pl.sub_bytes;
    e.nsub = pl.subsequences;
    e.nseq = pl.sequences;
    e.stage = pl.sub_bytes <= PSN_JPEG_STAGE_MAX_SUB ? 1 : 0;
    entropy_geometry(P, e.geo, e.nb0, e.bpm);
    e.nmcu = a.nmcu;
    for (int c = 0; c < a.nc; c++) {
        e.td[c] = a.c[c].td;
        e.ta[c] = a.c[c].ta;
    }
    e.stats = (DevStats *)(par + it.stats);
    e.st = (unsigned long long *)(par + it.states);
    e.cnt = (unsigned *)(par + it.counts);
    e.pre = (unsigned *)(par + it.prefix);
    e.seq_rounds = (int *)(par + it.rounds);
    e.coef = a.coef;
}

}  // namespace psn

extern "C" {

int psn_jpeg_batch_plan(const psn_jpeg_item *items, int n, psn_jpeg_batch_layout *out, psn_jpeg_plan *plans) {
    if (!out) return PSN_LK_ERR_ARG;
    psn::Batch B;
    std::string why;
    const int rc = psn::plan_batch(items, n, 0, 0, B, why);
    *out = B.L;
    if (rc) return rc;
    if (plans)
        for (int i = 0; i < n; i++) plans[i] = B.plans[(size_t)i];
    return PSN_LK_OK;
}

int psn_jpeg_info(const uint8_t *data, size_t len, int *w, int *h, int *comps) {
    if (!data || !w || !h) return PSN_LK_ERR_ARG;
    psn::Parsed P;
    std::string why;
    const int rc = psn::parse(data, len, P, why);
    if (rc) return rc;
    *w = P.a.W;
    *h = P.a.H;
    if (comps) *comps = P.a.nc;
    return PSN_LK_OK;
}

int psn_jpeg_entropy_plan(const uint8_t *data, size_t len, psn_jpeg_plan *out) {
    if (!data || !out) return PSN_LK_ERR_ARG;
    psn::Parsed P;
    std::string why;
    const int rc = psn::parse(data, len, P, why);
    if (rc) return rc;
    psn::plan_entropy(P, 0, 0, *out);
    return PSN_LK_OK;
}

}  // extern "C"
