// The planner sweep behind tests/golden/lk_plan_parent.jsonl: the calls, and the
// one-line JSON form of a planned call. A driver passes its run(case) to
// sweep_cases(); lk_plan_dump.cpp is the one for psn::plan_call.
#pragma once

#include <cstdio>
#include <string>
#include <vector>

#include "psn_lk_plan.h"

namespace sweep {

struct Case {
    std::string name;
    psn::PlanCfg cfg;
    std::vector<psn_lk_query> q;
    std::vector<char> filled;  // per slot
    bool allow_scratch = false, counted = false;
    int count_stride = 1;
};

// One launch as a driver saw it.
struct Launch {
    const char *kernel = "";  // st | bx | tiled | lg
    int nq = 0;
    const psn::LkQueryDev *q = nullptr;
    int wgs = 0, grid = 0, lds = 0;
    int nt = 0, ept = 0, ow_e = 0, occ = 0;  // st (nt: also bx, tiled)
    int upt = 0, notail = 0;                 // bx
    int tq = 0;                              // lg
    long long lg_slot = 0;
    int fuse = 0;
};

inline void appendf(std::string &s, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    s += buf;
}

// The first line of a dump: the order of the values in the arrays of the case lines.
inline void print_legend() {
    puts("{\"legend\":{\"frame\":\"w,h,nlevels (user_slots 4, nslots 6, num_cus 256)\","
         "\"knobs\":\"the PlanCfg fields off their defaults\","
         "\"queries\":\"repeat,pt_step,prev_slot,next_slot,first_pt,num_pts,win_w,win_h,max_level,term_type,max_count,epsilon,flags,min_eig\","
         "\"shape\":\"wgs,grid,lds,fuse,nt,ept,ow_e,occ,upt,notail,tq,lg_slot\","
         "\"q\":\"prev_slot,next_slot,wg_begin,pt_begin,num_pts,win_w,win_h,max_level,max_count,flags,tile_rows,min_eig,eps2,"
         "dv_w,dv_dw,dv_pm,dv_jrw,dv_jrw4,dv_g,dv_cw,ow_g,ow_rg,qidx,bx_tre,bx_hw|lg_jr|st_ovl,dv_bxpm,dv_bxjr,sub_pts,sub_pstride\"}}");
}

// {"case": ..., the inputs ...,   (print_case appends the result and closes the object)
inline std::string case_head(const Case &c) {
    std::string s;
    const psn::PlanCfg &g = c.cfg, d;
    appendf(s, "{\"case\":\"%s\",\"frame\":[%d,%d,%d],\"knobs\":{", c.name.c_str(), g.width, g.height, g.nlevels);
    const size_t k0 = s.size();
    auto knob = [&](const char *name, int v, int dflt) {
        if (v != dflt) appendf(s, "%s\"%s\":%d", s.size() > k0 ? "," : "", name, v);
    };
    knob("threads", g.force_threads, d.force_threads);
    knob("generic", g.force_generic, d.force_generic);
    knob("large", g.force_large, d.force_large);
    knob("onewave", g.onewave, d.onewave);
    knob("st_ovl", g.st_ovl, d.st_ovl);
    knob("box", g.box, d.box);
    knob("bx_waves", g.bx_waves, d.bx_waves);
    knob("tiled_lds", g.tiled_lds, d.tiled_lds);
    knob("lg_lds", g.lg_lds, d.lg_lds);
    knob("lg_jr", g.lg_jr, d.lg_jr);
    s += "},\"filled\":\"";
    for (char f : c.filled) s += f ? '1' : '0';
    appendf(s, "\",\"scratch\":%d,\"counted\":%d,\"stride\":%d,\"queries\":[", (int)c.allow_scratch, (int)c.counted, c.count_stride);
    // runs of queries that differ only in first_pt, a constant step apart, print once
    for (size_t i = 0; i < c.q.size();) {
        const psn_lk_query &a = c.q[i];
        const psn_lk_params &p = a.params;
        auto same = [&](const psn_lk_query &b) {
            const psn_lk_params &r = b.params;
            return b.prev_slot == a.prev_slot && b.next_slot == a.next_slot && b.num_pts == a.num_pts &&
                   r.win_w == p.win_w && r.win_h == p.win_h && r.max_level == p.max_level && r.term_type == p.term_type &&
                   r.max_count == p.max_count && r.epsilon == p.epsilon && r.flags == p.flags &&
                   r.min_eig_threshold == p.min_eig_threshold;
        };
        size_t n = 1;
        int step = 0;
        if (i + 1 < c.q.size() && same(c.q[i + 1])) {
            step = c.q[i + 1].first_pt - a.first_pt;
            while (i + n < c.q.size() && same(c.q[i + n]) && c.q[i + n].first_pt == a.first_pt + (int)n * step) n++;
        }
        appendf(s, "%s[%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,\"%a\",%d,\"%a\"]", i ? "," : "", (int)n, n > 1 ? step : 0, a.prev_slot,
                a.next_slot, a.first_pt, a.num_pts, p.win_w, p.win_h, p.max_level, p.term_type, p.max_count, p.epsilon, p.flags,
                p.min_eig_threshold);
        i += n;
    }
    s += "],";
    return s;
}

inline void append_launch(std::string &s, const Launch &l, bool first) {
    appendf(s, "%s{\"kernel\":\"%s\",\"shape\":[%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%lld],\"q\":[", first ? "" : ",", l.kernel, l.wgs,
            l.grid, l.lds, l.fuse, l.nt, l.ept, l.ow_e, l.occ, l.upt, l.notail, l.tq, l.lg_slot);
    for (int i = 0; i < l.nq; i++) {
        const psn::LkQueryDev &d = l.q[i];
        appendf(s, "%s[%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,\"%a\",\"%a\",", i ? "," : "", d.prev_slot, d.next_slot, d.wg_begin,
                d.pt_begin, d.num_pts, d.win_w, d.win_h, d.max_level, d.max_count, d.flags, d.tile_rows, (double)d.min_eig, d.eps2);
        appendf(s, "%u,%u,%u,%u,%u,%u,%u,%d,%d,%d,%d,%d,%u,%u,%d,%d]", d.dv_w, d.dv_dw, d.dv_pm, d.dv_jrw, d.dv_jrw4, d.dv_g,
                d.dv_cw, d.ow_g, d.ow_rg, d.qidx, d.bx_tre, d.bx_hw, d.dv_bxpm, d.dv_bxjr, d.sub_pts, d.sub_pstride);
    }
    s += "]}";
}

// ... "rc": code, "err": text of a failed call, "used": slots, "tag": kernel tag, "launches": [...]}
inline void print_case(const Case &c, int rc, const std::string &err, const std::vector<int> &used, int tag,
                       const std::vector<Launch> &launches) {
    std::string s = case_head(c);
    appendf(s, "\"rc\":%d,\"err\":\"%s\",\"used\":[", rc, rc ? err.c_str() : "");
    for (size_t i = 0; i < used.size(); i++) appendf(s, "%s%d", i ? "," : "", used[i]);
    appendf(s, "],\"tag\":%d,\"launches\":[", tag);
    for (size_t i = 0; i < launches.size(); i++) append_launch(s, launches[i], i == 0);
    s += "]}";
    puts(s.c_str());
}

inline psn_lk_query query(int w, int h, int num_pts, int first_pt = 0, int flags = 0, int max_level = 3, int prev = 0,
                          int next = 1) {
    psn_lk_query q{};
    q.prev_slot = prev;
    q.next_slot = next;
    q.first_pt = first_pt;
    q.num_pts = num_pts;
    q.params.win_w = w;
    q.params.win_h = h;
    q.params.max_level = max_level;
    q.params.term_type = PSN_LK_TERM_COUNT | PSN_LK_TERM_EPS;
    q.params.max_count = 30;
    q.params.epsilon = 0.01;
    q.params.flags = flags;
    q.params.min_eig_threshold = 1e-4;
    return q;
}

inline psn::PlanCfg frame(int w, int h, int nlevels = 4) {
    psn::PlanCfg g;
    g.width = w;
    g.height = h;
    g.nlevels = nlevels;
    g.user_slots = 4;
    g.nslots = 6;
    g.num_cus = 256;
    return g;
}

// Every window class and the sizes at their borders: the 1,024-pixel
// single-tile edge (32x32, 33x31), each box-kernel build, the large-window
// kernel with and without its LDS J region, and 6400x64, the widest window (the
// large-window kernel's LDS plan is refused for no window up to that width: its
// bands and J region stay below 160 KB).
// (the first kCoreWindows, one or two per kernel build, also run on the other frames and on a one-level ring)
constexpr int kCoreWindows = 11;
constexpr int kWindows[][2] = {{9, 9},    {21, 21},  {31, 31},  {33, 31},   {40, 50},   {64, 64},   {72, 64},  {64, 160},
                               {70, 201}, {100, 250}, {140, 357}, {3, 3},    {32, 32},   {16, 72},   {40, 32},  {72, 56},
                               {32, 128}, {64, 176}, {128, 128}, {8, 512},  {6400, 64}};

struct Knob {
    const char *name;
    void (*set)(psn::PlanCfg &);
};
// every variant of psn_lk_debug_set_variant the planner reads, alone
const Knob kKnobs[] = {
    {"THREADS=64", [](psn::PlanCfg &g) { g.force_threads = 64; }},
    {"THREADS=128", [](psn::PlanCfg &g) { g.force_threads = 128; }},
    {"THREADS=256", [](psn::PlanCfg &g) { g.force_threads = 256; }},
    {"THREADS=512", [](psn::PlanCfg &g) { g.force_threads = 512; }},
    {"GENERIC=1", [](psn::PlanCfg &g) { g.force_generic = true; }},
    {"LARGE=1", [](psn::PlanCfg &g) { g.force_large = true; }},
    {"ONEWAVE=0", [](psn::PlanCfg &g) { g.onewave = false; }},
    {"ST_OVL=0", [](psn::PlanCfg &g) { g.st_ovl = false; }},
    {"BOX=0", [](psn::PlanCfg &g) { g.box = false; }},
    {"BX_WAVES=2", [](psn::PlanCfg &g) { g.bx_waves = 2; }},
    {"BX_WAVES=4", [](psn::PlanCfg &g) { g.bx_waves = 4; }},
    {"TILED_LDS=32K", [](psn::PlanCfg &g) { g.tiled_lds = 32 * 1024; }},
    {"LG_LDS=64K", [](psn::PlanCfg &g) { g.lg_lds = 64 * 1024; }},
    {"LG_JR=0", [](psn::PlanCfg &g) { g.lg_jr = false; }},
};

template <class Run> void sweep_cases(Run run) {
    print_legend();
    auto one = [&](const std::string &name, const psn::PlanCfg &g, std::vector<psn_lk_query> q, bool scratch = false,
                   bool counted = false, int stride = 1, std::vector<char> filled = {}) {
        Case c;
        c.name = name;
        c.cfg = g;
        c.q = std::move(q);
        c.filled = filled.empty() ? std::vector<char>((size_t)g.nslots, 1) : filled;
        c.allow_scratch = scratch;
        c.counted = counted;
        c.count_stride = stride;
        run(c);
    };
    auto wname = [](const char *pre, const int *w, int flags, int ml, int n) {
        std::string s;
        appendf(s, "%s %dx%d %s L%d n%d", pre, w[0], w[1], flags ? "scalar" : "sse", ml, n);
        return s;
    };
    const psn::PlanCfg hd = frame(1920, 1080);
    // single queries at 1080p, every window: both accumulation orders, max_level 0 and 3, 1 / 100 / 600 points
    // (600 points: more than 2 * num_cus workgroups, the three-per-CU single-tile build)
    const struct {
        int flags, ml, n;
    } single[] = {{0, 3, 1}, {0, 3, 100}, {0, 3, 600}, {PSN_LK_ACCUM_SCALAR, 3, 600}, {0, 0, 100}, {PSN_LK_ACCUM_SCALAR, 0, 1}};
    for (const auto &w : kWindows)
        for (const auto &v : single) one(wname("1080p", w, v.flags, v.ml, v.n), hd, {query(w[0], w[1], v.n, 0, v.flags, v.ml)});
    // the other frames (at 640x480 and 960x540 the larger windows drop the effective level)
    const struct {
        const char *name;
        int w, h;
    } frames[] = {{"480p", 640, 480}, {"2160p", 3840, 2160}, {"540p", 960, 540}};
    for (const auto &f : frames)
        for (int i = 0; i < kCoreWindows; i++) {
            const int *w = kWindows[i], flags = i % 2 ? PSN_LK_ACCUM_SCALAR : 0;
            one(wname(f.name, w, flags, 3, 600), frame(f.w, f.h), {query(w[0], w[1], 600, 0, flags, 3)});
        }
    // a one-level ring
    for (int i = 0; i < kCoreWindows; i++)
        one(wname("1080p-1level", kWindows[i], 0, 0, 100), frame(1920, 1080, 1), {query(kWindows[i][0], kWindows[i][1], 100, 0, 0, 0)});
    // every variant knob alone
    for (const Knob &k : kKnobs) {
        psn::PlanCfg g = hd;
        k.set(g);
        // 9x9, 31x31, 33x31, 64x64, 64x160, 70x201, 140x357: each kernel class and box build
        for (int i : {0, 2, 3, 5, 7, 8, 10}) one(wname(k.name, kWindows[i], 0, 3, 600), g, {query(kWindows[i][0], kWindows[i][1], 600, 0, 0, 3)});
    }
    // multi-query calls
    {
        std::vector<psn_lk_query> q;
        for (int i = 0; i < 40; i++) q.push_back(query(64, 64, 24, 32 * i));
        one("40 identical 64x64, stride 32: merged", hd, q);
        one("40 identical 64x64, counted stride 1", hd, q, false, true, 1);
        one("40 identical 64x64, counted stride 3", hd, q, false, true, 3);
        for (int i = 20; i < 40; i++) q[i].first_pt += 7;
        one("40 identical 64x64, one gap: two merged queries", hd, q);
        q.clear();
        for (int i = 0; i < 8 * 32; i++) q.push_back(query(64, 160, 24, 24 * i, 0, 3, (i / 32) % 4, (i / 32 + 1) % 4));
        one("8 cameras x 32 of 64x160", hd, q);
        q.clear();
        for (int i = 0; i < 34; i++) q.push_back(query(9 + (i % 8), 9 + i / 8, 10 + i, 64 * i));
        one("34 distinct single-tile windows: split at kMaxQueries", hd, q);
        one("34 distinct single-tile windows, counted stride 3", hd, q, false, true, 3);
        one("70x201 + 140x357: the 16-unit box window joins the large-window launch", hd,
            {query(70, 201, 50, 0), query(140, 357, 50, 50)});
        one("70x201 alone beside small windows", hd, {query(70, 201, 50, 0), query(21, 21, 50, 50), query(64, 64, 50, 100)});
        one("every class in one call", hd,
            {query(21, 21, 100, 0), query(64, 64, 100, 100), query(64, 160, 100, 200, PSN_LK_ACCUM_SCALAR),
             query(100, 250, 100, 300), query(140, 357, 100, 400), query(31, 31, 100, 500, 0, 3, 2, 3)});
        one("zero-point queries between others", hd, {query(64, 64, 0, 0), query(21, 21, 30, 0), query(9999, 9999, 0, 0), query(21, 21, 30, 30)});
        one("only zero-point queries", hd, {query(64, 64, 0, 0), query(21, 21, 0, 0)});
        one("no queries", hd, {});
        one("a zero-point query with a bad window still fails", hd, {query(21, 21, 30, 0), query(2, 21, 0, 0)});
        one("scratch slots of the one-shot call", hd, {query(21, 21, 100, 0, 0, 3, 4, 5)}, true);
        // termination criteria and clamps
        psn_lk_query t = query(21, 21, 10);
        t.params.term_type = PSN_LK_TERM_COUNT;
        t.params.max_count = 500;
        psn_lk_query u = query(21, 21, 10, 10);
        u.params.term_type = PSN_LK_TERM_EPS;
        u.params.epsilon = 50.0;
        psn_lk_query v = query(21, 21, 10, 20, PSN_LK_USE_INITIAL_FLOW | PSN_LK_GET_MIN_EIGENVALS);
        v.params.term_type = 0;
        v.params.max_count = -3;
        v.params.min_eig_threshold = 0.25;
        one("termination criteria clamps", hd, {t, u, v});
    }
    // every error the planner returns
    one("error: slot out of range", hd, {query(21, 21, 10, 0, 0, 3, 0, 4)});
    one("error: negative slot", hd, {query(21, 21, 10, 0, 0, 3, -1, 1)});
    one("error: slot out of range with scratch slots allowed", hd, {query(21, 21, 10, 0, 0, 3, 5, 6)}, true);
    one("error: slot never filled", hd, {query(21, 21, 10, 0, 0, 3, 0, 2)}, false, false, 1, {1, 1, 0, 1, 1, 1});
    one("error: window <= 2", hd, {query(2, 21, 10)});
    one("error: window <= 2 wins over a negative max_level", hd, {query(21, 1, 10, 0, 0, -1)});
    one("error: negative max_level", hd, {query(21, 21, 10, 0, 0, -1)});
    one("error: negative point count", hd, {query(21, 21, -5)});
    one("error: negative first point", hd, {query(21, 21, 5, -1)});
    one("error: window wider than the limit", hd, {query(6401, 8, 10)});
    one("error: window of 2^24 px", hd, {query(4096, 4096, 10)});
    one("error: level cap", frame(1920, 1080, 1), {query(21, 21, 10, 0, 0, 3)});
    one("error: slot fault wins over a window fault", hd, {query(2, 2, 10, 0, 0, 3, 9, 9)});
    one("error: the second query is bad, nothing is planned", hd, {query(21, 21, 10), query(64, 64, 10, 10, 0, -2)});
}

}  // namespace sweep
