// The launch planner of a track call (psn_lk_plan.h): which kernel takes which
// query, and every launch's shape. The executor is track_device_impl
// (psn_lk_track.cpp).
#include "psn_lk_plan.h"

#include <algorithm>
#include <utility>

extern "C" {

int psn_lk_window_supported(int w, int h) {
    return w > 0 && h > 0 && w <= PSN_LK_MAX_WIN_WIDTH && (long long)h * ((w + 3) / 4) < (long long)PSN_LK_MAX_WIN_QUADS;
}

int psn_lk_effective_max_level(int width, int height, int win_w, int win_h, int max_level) {
    if (width <= 0 || height <= 0 || max_level < 0) return PSN_LK_ERR_ARG;
    int sw = width, sh = height;
    for (int level = 0; level <= max_level; level++) {
        sw = (sw + 1) / 2;
        sh = (sh + 1) / 2;
        if (sw <= win_w || sh <= win_h) return level;
    }
    return max_level;
}

}  // extern "C"

namespace psn {
namespace {

// The planner's default for the windows the two-wave box build fits
// (PSN_LK_VARIANT_BX_WAVES 0); DESIGN.md section 8 has the measurement behind it.
constexpr bool kBxPlanTwoWave = true;
// A launch group's frame class, packed above its key (box: <= 162, large: <= 192 quads)
constexpr int kFclsShift = 16;
// The launches the forward entry fits take it by default (PSN_LK_VARIANT_FW 0): the
// entry's gains are measured against lk_kernel_bx<10, true> in DESIGN.md section 8.
// The runtime variant fw=1 plans as if it did not exist.

// One query as planned: its device descriptor and the kernels that can take it.
struct PlannedQuery {
    int src = 0;  // index in the caller's query array
    LkQueryDev d{};
    bool single = false;        // single-tile kernel (window <= 1024 px, LDS plan fits)
    int st_lds = 0;             // its LDS
    int ow_rows = 1 << 30, ow_lds = 0;  // its one-wave mode
    int ovl_lds = 0;                    // the one-wave mode with the overlapped A phase (0: does not fit)
    int bx_upt = 0, bx_lds = 0;  // box kernel units per thread (0: does not fit)
    bool bx_w2 = false;          // + the two-wave build (bx_upt = kBxUPT2)
    int tiled_tr = 0;           // row-tiled kernel: tile rows (0: window not LDS-resident)
    int lg_tr = 0;              // large-window kernel: band rows
    bool lg_jr = false;         // + J region in LDS
    int lg_tq = 192;            // + quads per ordered-chain tile
    int cls = kClsLg, key = 0;  // the launch it goes to
    int fcls = 0;               // the frame class of its two slots
};

// Row tiles of the row-tiled kernel (window LDS-resident): within the occupancy
// budget when the window allows, else the LDS limit; 0 if it does not fit.
int tiled_rows(const PlanCfg &c, int w, int h) {
    if ((long)w * h > 16384) return 0;  // Iw + Dw in LDS: 6 B per window pixel
    int tr = h;
    const int budget = 160 * 1024 - 1024;
    while (tr > 1 && lk_lds_bytes(w, h, tr) > c.tiled_lds) tr--;
    while (tr > 1 && lk_lds_bytes(w, h, tr) > budget) tr--;
    return lk_lds_bytes(w, h, tr) <= budget ? tr : 0;
}
// Band rows of the large-window kernel's A phase within its LDS budget (>= 1 row;
// the tile planes of the fallbacks set the floor of the budget).
int lg_rows(const PlanCfg &c, int w, int h, bool jr, int tq) {
    int tr = 1;
    const int budget = std::max(c.lg_lds, lg_lds_bytes(w, h, 1, jr, tq));
    while (tr < h && lg_lds_bytes(w, h, tr + 1, jr, tq) <= budget) tr++;
    return tr;
}
// The large-window kernel's plan: the J region of the iterations in LDS with the
// largest ordered-chain tile (kLgTQs) that keeps the workgroup within
// kLgJrMaxLds (J staging needs the region's dword rows exactly divisible by the
// staging's magic: q * (d - 1) < 2^22 and q * magic < 2^32 for every dword q),
// else J from the level with kLgTQNoJr-quad tiles (measured with
// tools/gpu_lg_ab.sh, 512 points: 100x250 981 -> 858 us with 192-quad tiles;
// without the LDS J region 192-quad tiles were slower than 128 at 140x357).
void lg_plan(const PlanCfg &c, int w, int h, bool &jr, int &tq) {
    jr = false;
    tq = kLgTQNoJr;
    if (!c.lg_jr) return;
    const long long d = bx_jrp(w) / 4, n = (long long)st_jreg_h(h) * d;
    if (!(n * (d - 1) < (1LL << 22) && n * (long long)div_magic((int)d) < (1LL << 32))) return;
    for (int t : kLgTQs)
        if (lg_lds_bytes(w, h, 1, true, t) <= kLgJrMaxLds) {
            jr = true;
            tq = t;
            return;
        }
}

// Validate and plan one query.
// no_bx16: a window of 13-16 units per thread goes to the large-window kernel
// (the call has large windows anyway: one launch fewer, see plan_call)
int plan_query(const PlanCfg &c, const char *filled, const psn_lk_query &q, bool allow_scratch, PlannedQuery &pq,
               std::string &err, bool no_bx16 = false) {
    const psn_lk_params &p = q.params;
    const int limit = allow_scratch ? c.nslots : c.user_slots;
    if (q.prev_slot < 0 || q.prev_slot >= limit || q.next_slot < 0 || q.next_slot >= limit)
        return set_err(err, PSN_LK_ERR_SLOT, "slot out of range (%d, %d)", q.prev_slot, q.next_slot);
    if (!filled[q.prev_slot] || !filled[q.next_slot])
        return set_err(err, PSN_LK_ERR_SLOT, "slot never filled (%d, %d)", q.prev_slot, q.next_slot);
    if (p.win_w <= 2 || p.win_h <= 2) return set_err(err, PSN_LK_ERR_WINSIZE, "winSize %dx%d <= 2", p.win_w, p.win_h);
    if (p.max_level < 0 || q.num_pts < 0 || q.first_pt < 0) return set_err(err, PSN_LK_ERR_ARG, "bad query");
    if (!psn_lk_window_supported(p.win_w, p.win_h))
        return set_err(err, PSN_LK_ERR_UNSUPPORTED, "window %dx%d wider than %d px or above 2^24 px", p.win_w, p.win_h,
                       PSN_LK_MAX_WIN_WIDTH);
    // both pyramids of a query have one geometry: the launch's (its class's RingGeo)
    pq.fcls = c.slot_class(q.prev_slot);
    if (c.slot_class(q.next_slot) != pq.fcls)
        return set_err(err, PSN_LK_ERR_ARG, "slots %d and %d hold frames of different classes (%d, %d)", q.prev_slot,
                       q.next_slot, pq.fcls, c.slot_class(q.next_slot));
    const int ml = psn_lk_effective_max_level(c.class_width(pq.fcls), c.class_height(pq.fcls), p.win_w, p.win_h, p.max_level);
    if (ml >= c.nlevels)
        return set_err(err, PSN_LK_ERR_LEVEL_CAP, "query needs %d levels, ring holds %d", ml + 1, c.nlevels);
    int max_count = (p.term_type & PSN_LK_TERM_COUNT) ? std::min(std::max(p.max_count, 0), 100) : 30;
    double eps = (p.term_type & PSN_LK_TERM_EPS) ? std::min(std::max(p.epsilon, 0.), 10.) : 0.01;
    const int w = p.win_w, h = p.win_h;
    const bool sse = (p.flags & PSN_LK_ACCUM_SCALAR) == 0;
    LkQueryDev &d = pq.d;
    d = LkQueryDev{};
    if ((long)w * h <= 256 * kStEPTMax) {
        const LkStLayout st(w, h, sse, ml + 1);
        if (st.total <= kStMaxLds) {
            pq.single = true;
            pq.st_lds = st.total;
            const LkStLayout so(w, h, sse, ml + 1, true);
            if (ow_rows(w, h) <= kOwMaxRows && so.total <= kStMaxLds) {
                pq.ow_rows = ow_rows(w, h);
                pq.ow_lds = so.total;
                const LkStLayout sv(w, h, sse, ml + 1, true, true);
                if (sv.total <= kStMaxLds) pq.ovl_lds = sv.total;
            }
        }
    }
    pq.tiled_tr = tiled_rows(c, w, h);
    lg_plan(c, w, h, pq.lg_jr, pq.lg_tq);
    pq.lg_tr = lg_rows(c, w, h, pq.lg_jr, pq.lg_tq);
    d.prev_slot = q.prev_slot;
    d.next_slot = q.next_slot;
    d.pt_begin = q.first_pt;
    d.num_pts = q.num_pts;
    d.win_w = w;
    d.win_h = h;
    d.max_level = ml;
    d.max_count = max_count;
    d.flags = c.err_status_ignore ? p.flags & ~PSN_LK_ERR_STATUS_ONLY : p.flags;
    d.tile_rows = pq.single ? h : pq.tiled_tr;
    d.min_eig = (float)p.min_eig_threshold;
    d.eps2 = eps * eps;
    const int jrw = st_jreg_w(w);
    const int nc = sse ? (w / 8) * 2 : 0;  // columns per SSE2 chain class
    d.ow_g = std::max(ow_groups(w), 1);
    d.ow_rg = (h + d.ow_g - 1) / d.ow_g;
    d.dv_w = div_magic(w);
    d.dv_dw = div_magic(w + 1);
    d.dv_pm = div_magic(lk_pat_m(w));
    d.dv_jrw = div_magic(jrw);
    d.dv_jrw4 = div_magic(jrw / 4);
    d.dv_g = div_magic(d.ow_g);
    d.dv_cw = div_magic(nc);
    {  // box-window kernel: units of 4 pixels, <= kBxMaxUPT per thread
        const long need = ((long)h * bx_qw(w) + kBxNT - 1) / kBxNT;
        const int upt = need <= 4 ? 4 : need <= 8 ? 8 : need <= 10 ? 10 : need <= 12 ? 12 : 16;
        const bool notail = sse && w % 8 == 0;
        // (a unit's J offset in the region, y * bx_jrp(w) + 4 q, is a 16-bit half)
        if (need <= kBxMaxUPT && BxLayout(w, h, upt).total <= bx_max_lds(upt, notail) &&
            (long)st_jreg_h(h) * bx_jrp(w) < 65536) {
            pq.bx_upt = upt;
            pq.bx_lds = BxLayout(w, h, upt).total;
            d.bx_tre = bx_err_rows(w, h, BxLayout(w, h, 4).pb);
            // the two-wave build: the planner's choice for the windows it fits
            // (kBxPlanTwoWave), or what the BX_WAVES variant says
            const bool want2 = c.bx_waves == 2 || (c.bx_waves == 0 && kBxPlanTwoWave);
            if (want2 && bx_two_wave_fits(w, h, notail)) {
                const BxLayout l2(w, h, kBxUPT2, 1, kBxTile2);
                pq.bx_w2 = true;
                pq.bx_upt = kBxUPT2;
                pq.bx_lds = l2.total;
                d.bx_tre = bx_err_rows(w, h, l2.pb);
            }
            d.dv_bxpm = div_magic(bx_pm(w));
            d.dv_bxjr = div_magic(bx_jrp(w) / 4);
        }
    }
    // the class: the single-tile kernel for small windows, the box kernel for
    // Tracker2D boxes it holds in registers, else the large-window kernel (the
    // row-tiled kernel only when a variant asks for it and the window fits it)
    const bool forced = c.force_threads != 0;
    if (c.force_large) {
        pq.cls = kClsLg;
    } else if (pq.single && !c.force_generic && !(c.box_small && pq.bx_upt > 0)) {
        pq.cls = kClsSt;
    } else if (pq.bx_upt > 0 && c.box && !c.force_generic && !forced && !(no_bx16 && pq.bx_upt == 16)) {
        pq.cls = kClsBx;
        // (key % 10: 0 = the scalar-tail build, 1 = no-tail, 2 = no-tail two-wave)
        pq.key = 10 * pq.bx_upt + (pq.bx_w2 ? 2 : (sse && w % 8 == 0) ? 1 : 0);
    } else if (pq.tiled_tr > 0 && (c.force_generic || !c.box || forced)) {
        pq.cls = kClsTiled;
    } else {
        pq.cls = kClsLg;
    }
    if (pq.cls == kClsLg) {
        // (the kernel's LDS plan within the CU's: never an invalid launch)
        if (lg_lds_bytes(w, h, pq.lg_tr, pq.lg_jr, pq.lg_tq) > kMaxLdsBytes)
            return set_err(err, PSN_LK_ERR_UNSUPPORTED, "window %dx%d: large-window LDS plan above 160 KB", w, h);
        pq.key = pq.lg_tq;  // one launch per tile size
        d.tile_rows = pq.lg_tr;
        d.lg_jr = pq.lg_jr ? 1 : 0;
        if (pq.lg_jr) d.dv_bxjr = div_magic(bx_jrp(w) / 4);
    }
    if (pq.cls == kClsTiled) d.tile_rows = pq.tiled_tr;
    return PSN_LK_OK;
}

// Consecutive caller queries with the same plan and the same point count,
// their point blocks a constant stride apart, become one merged query of
// sub-queries (LkQueryDev::sub_pts; each keeps its points, its device count
// and its result slots, so the outputs are the same bits). Tracker2D's uniform
// boxes are one query per camera then, not one per detection, and a call of
// more than kMaxQueries detections -- configs[3]: 8 cameras x 32, the 4K Run:
// 8 x 64 -- is one launch per kernel class instead of one per 32 detections,
// each with its own tail.
void merge_sub_queries(std::vector<PlannedQuery> &plan) {
    if (plan.size() <= 1) return;
    auto same_plan = [](const PlannedQuery &x, const PlannedQuery &y) {
        const LkQueryDev &a = x.d, &b = y.d;
        return x.cls == y.cls && x.key == y.key && x.fcls == y.fcls && a.prev_slot == b.prev_slot && a.next_slot == b.next_slot &&
               a.num_pts == b.num_pts && a.win_w == b.win_w && a.win_h == b.win_h &&
               a.max_level == b.max_level && a.max_count == b.max_count && a.flags == b.flags &&
               a.tile_rows == b.tile_rows && a.min_eig == b.min_eig && a.eps2 == b.eps2 && a.dv_w == b.dv_w &&
               a.dv_dw == b.dv_dw && a.dv_pm == b.dv_pm && a.dv_jrw == b.dv_jrw && a.dv_jrw4 == b.dv_jrw4 &&
               a.dv_g == b.dv_g && a.dv_cw == b.dv_cw && a.ow_g == b.ow_g && a.ow_rg == b.ow_rg &&
               a.bx_tre == b.bx_tre && a.bx_hw == b.bx_hw && a.dv_bxpm == b.dv_bxpm && a.dv_bxjr == b.dv_bxjr &&
               x.single == y.single && x.st_lds == y.st_lds && x.ow_rows == y.ow_rows && x.ow_lds == y.ow_lds &&
               x.ovl_lds == y.ovl_lds && x.bx_upt == y.bx_upt && x.bx_lds == y.bx_lds && x.bx_w2 == y.bx_w2 &&
               x.tiled_tr == y.tiled_tr && x.lg_tr == y.lg_tr && x.lg_jr == y.lg_jr && x.lg_tq == y.lg_tq;
    };
    auto close = [&plan](size_t o, int nsub, int stride) {
        if (nsub <= 1) return;
        plan[o].d.sub_pts = plan[o].d.num_pts;
        plan[o].d.sub_pstride = stride;
        plan[o].d.num_pts *= nsub;
    };
    size_t o = 0;
    int nsub = 1, stride = 0;  // sub-queries of plan[o] so far, their point stride
    for (size_t i = 1; i < plan.size(); i++) {
        const PlannedQuery &f = plan[o], &x = plan[i];
        const int sp = nsub == 1 ? x.d.pt_begin - f.d.pt_begin : stride;
        if (same_plan(f, x) && x.src == f.src + nsub && sp >= f.d.num_pts && sp > 0 &&
            x.d.pt_begin == f.d.pt_begin + nsub * sp) {
            stride = sp;
            nsub++;
            continue;
        }
        close(o, nsub, stride);
        plan[++o] = plan[i];
        nsub = 1;
        stride = 0;
    }
    close(o, nsub, stride);
    plan.resize(o + 1);
}

// One launch of a planned group (queries of one class and key, <= kMaxQueries).
// fuse_given: an earlier launch of the call may take the deferred build already.
void plan_launch(const PlanCfg &c, PlannedQuery *const *grp, int n, int cls, int key, bool counted, int count_stride,
                 bool &fuse_given, LkLaunchPlan &L) {
    L.cls = cls;
    L.key = key;
    L.fcls = n ? grp[0]->fcls : 0;
    int wgs = 0, maxpx = 0, rows_ow = 0, lds_ow = 0, lds = 0;
    for (int i = 0; i < n; i++) {
        const PlannedQuery &pq = *grp[i];
        L.q[i] = pq.d;
        L.q[i].wg_begin = wgs;
        L.q[i].qidx = pq.src * count_stride;  // the query's count: d_counts[src * count_stride]
        wgs += pq.d.num_pts;
        maxpx = std::max(maxpx, pq.d.win_w * pq.d.win_h);
        rows_ow = std::max(rows_ow, pq.ow_rows);
        lds_ow = std::max(lds_ow, pq.ow_lds);
        lds = std::max(lds, pq.st_lds);
    }
    L.nq = n;
    L.wgs = wgs;
    if (wgs == 0) return;
    const int forced = c.force_threads;
    if (cls == kClsSt) {
        // single-tile kernel: (workgroup size, window pixels per thread)
        int nt = maxpx <= 128 ? 64 : maxpx <= 256 ? 128 : 256;
        if (forced == 64 || forced == 128 || forced == 256 || forced == 512) {
            const int max_ept = forced == 512 ? 2 : kStEPTMax;
            if (forced * max_ept >= maxpx) nt = forced;
        }
        int ept = nt == 512 ? (maxpx <= 512 ? 1 : 2) : (maxpx <= 2 * nt ? 2 : 4);
        int ow_e = 0, occ = 1;  // lk_kernel_st<nt, ept, ow_e, occ>
        // one-wave iterations (wave 0 iterates, waves 1-3 stage the next level)
        if (c.onewave && !forced && rows_ow <= kOwMaxRows) {
            const int oept = maxpx <= 512 ? 2 : 4;
            int E = rows_ow <= 4 ? 4 : rows_ow <= 7 ? 7 : rows_ow <= 8 ? 8 : 16;
            if (oept == 4 && E < 8) E = 8;
            nt = 256;
            ept = oept;
            ow_e = E;
            lds = lds_ow;
            // more points than two workgroups per CU hold, and LDS for three:
            // the 168-VGPR variant (three per CU; one-camera launches fit at two)
            if (oept == 2 && E <= 8 && lds_ow <= 53 * 1024 && wgs > 2 * c.num_cus) {
                occ = 3;
            } else if (c.st_ovl && E > 4) {
                // two workgroups per CU: the finer levels' A phase beside the
                // iterations, per query whose overlapped layout fits
                lds = 0;
                for (int i = 0; i < n; i++) {
                    const PlannedQuery &pq = *grp[i];
                    L.q[i].st_ovl = pq.ovl_lds > 0 ? 1 : 0;
                    lds = std::max(lds, pq.ovl_lds > 0 ? pq.ovl_lds : pq.ow_lds);
                }
            }
        }
        L.nt = nt;
        L.ept = ept;
        L.ow_e = ow_e;
        L.occ = occ;
        L.lds = lds;
        // early-exit workgroups cannot take part in a fused build
        L.may_fuse = !fuse_given && !counted;
        fuse_given |= L.may_fuse;
        return;
    }
    if (cls == kClsBx) {
        const int upt = key / 10;
        const bool notail = key % 10 != 0;
        const int nt = key % 10 == 2 ? kBxNT2 : kBxNT;
        const int tile = nt == kBxNT2 ? kBxTile2 : kBxTile;
        // the launch's UPT sizes every query's fallback planes; tiles as large as the
        // kernel's occupancy (bx_occupancy) allows -- the two-wave build keeps its
        // single quarter-wave tiles: a second one would pass the six-per-CU target
        int lds_bx = 0;
        for (int i = 0; i < n; i++) {
            LkQueryDev &d = L.q[i];
            d.bx_hw = 1;
            while (nt == kBxNT && d.bx_hw < 8 &&
                   BxLayout(d.win_w, d.win_h, upt, d.bx_hw + 1, tile).total <= bx_lds_target(upt, notail, nt))
                d.bx_hw++;
            lds_bx = std::max(lds_bx, BxLayout(d.win_w, d.win_h, upt, d.bx_hw, tile).total);
            if (bx_slides(d.win_w, nt)) L.slide_wgs += d.num_pts;
        }
        L.upt = upt;
        L.notail = notail;
        L.nt = nt;
        // the forward entry of the build: a launch-time choice (same queries, same
        // LDS plan, same launch group and key)
        L.fw = bx_fw_fits(upt, notail, nt) && c.fw != 1;
        L.lds = lds_bx;
        return;
    }
    if (cls == kClsTiled) {
        int threads = maxpx <= 1024 ? 64 : maxpx <= 4096 ? 128 : 256;
        if (forced == 64 || forced == 128 || forced == 256) threads = forced;
        lds = 0;
        for (int i = 0; i < n; i++) lds = std::max(lds, lk_lds_bytes(L.q[i].win_w, L.q[i].win_h, L.q[i].tile_rows));
        L.nt = threads;
        L.lds = lds;
        return;
    }
    // large windows: one HBM slot per workgroup, the grid strides over the points
    long long slot = 0;
    lds = 0;
    for (int i = 0; i < n; i++) {
        slot = std::max(slot, lg_slot_int2(L.q[i].win_w, L.q[i].win_h));
        lds = std::max(lds, lg_lds_bytes(L.q[i].win_w, L.q[i].win_h, L.q[i].tile_rows, L.q[i].lg_jr != 0, key));
    }
    const size_t slot_bytes = (size_t)slot * 8;
    // (within the budget also for the largest windows: one slot of a 2^24-px window
    // is ~100 MB, so no floor on the slot count past what the budget holds)
    const long long fit = std::max<long long>((long long)(kLgWsBudget / slot_bytes), 1);
    L.lg_slot = slot;
    L.grid = (int)std::min<long long>(wgs, fit);
    L.lds = lds;
}

}  // namespace

int plan_call(const PlanCfg &cfg, const psn_lk_query *q, int nq, const char *filled, bool allow_scratch, bool counted,
              int count_stride, LkCallPlan &out, std::string &err) {
    out.launches.clear();
    out.used_slots.clear();
    out.tag = 0;
    out.entry = 0;
    out.slide_wgs = 0;
    // plan every query first: a bad one fails the call before anything is launched
    std::vector<PlannedQuery> plan;
    plan.reserve((size_t)nq);
    for (int i = 0; i < nq; i++) {
        if (q[i].num_pts == 0) {
            if (q[i].params.win_w <= 2 || q[i].params.win_h <= 2)
                return set_err(err, PSN_LK_ERR_WINSIZE, "winSize %dx%d <= 2", q[i].params.win_w, q[i].params.win_h);
            continue;
        }
        plan.emplace_back();
        plan.back().src = i;
        int rc = plan_query(cfg, filled, q[i], allow_scratch, plan.back(), err);
        if (rc) return rc;
    }
    // The 16-unit box kernel (two workgroups per CU) beats the large-window kernel
    // on a launch of its own (512 points of 70x201: 513 vs 581 us), but a call
    // that holds large windows as well would launch one class more on the same
    // stream, each launch a fraction of the GPU with its own tail: there its
    // windows join the large-window launch (PETS-like boxes: 406 vs 450
    // camera-frames/s with the extra launch)
    // (per frame class: a large-window launch of another class is another launch anyway)
    unsigned lg_classes = 0;
    for (const PlannedQuery &pq : plan)
        if (pq.cls == kClsLg) lg_classes |= 1u << pq.fcls;
    if (lg_classes)
        for (PlannedQuery &pq : plan)
            if (pq.cls == kClsBx && pq.bx_upt == 16 && (lg_classes >> pq.fcls & 1)) {
                PlannedQuery lq;
                lq.src = pq.src;
                int rc = plan_query(cfg, filled, q[pq.src], allow_scratch, lq, err, true);
                if (rc) return rc;
                pq = lq;
            }
    merge_sub_queries(plan);
    for (const PlannedQuery &pq : plan)
        for (int sl : {pq.d.prev_slot, pq.d.next_slot})
            if (std::find(out.used_slots.begin(), out.used_slots.end(), sl) == out.used_slots.end())
                out.used_slots.push_back(sl);
    // launch groups: (class, key, frame class) in a fixed order, queries in call
    // order; the frame class rides in the pair's second member above the key
    auto group_of = [](const PlannedQuery &pq) { return std::pair<int, int>(pq.cls, pq.key + (pq.fcls << kFclsShift)); };
    auto key_of = [](const std::pair<int, int> &g) { return g.second & ((1 << kFclsShift) - 1); };
    std::vector<std::pair<int, int>> groups;
    std::vector<long long> group_px;
    for (const PlannedQuery &pq : plan) {
        const std::pair<int, int> g = group_of(pq);
        const long long px = (long long)pq.d.win_w * pq.d.win_h * pq.d.num_pts;
        auto it = std::find(groups.begin(), groups.end(), g);
        if (it == groups.end()) {
            groups.push_back(g);
            group_px.push_back(px);
        } else {
            group_px[it - groups.begin()] += px;
        }
    }
    bool fuse_given = false;
    PlannedQuery *grp[kMaxQueries];
    int n = 0;
    auto flush = [&](const std::pair<int, int> &g) {
        out.launches.emplace_back();
        plan_launch(cfg, grp, n, g.first, key_of(g), counted, count_stride, fuse_given, out.launches.back());
        if (out.launches.back().wgs == 0) out.launches.pop_back();
        n = 0;
    };
    for (const auto &g : groups) {
        for (PlannedQuery &pq : plan) {
            if (group_of(pq) != g) continue;
            grp[n++] = &pq;
            if (n == kMaxQueries) flush(g);
        }
        if (n) flush(g);
    }
    for (const LkLaunchPlan &L : out.launches) out.slide_wgs += L.slide_wgs;
    if (!groups.empty()) {
        const size_t dom = (size_t)(std::max_element(group_px.begin(), group_px.end()) - group_px.begin());
        const int dcls = groups[dom].first, dkey = key_of(groups[dom]);
        out.tag = kernel_tag(dcls, dkey) + (groups.size() > 1 ? 1000 : 0);
        bool fw = false;  // (a group's launches share their build, hence their entry)
        for (const LkLaunchPlan &L : out.launches) fw |= L.cls == dcls && L.key == dkey && L.fw;
        out.entry = entry_tag(dcls, dkey, fw) + (groups.size() > 1 ? 1000 : 0);
    }
    return PSN_LK_OK;
}

}  // namespace psn
