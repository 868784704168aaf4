// The launch planner with frame classes (psn::PlanCfg::cls), alone on the CPU:
// links psn_lk_plan.cpp and nothing else of the library. Prints, as its last line,
// one JSON object that tests/test_lk_plan_classes.py checks:
//   "mixed"   one call with queries on two classes (320x240 in slots 0-3,
//             200x150 in slots 4-7): its launches with their frame class
//   "merge"   identical consecutive queries, four per class, regular point stride
//   "cross"   a query whose two slots lie in different classes
//   "scratch" the one-shot call's scratch slots (class 0) in a two-class context
//   "sweep"   every case of lk_plan_sweep.h planned without a class table and with
//             a one-entry table: cases, and those that planned differently
#include <cstring>

#include "lk_plan_sweep.h"

using namespace psn;

static PlanCfg two_classes() {
    PlanCfg g = sweep::frame(320, 240);
    g.user_slots = 8;
    g.nslots = 10;
    g.ncls = 2;
    g.cls[0] = PlanFrameClass{320, 240, 0, 4};
    g.cls[1] = PlanFrameClass{200, 150, 4, 4};
    return g;
}

static void print_plan(const char *name, const PlanCfg &g, const std::vector<psn_lk_query> &q, bool scratch, bool counted) {
    const std::vector<char> filled((size_t)g.nslots, 1);
    LkCallPlan p;
    std::string err;
    const int rc = plan_call(g, q.data(), (int)q.size(), filled.data(), scratch, counted, 1, p, err);
    printf("\"%s\": {\"rc\": %d, \"err\": \"%s\", \"tag\": %d, \"used\": [", name, rc, rc ? err.c_str() : "", p.tag);
    for (size_t i = 0; i < p.used_slots.size(); i++) printf("%s%d", i ? ", " : "", p.used_slots[i]);
    printf("], \"launches\": [");
    for (size_t i = 0; i < p.launches.size(); i++) {
        const LkLaunchPlan &L = p.launches[i];
        printf("%s{\"cls\": %d, \"key\": %d, \"fcls\": %d, \"wgs\": %d, \"fuse\": %d, \"q\": [", i ? ", " : "", L.cls, L.key,
               L.fcls, L.wgs, (int)L.may_fuse);
        for (int k = 0; k < L.nq; k++) {
            const LkQueryDev &d = L.q[k];
            printf("%s{\"prev\": %d, \"next\": %d, \"prev_cls\": %d, \"next_cls\": %d, \"w\": %d, \"h\": %d, \"max_level\": %d, "
                   "\"num_pts\": %d, \"sub_pts\": %d, \"qidx\": %d}",
                   k ? ", " : "", d.prev_slot, d.next_slot, g.slot_class(d.prev_slot), g.slot_class(d.next_slot), d.win_w,
                   d.win_h, d.max_level, d.num_pts, d.sub_pts, d.qidx);
        }
        printf("]}");
    }
    printf("]}");
}

// A planned call as text: everything lk_plan_dump prints of it, and the launches' frame class.
static std::string plan_text(const sweep::Case &c, const PlanCfg &g) {
    LkCallPlan p;
    std::string err, s;
    const int rc = plan_call(g, c.q.data(), (int)c.q.size(), c.filled.data(), c.allow_scratch, c.counted, c.count_stride, p, err);
    sweep::appendf(s, "%d|%s|%d|%d|%d|", rc, rc ? err.c_str() : "", p.tag, p.entry, p.slide_wgs);
    for (int u : p.used_slots) sweep::appendf(s, "%d,", u);
    for (const LkLaunchPlan &L : p.launches) {
        sweep::Launch l;
        l.kernel = L.cls == kClsSt ? "st" : L.cls == kClsBx ? "bx" : L.cls == kClsTiled ? "tiled" : "lg";
        l.nq = L.nq;
        l.q = L.q;
        l.wgs = L.wgs;
        l.grid = L.grid;
        l.lds = L.lds;
        l.fuse = L.may_fuse;
        l.nt = L.nt;
        l.ept = L.ept;
        l.ow_e = L.ow_e;
        l.occ = L.occ;
        l.upt = L.upt;
        l.notail = L.notail;
        l.tq = L.key;
        l.lg_slot = L.lg_slot;
        sweep::append_launch(s, l, false);
        sweep::appendf(s, "|%d,%d,%d,%d", L.cls, (int)L.fw, L.slide_wgs, L.fcls);
    }
    return s;
}

int main() {
    const PlanCfg g = two_classes();
    int cases = 0, differ = 0;
    std::string first_diff;
    // (sweep_cases prints its legend first: the object below is the last line)
    sweep::sweep_cases([&](const sweep::Case &c) {
        PlanCfg one = c.cfg;
        one.ncls = 1;
        one.cls[0] = PlanFrameClass{c.cfg.width, c.cfg.height, 0, c.cfg.user_slots};
        cases++;
        if (plan_text(c, c.cfg) != plan_text(c, one)) {
            if (!differ++) first_diff = c.name;
        }
    });
    printf("{\"levels\": [%d, %d], ", psn_lk_effective_max_level(320, 240, 32, 80, 3),
           psn_lk_effective_max_level(200, 150, 32, 80, 3));
    {
        std::vector<psn_lk_query> q;
        int pt = 0;
        const int wins[][2] = {{21, 21}, {32, 32}, {32, 80}};
        for (int k = 0; k < 2; k++)  // the classes interleaved per window
            for (auto &w : wins) {
                for (int c = 0; c < 2; c++) {
                    q.push_back(sweep::query(w[0], w[1], 12, pt, 0, 3, 4 * c, 4 * c + 1 + k));
                    pt += 12;
                }
            }
        q.push_back(sweep::query(70, 201, 12, pt, 0, 3, 0, 1));
        print_plan("mixed", g, q, false, false);
    }
    printf(", ");
    {
        // Tracker2D's shape: uniform boxes, one query per detection, a camera after the other
        std::vector<psn_lk_query> q;
        for (int i = 0; i < 8; i++) q.push_back(sweep::query(32, 32, 100, 100 * i, 0, 3, i < 4 ? 1 : 5, i < 4 ? 0 : 4));
        print_plan("merge", g, q, false, true);
    }
    printf(", ");
    print_plan("cross", g, {sweep::query(21, 21, 12, 0, 0, 3, 0, 1), sweep::query(21, 21, 12, 12, 0, 3, 3, 4)}, false, false);
    printf(", ");
    print_plan("scratch", g, {sweep::query(32, 80, 12, 0, 0, 3, 8, 9)}, true, false);
    printf(", \"sweep\": {\"cases\": %d, \"differ\": %d, \"first\": \"%s\"}}\n", cases, differ, first_diff.c_str());
    return 0;
}
