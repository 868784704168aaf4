// Prints what psn::plan_call plans for the sweep of lk_plan_sweep.h, one JSON
// line per call (tests/test_lk_plan.py compares the lines with the record in
// tests/golden/lk_plan_parent.jsonl). Links psn_lk_plan.cpp and nothing else of
// the library: no GPU, no libpsn_lk.so.
//
//   lk_plan_dump                  the sweep
//   lk_plan_dump --time N [WxH]   ns per plan_call of the Tracker2D call shape
//                                 (8 cameras x 32 uniform queries), N calls
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "lk_plan_sweep.h"

static void run_case(const sweep::Case &c) {
    psn::LkCallPlan plan;
    std::string err;
    const int rc = psn::plan_call(c.cfg, c.q.data(), (int)c.q.size(), c.filled.data(), c.allow_scratch, c.counted,
                                  c.count_stride, plan, err);
    std::vector<sweep::Launch> ls;
    for (const psn::LkLaunchPlan &p : plan.launches) {
        sweep::Launch l;
        l.kernel = p.cls == psn::kClsSt ? "st" : p.cls == psn::kClsBx ? "bx" : p.cls == psn::kClsTiled ? "tiled" : "lg";
        l.nq = p.nq;
        l.q = p.q;
        l.wgs = p.wgs;
        l.grid = p.cls == psn::kClsLg ? p.grid : p.wgs;
        l.lds = p.lds;
        l.fuse = p.may_fuse;
        l.nt = p.nt;
        l.ept = p.ept;
        l.ow_e = p.ow_e;
        l.occ = p.cls == psn::kClsSt ? p.occ : 0;
        l.upt = p.upt;
        l.notail = p.notail;
        l.tq = p.cls == psn::kClsLg ? p.key : 0;
        l.lg_slot = p.lg_slot;
        ls.push_back(l);
    }
    sweep::print_case(c, rc, err, plan.used_slots, plan.tag, ls);
}

int main(int argc, char **argv) {
    if (argc >= 3 && !strcmp(argv[1], "--time")) {
        const long n = atol(argv[2]);
        int w = 64, h = 64;
        if (argc >= 4) sscanf(argv[3], "%dx%d", &w, &h);
        const psn::PlanCfg g = sweep::frame(1920, 1080);
        std::vector<psn_lk_query> q;
        for (int i = 0; i < 8 * 32; i++) q.push_back(sweep::query(w, h, 24, 24 * i, 0, 3, (i / 32) % 4, (i / 32 + 1) % 4));
        const std::vector<char> filled((size_t)g.nslots, 1);
        psn::LkCallPlan plan;  // kept between calls, as a context keeps it
        std::string err;
        long long sink = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (long i = 0; i < n; i++) {
            if (psn::plan_call(g, q.data(), (int)q.size(), filled.data(), false, false, 1, plan, err)) return 1;
            sink += plan.launches.size() + plan.launches[0].wgs;
        }
        const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
        printf("plan_call %dx%d: %.0f ns per call (%ld calls, check %lld)\n", w, h, ns / (double)n, n, sink);
        return 0;
    }
    sweep::sweep_cases(run_case);
    return 0;
}
