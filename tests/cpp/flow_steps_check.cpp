// TEST HARNESS: a stand-alone caller of the reference's Tracker2D steps
// (mcmtt_opticalflow_amd/host/tracker2d_steps.cpp), compiled together with it
// and tracker2d_match.cpp under -fsanitize=address,undefined by
// tests/test_flow_steps.py. It reads a case file, runs the backward chain loop
// (BackwardBegin; BackwardJobs + BackwardStepDone per step; BackwardEnd) and
// ForwardJobs + ForwardDone, and prints every job, box, point set, overlap flag
// and cost (floats as %a). No LK runs: the output of a job is the point set the
// case file supplies for it.
//
// Case file, whitespace-separated (floats in any strtod form, hex included):
//   scale S  npast P  ring r0 r1 r2 r3
//   dets D   then per detection:  x y w h  n  (x y)*n
//   bsets B  then per set:  det step n  (x y)*n  (status)*n
//   trackers T  then per tracker:  duration  nboxes (x y w h)*nboxes  n (x y)*n  (x y)*n (status)*n
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "tracker2d_steps.hpp"

using namespace psn;

static FILE *in = nullptr;

static std::string token() {
    char buf[64];
    if (std::fscanf(in, "%63s", buf) != 1) {
        std::printf("FAILED: case file ends early\n");
        std::exit(2);
    }
    return buf;
}
static double num() { return std::strtod(token().c_str(), nullptr); }
static size_t count() { return (size_t)std::strtoul(token().c_str(), nullptr, 10); }
static void expect(const char *word) {
    const std::string t = token();
    if (t != word) {
        std::printf("FAILED: expected '%s' in the case file, found '%s'\n", word, t.c_str());
        std::exit(2);
    }
}
static Rect rect() {
    const double x = num(), y = num(), w = num(), h = num();
    return Rect(x, y, w, h);
}
static std::vector<Point2f> points(size_t n) {
    std::vector<Point2f> v(n);
    for (Point2f &p : v) {
        p.x = (float)num();
        p.y = (float)num();
    }
    return v;
}
static std::vector<uint8_t> bytes(size_t n) {
    std::vector<uint8_t> v(n);
    for (uint8_t &b : v) b = (uint8_t)count();
    return v;
}

static void print_box(const char *what, const Rect &r) { std::printf("%s %a %a %a %a\n", what, r.x, r.y, r.w, r.h); }
static void print_points(const char *what, const std::vector<Point2f> &v) {
    std::printf("%s %zu", what, v.size());
    for (const Point2f &p : v) std::printf(" %a %a", (double)p.x, (double)p.y);
    std::printf("\n");
}

struct Supplied {
    std::vector<Point2f> pts;
    std::vector<uint8_t> status;
};
// the "LK" of a job: the supplied set, which must fit the job's input
static void supply(const Job &jb, const Supplied &s) {
    if (s.pts.size() != jb.in->size()) {
        std::printf("FAILED: a supplied set holds %zu points, the job %zu\n", s.pts.size(), jb.in->size());
        std::exit(2);
    }
    *jb.out = s.pts;
    *jb.status = s.status;
}

int main(int argc, char **argv) {
    if (argc != 2 || !(in = std::fopen(argv[1], "r"))) {
        std::printf("usage: flow_steps_check CASEFILE\n");
        return 2;
    }
    expect("scale");
    const double scale = num();
    expect("npast");
    const int npast = (int)count();
    expect("ring");
    int ring[kT2dInterval];
    for (int &r : ring) r = (int)count();

    expect("dets");
    const size_t D = count();
    std::vector<Detection> dets(D);
    std::vector<std::vector<Point2f>> features(D);
    for (size_t i = 0; i < D; i++) {
        dets[i].box = rect();
        features[i] = points(count());
    }
    expect("bsets");
    std::map<std::pair<unsigned, int>, Supplied> bsets;
    for (size_t n = count(); n > 0; n--) {
        const unsigned det = (unsigned)count();
        const int step = (int)count();
        const size_t m = count();
        Supplied &s = bsets[{det, step}];
        s.pts = points(m);
        s.status = bytes(m);
    }
    expect("trackers");
    const size_t T = count();
    std::vector<Tracker2D> storage(T);
    std::vector<Supplied> fsets(T);
    std::vector<Tracker2D *> trackers;
    for (size_t t = 0; t < T; t++) {
        Tracker2D &tr = storage[t];
        tr.duration = (unsigned)count();
        for (size_t n = count(); n > 0; n--) tr.boxes.push_back(rect());
        tr.heads = tr.boxes;
        const size_t m = count();
        tr.featurePoints = points(m);
        fsets[t].pts = points(m);
        fsets[t].status = bytes(m);
        trackers.push_back(&tr);
    }
    std::fclose(in);

    // the backward chain loop, as Tracker2DFlow::BackwardFeatureTracking drives it
    std::vector<DetectedObject> out;
    std::vector<Chain> chains;
    std::vector<Job> jobs;
    BackwardBegin(dets, features, out, chains);
    for (int step = 1; step <= npast; step++) {
        jobs.clear();
        BackwardJobs(step, ring, scale, chains, out, jobs);
        if (jobs.empty()) break;
        size_t j = 0;
        for (const Chain &c : chains) {  // one job per running chain, in chain order
            if (!c.active) continue;
            const Job &jb = jobs[j++];
            const unsigned det = out[c.obj].id;
            std::printf("job bwd %u %d %d %d %d %d\n", det, step, jb.prev_slot, jb.next_slot, jb.win_w, jb.win_h);
            const auto it = bsets.find({det, step});
            if (jb.in != &c.curr || it == bsets.end()) {
                std::printf("FAILED: no supplied set for detection %u step %d\n", det, step);
                return 2;
            }
            supply(jb, it->second);
        }
        BackwardStepDone(chains, out, scale);
    }
    BackwardEnd(out, features);
    for (const DetectedObject &o : out) {
        std::printf("obj %u overlap %d nboxes %zu nsets %zu\n", o.id, (int)o.bOverlapWithOtherDetection, o.boxes.size(),
                    o.vecvecTrackedFeatures.size());
        for (const Rect &r : o.boxes) print_box("box", r);
        for (const std::vector<Point2f> &s : o.vecvecTrackedFeatures) print_points("set", s);
    }

    // forward tracking + matching score
    std::vector<std::vector<uint8_t>> status;
    std::vector<float> cost;
    jobs.clear();
    ForwardJobs(ring, scale, trackers, status, jobs);
    for (size_t t = 0; t < jobs.size(); t++) {
        std::printf("job fwd %zu %d %d %d %d\n", t, jobs[t].prev_slot, jobs[t].next_slot, jobs[t].win_w, jobs[t].win_h);
        supply(jobs[t], fsets[t]);
    }
    ForwardDone(trackers, status, out, cost, scale);
    for (size_t t = 0; t < T; t++) {
        const Tracker2D &tr = storage[t];
        std::printf("trk %zu nboxes %zu nheads %zu\n", t, tr.boxes.size(), tr.heads.size());
        for (const Rect &r : tr.boxes) print_box("box", r);
        for (const Rect &r : tr.heads) print_box("head", r);
        print_points("feat", tr.featurePoints);
        print_points("tracked", tr.trackedPoints);
    }
    std::printf("cost %zu %zu\n", out.size(), T);
    for (size_t d = 0; d < out.size(); d++) {
        std::printf("row");
        for (size_t t = 0; t < T; t++) std::printf(" %a", (double)cost[d * T + t]);
        std::printf("\n");
    }
    std::printf("flow steps check: ok\n");
    return 0;
}
