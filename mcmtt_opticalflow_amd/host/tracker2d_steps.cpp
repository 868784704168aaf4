// The reference's Tracker2D steps (see tracker2d_steps.hpp). Reference lines
// cited are in psn_where/PSNWhere_Tracker2D.cpp unless noted.
#include "tracker2d_steps.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace psn {

// :452-554. Vectors with |d| >= 0.1 px vote; if fewer than half the points
// move, the box stays put with no inliers. Otherwise the mode of dx and of dy
// (most neighbours within 0.2 box widths, first maximum in sorted order) is
// the box shift and the inliers are the moving vectors within that window of
// the mode, in point order.
Rect LocalSearchKLT(Rect preBox, const std::vector<Point2f> &preFeatures, const std::vector<Point2f> &curFeatures,
                    std::vector<size_t> &inlierFeatureIndex, double scale) {
    const double kMinMovement = 0.1, kNeighborRatio = 0.2;
    const size_t numFeatures = preFeatures.size();
    size_t numMoving = 0;
    inlierFeatureIndex.clear();
    std::vector<Point2D> vecMoving;
    std::vector<size_t> vecMovingIdx;
    std::vector<double> vecDx, vecDy;
    for (size_t i = 0; i < numFeatures; i++) {
        // cv::Point2f difference (float), then widened to PSN_Point2D
        const Point2f d{curFeatures[i].x - preFeatures[i].x, curFeatures[i].y - preFeatures[i].y};
        const Point2D mv(d);
        if (mv.norm_L2() < kMinMovement * scale) continue;
        vecMoving.push_back(mv);
        vecMovingIdx.push_back(i);
        vecDx.push_back(mv.x);
        vecDy.push_back(mv.y);
        numMoving++;
    }
    if ((double)numMoving < (double)numFeatures * 0.5) return preBox;
    std::sort(vecDx.begin(), vecDx.end());
    std::sort(vecDy.begin(), vecDy.end());
    const double windowSize = preBox.w * kNeighborRatio * scale;
    size_t maxX = 0, maxY = 0;
    Point2D est(0.0, 0.0);
    // neighbour counts |v[d] - v[c]| < windowSize of every d. On sorted finite
    // values with windowSize > 0 the neighbours of d are one index range [lo, hi)
    // whose ends never decrease with d (fl(a - b) is monotone in a and b, and
    // |fl(a - b)| = fl(b - a)), so two pointers count exactly what the reference's
    // double loop counts; otherwise (NaN, windowSize <= 0) that loop itself.
    const bool finite = windowSize > 0 &&
                        std::all_of(vecDx.begin(), vecDx.end(), [](double v) { return std::isfinite(v); }) &&
                        std::all_of(vecDy.begin(), vecDy.end(), [](double v) { return std::isfinite(v); });
    auto counts = [&](const std::vector<double> &v, std::vector<size_t> &cnt) {
        cnt.assign(numMoving, 0);
        if (finite) {
            size_t lo = 0, hi = 0;
            for (size_t d = 0; d < numMoving; d++) {
                while (!(v[d] - v[lo] < windowSize)) lo++;  // lo <= d: v[d] - v[d] = 0 < windowSize
                if (hi < d + 1) hi = d + 1;
                while (hi < numMoving && v[hi] - v[d] < windowSize) hi++;
                cnt[d] = hi - lo;
            }
        } else {
            for (size_t d = 0; d < numMoving; d++)
                for (size_t c = 0; c < numMoving; c++)
                    if (std::abs(v[d] - v[c]) < windowSize) cnt[d]++;
        }
    };
    std::vector<size_t> cntX, cntY;
    counts(vecDx, cntX);
    counts(vecDy, cntY);
    for (size_t d = 0; d < numMoving; d++) {
        if (maxX < cntX[d]) {
            est.x = vecDx[d];
            maxX = cntX[d];
        }
        if (maxY < cntY[d]) {
            est.y = vecDy[d];
            maxY = cntY[d];
        }
    }
    for (size_t v = 0; v < numMoving; v++)
        if ((vecMoving[v] - est).norm_L2() < windowSize) inlierFeatureIndex.push_back(vecMovingIdx[v]);
    Rect box = preBox;
    box.x += est.x;
    box.y += est.y;
    return box;
}

// :600-613
double BoxMatchingCost(const Rect &box1, const Rect &box2) {
    const double nom = (box1.center() - box2.center()).norm_L2();
    const double den = (box1.w + box2.w) / 2.0;
    return (nom * nom) / (den * den);
}

// :1231-1257 (PSN_2D_DEBUG_DISPLAY_SCALE = 1.0: the float scaling is exact)
void ResultWithTracker(const Tracker2D &tracker, Object2DInfo &out) {
    const float s = 1.0f;
    out.featurePointsPrev = tracker.featurePoints;
    out.featurePointsCurr = tracker.trackedPoints;
    out.id = tracker.id;
    const Rect &b = tracker.boxes.back(), &h = tracker.heads.back();
    out.box = Rect(b.x * s, b.y * s, b.w * s, b.h * s);
    out.head = Rect(h.x * s, h.y * s, h.w * s, h.h * s);
    out.score = 0;
    for (size_t i = 0; i < out.featurePointsPrev.size(); i++) {
        out.featurePointsPrev[i].x *= s;
        out.featurePointsPrev[i].y *= s;
        if (i >= out.featurePointsCurr.size()) continue;
        out.featurePointsCurr[i].x *= s;
        out.featurePointsCurr[i].y *= s;
    }
}

// ---------------------------------------------------------------------------
// Backward chain (:690-838)
// ---------------------------------------------------------------------------

void BackwardBegin(const std::vector<Detection> &dets, const std::vector<std::vector<Point2f>> &features,
                   std::vector<DetectedObject> &out, std::vector<Chain> &chains) {
    out.clear();
    chains.clear();
    for (size_t i = 0; i < dets.size(); i++) {
        DetectedObject o;
        o.id = (unsigned)i;  // detectionID counts every detection past the height gate (:718)
        o.detection = dets[i];
        for (int k = 0; k < 3; k++) o.location[k] = dets[i].location[k];
        o.height = dets[i].height;
        o.boxes.push_back(dets[i].box);
        const std::vector<Point2f> &f = features[i];
        if (f.size() < kT2dMinFeatures) continue;  // :744
        Chain c;
        c.curr.assign(f.begin(), f.begin() + std::min(f.size(), kT2dMaxFeatures));  // :753-757
        c.obj = out.size();
        c.active = true;
        out.push_back(std::move(o));
        chains.push_back(std::move(c));
    }
}

void BackwardJobs(int step, const int *ring, double scale, std::vector<Chain> &chains,
                  const std::vector<DetectedObject> &out, std::vector<Job> &jobs) {
    for (Chain &c : chains) {
        if (!c.active) continue;
        const Rect box = out[c.obj].detection.box.scale(scale);
        const int win = (int)(box.w * kWinSizeRatio);  // square window of the box width (:782)
        jobs.push_back(
            Job{ring[kT2dInterval - step], ring[kT2dInterval - 1 - step], win, win, &c.curr, &c.prev, &c.status});
    }
}

void BackwardStepDone(std::vector<Chain> &chains, std::vector<DetectedObject> &out, double scale) {
    std::vector<size_t> inl;
    for (Chain &c : chains) {
        if (!c.active) continue;
        DetectedObject &o = out[c.obj];
        // status is ignored: every nextPts value feeds LocalSearchKLT (:787)
        const Rect newRect = LocalSearchKLT(o.detection.box.scale(scale), c.curr, c.prev, inl, scale);
        if (inl.size() < kT2dMinFeatures) {  // :788
            c.active = false;
            continue;
        }
        o.boxes.push_back(newRect.scale(1.0 / scale));
        if (o.vecvecTrackedFeatures.empty()) {
            std::vector<Point2f> cur;
            for (size_t k : inl) cur.push_back(c.curr[k]);
            o.vecvecTrackedFeatures.push_back(cur);
        }
        std::vector<Point2f> next;
        next.reserve(inl.size());
        for (size_t k : inl) next.push_back(c.prev[k]);
        o.vecvecTrackedFeatures.push_back(next);
        c.curr.swap(next);
    }
}

void BackwardEnd(std::vector<DetectedObject> &out, const std::vector<std::vector<Point2f>> &features) {
    for (DetectedObject &o : out)  // no step kept >= 4 inliers: the features at t (:815-818)
        if (o.vecvecTrackedFeatures.empty()) {
            const std::vector<Point2f> &f = features[o.id];
            o.vecvecTrackedFeatures.emplace_back(f.begin(), f.begin() + (ptrdiff_t)std::min(f.size(), kT2dMaxFeatures));
        }
    // overlap flags (:824-835)
    for (size_t a = 0; a < out.size(); a++) {
        if (out[a].bOverlapWithOtherDetection) continue;
        for (size_t b = a + 1; b < out.size(); b++)
            if (out[a].detection.box.overlap(out[b].detection.box)) {
                out[a].bOverlapWithOtherDetection = true;
                break;
            }
    }
}

// ---------------------------------------------------------------------------
// Forward tracking + matching score (:851-1025)
// ---------------------------------------------------------------------------

void ForwardJobs(const int *ring, double scale, const std::vector<Tracker2D *> &trackers,
                 std::vector<std::vector<uint8_t>> &status, std::vector<Job> &jobs) {
    status.assign(trackers.size(), {});
    for (size_t t = 0; t < trackers.size(); t++) {
        Tracker2D *tr = trackers[t];
        tr->trackedPoints.clear();
        const Rect cur = tr->boxes.back().scale(scale);
        jobs.push_back(Job{ring[kT2dInterval - 2], ring[kT2dInterval - 1], (int)(cur.w * kWinSizeRatio),
                           (int)(cur.h * kWinSizeRatio), &tr->featurePoints, &tr->trackedPoints, &status[t]});
    }
}

void ForwardDone(const std::vector<Tracker2D *> &trackers, std::vector<std::vector<uint8_t>> &status,
                 const std::vector<DetectedObject> &dets, std::vector<float> &cost, double scale) {
    const double kBoxMaxDistance = 1.0, kMinOverlapRatio = 0.3, kMaxCenterDiffRatio = 0.5, kMajority = 0.5;
    const size_t T = trackers.size(), D = dets.size();
    const float inf = std::numeric_limits<float>::infinity();
    cost.assign(D * T, inf);
    std::vector<std::deque<int>> inBox(D);
    std::vector<size_t> inl;
    for (size_t t = 0; t < T; t++) {
        Tracker2D *tr = trackers[t];
        std::vector<Point2f> vPrev, vCurr;
        for (size_t i = 0; i < status[t].size(); i++) {  // keep status == 1 (:883-888)
            if (!status[t][i]) continue;
            vPrev.push_back(tr->featurePoints[i]);
            vCurr.push_back(tr->trackedPoints[i]);
        }
        if (vCurr.size() < kT2dMinFeatures) continue;  // :889 (featurePoints kept, trackedPoints = raw output)
        Rect newBox = LocalSearchKLT(tr->boxes.back().scale(scale), vPrev, vCurr, inl, scale);
        newBox = newBox.scale(1.0 / scale);
        tr->boxes.push_back(newBox);
        tr->heads.push_back(tr->heads.empty() ? Rect() : tr->heads.back());
        for (size_t d = 0; d < D; d++) {
            const DetectedObject &det = dets[d];
            const size_t pos = d * T + t;
            if (!newBox.overlap(det.detection.box)) continue;
            for (const Point2f &p : tr->trackedPoints)  // the raw LK output (:914-918)
                if (det.detection.box.contain(p)) inBox[d].push_back((int)t);
            double boxCost = 0.0;
            const size_t len = std::min((size_t)kT2dInterval, std::min(tr->boxes.size(), det.boxes.size()));
            size_t tb = (size_t)tr->duration;  // duration = #boxes - 1
            for (size_t b = 0; b < len; b++, tb--) {
                // after a failed frame a tracker's duration (frame based, :1085) runs
                // past its boxes: the reference reads outside the vector (undefined);
                // here the pair cannot match (as oracle/tracker2d_oracle.py)
                if (tb >= tr->boxes.size()) {
                    boxCost = std::numeric_limits<double>::infinity();
                    break;
                }
                const Rect &db = det.boxes[b], &trb = tr->boxes[tb];
                if (!db.overlap(trb) || kBoxMaxDistance < db.distance(trb) ||
                    kMinOverlapRatio > db.overlappedArea(trb) / std::min(db.area(), trb.area()) ||
                    kMaxCenterDiffRatio * std::max(db.w, trb.w) < (db.center() - trb.center()).norm_L2()) {
                    boxCost = std::numeric_limits<double>::infinity();
                    break;
                }
                boxCost += BoxMatchingCost(trb, db);
            }
            if (std::numeric_limits<double>::infinity() == boxCost) continue;
            boxCost /= (double)len;
            cost[pos] = (float)boxCost;
        }
        tr->featurePoints = vPrev;  // :977-978
        tr->trackedPoints = vCurr;
    }
    // feature-point majority check (:982-1022), run lengths as the reference counts them
    for (size_t d = 0; d < D; d++) {
        const std::deque<int> &f = inBox[d];
        if (f.empty()) continue;
        int nMajor = 0, nCur = 0;
        int major = f.front(), cur = f.front();
        for (size_t k = 0; k < f.size(); k++) {
            if (cur == f[k]) {
                nCur++;
                continue;
            }
            if (nCur > nMajor) {
                major = cur;
                nMajor = nCur;
            }
            cur = f[k];
            nCur = 0;
        }
        (void)major;
        if (f.front() == cur) nMajor = nCur;  // sole tracker
        if ((double)nMajor > (double)f.size() * kMajority) continue;
        for (size_t t = 0; t < T; t++) cost[d * T + t] = inf;
    }
}

}  // namespace psn
