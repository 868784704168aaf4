// The reference's Tracker2D steps as plain host arithmetic: LocalSearchKLT
// (psn_where/PSNWhere_Tracker2D.cpp:452-554), BoxMatchingCost (:600-613), the
// backward chain's bookkeeping (:690-838), the forward matching score with its
// majority gate (:851-1025), and, in tracker2d_match.cpp, the assignment and
// tracker update (:1038-1164) with ResultWithTracker (:1231-1257). No device and
// no LK library: an LK call is a Job record the caller runs. Tracker2DFlow
// (tracker2d_flow.hpp) drives these steps.
#pragma once

#include <cstddef>
#include <cstdint>
#include <list>
#include <vector>

#include "psn_types.hpp"

namespace psn {

constexpr int kT2dInterval = 4;          // PSN_2D_BACKTRACKING_INTERVAL (:16)
// the ring + two staging slots: frame t+2 uploads (and its pyramid builds) while
// frame t+1 waits staged and frame t runs
constexpr int kT2dStaging = 2;
constexpr int kSlotsPerCam = kT2dInterval + kT2dStaging;
constexpr size_t kT2dMinFeatures = 4;    // PSN_2D_FEATURE_MIN_NUM_TRACK (:12)
constexpr size_t kT2dMaxFeatures = 100;  // PSN_2D_FEATURE_MAX_NUM_TRACK (:13)
constexpr int kT2dResBlocks = 3;         // chain result blocks used in turn by consecutive passes
// PSN_2D_OPTICALFLOW_SCALE (:18) is a runtime value here: Tracker2DFlow's scale,
// the `scale` argument of the steps (a product with a runtime 1.0 is exact,
// so one code path serves both of the reference's builds)
constexpr double kWinSizeRatio = 1.0;    // PSN_2D_FEATURE_WIN_SIZE_RATIO (:15)

struct Job {  // one calcOpticalFlowPyrLK call
    int prev_slot, next_slot, win_w, win_h;
    const std::vector<Point2f> *in;
    std::vector<Point2f> *out;
    std::vector<uint8_t> *status;
};
struct Chain {  // one detection's backward chain (host-chain mode)
    size_t obj;
    std::vector<Point2f> curr, prev;
    std::vector<uint8_t> status;
    bool active;
};

// preBox is the box already scaled; scale enters the minimum movement (:481) and,
// a second time, the neighbour window (:502), as in the reference
Rect LocalSearchKLT(Rect preBox, const std::vector<Point2f> &preFeatures, const std::vector<Point2f> &curFeatures,
                    std::vector<size_t> &inlierFeatureIndex, double scale = 1.0);
double BoxMatchingCost(const Rect &box1, const Rect &box2);
void ResultWithTracker(const Tracker2D &tracker, Object2DInfo &out);

// Backward chain (:690-838). ring: a camera's kT2dInterval slot ids, oldest
// first (ring[kT2dInterval - 1] = frame t). Begin keeps the detections with
// enough features; per step, Jobs emits one LK call per running chain (frame
// t-step+1 -> t-step) and StepDone takes its outputs (Chain::prev); End fills
// the sets of chains that kept no step and the overlap flags.
void BackwardBegin(const std::vector<Detection> &dets, const std::vector<std::vector<Point2f>> &features,
                   std::vector<DetectedObject> &out, std::vector<Chain> &chains);
void BackwardJobs(int step, const int *ring, double scale, std::vector<Chain> &chains,
                  const std::vector<DetectedObject> &out, std::vector<Job> &jobs);
void BackwardStepDone(std::vector<Chain> &chains, std::vector<DetectedObject> &out, double scale);
void BackwardEnd(std::vector<DetectedObject> &out, const std::vector<std::vector<Point2f>> &features);
// Forward tracking + matching score (:851-1025): Jobs emits one LK call per
// tracker (frame t-1 -> t), Done takes their outputs (trackedPoints, status);
// cost = matchingCostArray [dets x trackers], +inf where not matched.
void ForwardJobs(const int *ring, double scale, const std::vector<Tracker2D *> &trackers,
                 std::vector<std::vector<uint8_t>> &status, std::vector<Job> &jobs);
void ForwardDone(const std::vector<Tracker2D *> &trackers, std::vector<std::vector<uint8_t>> &status,
                 const std::vector<DetectedObject> &dets, std::vector<float> &cost, double scale);

// tracker2d_match.cpp: the assignment of Track2D_MatchingAndUpdating (inf
// handling + minimum-cost matching, :1040-1064) and the update (:1066-1164)
std::vector<int> AssignDetections(const std::vector<float> &cost, size_t rows, size_t cols);
// CPSNWhere_Hungarian::Match (helpers/PSNWhere_Hungarian.cpp:212-359): matched pairs in row-major order
bool HungarianMatch(const std::vector<float> &cost, size_t rows, size_t cols, std::vector<int> &outRows,
                    std::vector<int> &outCols, std::vector<float> &outCosts);
void MatchingAndUpdating(std::vector<DetectedObject> &dets, std::deque<Tracker2D *> &active,
                         std::list<Tracker2D> &storage, const std::vector<int> &match, unsigned frameIdx,
                         unsigned &newTrackerID, Track2DResult &result);

}  // namespace psn
