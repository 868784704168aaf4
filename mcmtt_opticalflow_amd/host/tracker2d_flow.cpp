// Tracker2D flow stage (see tracker2d_flow.hpp). Reference lines cited are in
// psn_where/PSNWhere_Tracker2D.cpp unless noted.
// This file: set-up and tear-down, frame staging, the camera Run and the
// single-camera API; the device pass they drive is in tracker2d_pass.cpp, the
// reference's arithmetic in tracker2d_steps.cpp.
#include "tracker2d_flow.hpp"

#include <algorithm>
#include <chrono>

namespace psn {

int Tracker2DFlow::fail(int rc, const char *what) {
    err_ = std::string(what) + ": " + (lk_ ? psn_lk_last_error(lk_) : "no context") + " (" + std::to_string(rc) + ")";
    return rc;
}

int Tracker2DFlow::Initialize(unsigned camID, int width, int height, int device, double scale) {
    return InitializeCameras(std::vector<unsigned>{camID}, width, height, device, scale);
}

int Tracker2DFlow::InitializeCameras(const std::vector<unsigned> &camIDs, int width, int height, int device,
                                     double scale) {
    return InitializeCameras(camIDs, std::vector<int>(camIDs.size(), width), std::vector<int>(camIDs.size(), height),
                             device, scale);
}

int Tracker2DFlow::InitializeCameras(const std::vector<unsigned> &camIDs, const std::vector<int> &widths,
                                     const std::vector<int> &heights, int device, double scale) {
    Finalize();
    const size_t C = camIDs.size();
    if (C == 0 || widths.size() != C || heights.size() != C) return PSN_LK_ERR_ARG;
    // frame classes: one per distinct size, in order of first appearance
    std::vector<psn_lk_frame_class> cls;
    std::vector<size_t> cam_cls(C), cam_idx(C);  // a camera's class and its place among the class's cameras
    std::vector<Cam> cams(C);
    for (size_t c = 0; c < C; c++) {
        if (widths[c] <= 0 || heights[c] <= 0) return PSN_LK_ERR_ARG;
        if (psn_lk_scaled_size(widths[c], heights[c], scale, &cams[c].lk_w, &cams[c].lk_h)) {
            err_ = "scale outside (0, 1] or a scaled frame below 1 px";
            return PSN_LK_ERR_ARG;
        }
        size_t k = 0;
        while (k < cls.size() && (cls[k].width != widths[c] || cls[k].height != heights[c])) k++;
        if (k == cls.size()) {
            if (k == PSN_LK_MAX_FRAME_CLASSES) {
                err_ = "more than " + std::to_string(PSN_LK_MAX_FRAME_CLASSES) + " distinct frame sizes";
                return PSN_LK_ERR_ARG;
            }
            cls.push_back(psn_lk_frame_class{widths[c], heights[c], 0});
        }
        cam_cls[c] = k;
        cam_idx[c] = (size_t)cls[k].ring_slots / kSlotsPerCam;
        cls[k].ring_slots += kSlotsPerCam;
    }
    scale_ = scale;
    const int nslots = (int)C * kSlotsPerCam;
    // full pyramids of every camera's slots; the reference's default maxLevel 3 needs 4 levels
    // (one size: psn_lk_create_scaled's context, at scale 1.0 psn_lk_create's: no resize launch)
    int rc = psn_lk_create_classes(device, cls.data(), (int)cls.size(), scale, 3, &lk_);
    if (rc) {
        lk_ = nullptr;
        err_ = "psn_lk_create_classes failed (" + std::to_string(rc) + ")";
        return rc;
    }
    cams_.swap(cams);
    for (size_t c = 0; c < C; c++) {
        int first = 0;
        psn_lk_class_slots(lk_, (int)cam_cls[c], &first, nullptr);
        const int base = first + (int)cam_idx[c] * kSlotsPerCam;
        cams_[c].camID = camIDs[c];
        cams_[c].width = widths[c];
        cams_[c].height = heights[c];
        for (int i = 0; i < kT2dInterval; i++) cams_[c].ring[i] = base + i;
        for (int i = 0; i < kT2dStaging; i++) cams_[c].spares[i] = base + kT2dInterval + i;
        cams_[c].nstaged = 0;
    }
    filled_.assign((size_t)nslots, 0);
    slot_frame_.assign((size_t)nslots, -1);
    // a failure from here on leaves the object as Finalize leaves it: no context,
    // no cameras, no half-made set of streams for the next call to run on
    auto undo = [&](const char *what) {
        err_ = what;
        Finalize();
        return PSN_LK_ERR_HIP;
    };
    // stream priorities: the backward chains (three dependent launches per frame)
    // are the frame's critical path; the forward calls fill the compute units they
    // leave free instead of taking half of them (the device dispatches waiting
    // workgroups of higher-priority queues first)
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return undo("forward stream");
    for (Stream &fs : fwd_streams_)
        if (!fs.create(least)) return undo("forward stream");
    for (Stream &cs : chain_streams_)
        if (!cs.create(greatest)) return undo("chain stream");
    Schedule &s = sched_;
    if (!s.chain_done.create() || !s.fwd_done.create()) return undo("result events");
    if (!s.gf.create()) return undo("gridfast event");
    for (int p = 0; p < 2; p++)
        if (!s.fend[p].create() || !s.fcopied[p].create()) return undo("forward block events");
    for (int r = 0; r < kT2dResBlocks; r++)
        if (!s.set0[r].create() || !s.fread[r].create()) return undo("result block events");
    rc = psn_lk_set_stream(lk_, ChainStream(0));
    if (rc) Finalize();
    return rc;
}

// Order matters: the forward streams go first; the LK context next, while the
// chain stream it was last set to still exists; then the chain streams; the
// events, which those streams may still have waited on, last.
void Tracker2DFlow::Finalize() {
    if (dev_) {
        // every stream that may still use the device buffers: the LK context's,
        // both chain streams (a frame launched ahead runs on the other one) and
        // both forward streams
        if (lk_) psn_lk_sync(lk_);
        SyncChains();
        SyncForward();
        dev_.reset();
    }
    for (Stream &fs : fwd_streams_) fs.reset();
    if (lk_) psn_lk_destroy(lk_);
    lk_ = nullptr;
    for (Stream &cs : chain_streams_) cs.reset();
    sched_ = Schedule();  // the events, the result-block cursor, what the last passes left
    cams_.clear();
}

int Tracker2DFlow::PushFrame(const uint8_t *frame, int stride, int channels) {
    if (!lk_) return PSN_LK_ERR_ARG;
    const int slot = cams_[0].ring[kT2dInterval - 1];
    const int rc = psn_lk_push_frame(lk_, slot, frame, stride, channels);
    if (rc) return fail(rc, "psn_lk_push_frame");
    filled_[(size_t)slot] = 1;
    return PSN_LK_OK;
}

int Tracker2DFlow::PushFrameDevice(const uint8_t *dev, int stride, int channels) {
    if (!lk_) return PSN_LK_ERR_ARG;
    const int slot = cams_[0].ring[kT2dInterval - 1];
    const int rc = psn_lk_push_frame_device(lk_, slot, dev, stride, channels);
    if (rc) return fail(rc, "psn_lk_push_frame_device");
    filled_[(size_t)slot] = 1;
    return PSN_LK_OK;
}

// The next free staging slot of a camera (frames are adopted in push order).
int Tracker2DFlow::NextStagingSlot(size_t cam, int *slot) {
    Cam &c = cams_[cam];
    if (c.nstaged >= kT2dStaging) {
        err_ = "camera " + std::to_string(cam) + ": " + std::to_string(kT2dStaging) + " frames staged already";
        return PSN_LK_ERR_ARG;
    }
    *slot = c.spares[c.nstaged];
    return PSN_LK_OK;
}

int Tracker2DFlow::StageFrame(size_t cam, const uint8_t *frame, int stride, int channels, bool on_device) {
    if (!lk_ || cam >= cams_.size() || !frame) return PSN_LK_ERR_ARG;
    Cam &c = cams_[cam];
    int slot = -1, rc = NextStagingSlot(cam, &slot);
    if (rc) return rc;
    rc = on_device ? psn_lk_push_frame_device(lk_, slot, frame, stride, channels)
                   : psn_lk_push_frame_async(lk_, slot, frame, stride, channels);
    if (rc) return fail(rc, "stage frame");
    filled_[(size_t)slot] = 1;
    c.nstaged++;
    return PSN_LK_OK;
}

int Tracker2DFlow::StageFrameJpeg(size_t cam, const uint8_t *jpeg, size_t len) {
    if (!lk_ || cam >= cams_.size() || !jpeg) return PSN_LK_ERR_ARG;
    Cam &c = cams_[cam];
    int slot = -1, rc = NextStagingSlot(cam, &slot);
    if (rc) return rc;
    rc = psn_lk_push_frame_jpeg(lk_, slot, jpeg, len);
    if (rc) return fail(rc, "stage JPEG frame");
    filled_[(size_t)slot] = 1;
    c.nstaged++;
    return PSN_LK_OK;
}

int Tracker2DFlow::StageFramesJpeg(const uint8_t *const *jpeg, const size_t *len) {
    if (!lk_ || !jpeg || !len) return PSN_LK_ERR_ARG;
    std::vector<int> slots(cams_.size());
    for (size_t cam = 0; cam < cams_.size(); cam++) {
        const int rc = NextStagingSlot(cam, &slots[cam]);
        if (rc) return rc;
    }
    const int rc = psn_lk_push_frames_jpeg(lk_, slots.data(), jpeg, len, (int)slots.size());
    if (rc) return fail(rc, "stage JPEG frames");
    for (size_t cam = 0; cam < cams_.size(); cam++) {  // committed only now: the whole push succeeded
        filled_[(size_t)slots[cam]] = 1;
        cams_[cam].nstaged++;
    }
    return PSN_LK_OK;
}

int Tracker2DFlow::DetectFeatures(const std::vector<Detection> &dets, uint32_t seed,
                                  std::vector<std::vector<Point2f>> &features) {
    if (!lk_) return PSN_LK_ERR_ARG;
    const size_t n = dets.size();
    features.assign(n, {});
    if (n == 0) return PSN_LK_OK;
    std::vector<int> rois(4 * n), cnt(n), tot(n);
    for (size_t i = 0; i < n; i++) Roi(0, dets[i].box, &rois[4 * i]);
    psn_gridfast_params p;
    psn_gridfast_default_params(&p);
    p.cap = (int)kT2dMaxFeatures;
    gf_xy_.resize(2 * n * kT2dMaxFeatures);
    const int rc = psn_gridfast_detect(lk_, cams_[0].ring[kT2dInterval - 1], rois.data(), (int)n, &p, seed,
                                       gf_xy_.data(), cnt.data(), tot.data());
    if (rc) return fail(rc, "psn_gridfast_detect");
    for (size_t i = 0; i < n; i++) {
        const float *xy = gf_xy_.data() + 2 * kT2dMaxFeatures * i;
        features[i].resize((size_t)cnt[i]);
        for (int k = 0; k < cnt[i]; k++) features[i][(size_t)k] = Point2f{xy[2 * k], xy[2 * k + 1]};
    }
    return PSN_LK_OK;
}

void Tracker2DFlow::RotateRing() { std::rotate(cams_[0].ring, cams_[0].ring + 1, cams_[0].ring + kT2dInterval); }

// steps s = 1..3 need frame t-s: consecutive filled slots behind the newest
int Tracker2DFlow::StepsAvailable(size_t cam) const {
    int s = 0;
    while (s + 1 < kT2dInterval && filled_[(size_t)cams_[cam].ring[kT2dInterval - 2 - s]]) s++;
    return s;
}

// One launch for all jobs: points concatenated, one query per job. err is
// requested as the reference does (:781, :876): its bounds re-check can clear
// status. The err values are never read (Query sets PSN_LK_ERR_STATUS_ONLY:
// err_out_ is what the re-check needs to run, its contents are unspecified).
int Tracker2DFlow::RunJobs(std::vector<Job> &jobs) {
    size_t n = 0;
    queries_.clear();
    for (const Job &j : jobs) {
        psn_lk_query q = Query(j.prev_slot, j.next_slot, n, j.in->size());
        q.params.win_w = j.win_w;
        q.params.win_h = j.win_h;
        queries_.push_back(q);
        n += j.in->size();
    }
    if (queries_.empty()) return PSN_LK_OK;
    xy_in_.resize(2 * n);
    xy_out_.resize(2 * n);
    err_out_.resize(n);
    st_out_.resize(n);
    size_t o = 0;
    for (const Job &j : jobs)
        for (const Point2f &p : *j.in) {
            xy_in_[2 * o] = p.x;
            xy_in_[2 * o + 1] = p.y;
            o++;
        }
    const int rc = psn_lk_track(lk_, queries_.data(), (int)queries_.size(), xy_in_.data(), xy_out_.data(),
                                st_out_.data(), err_out_.data());
    if (rc) return fail(rc, "psn_lk_track");
    o = 0;
    for (Job &j : jobs) {
        const size_t m = j.in->size();
        j.out->resize(m);
        j.status->resize(m);
        for (size_t i = 0; i < m; i++, o++) {
            (*j.out)[i] = Point2f{xy_out_[2 * o], xy_out_[2 * o + 1]};
            (*j.status)[i] = st_out_[o];
        }
    }
    return PSN_LK_OK;
}

int Tracker2DFlow::BackwardFeatureTracking(const std::vector<Detection> &dets,
                                           const std::vector<std::vector<Point2f>> &features,
                                           std::vector<DetectedObject> &out) {
    if (!lk_ || features.size() != dets.size()) return PSN_LK_ERR_ARG;
    if (device_chain_) {
        std::vector<std::vector<Point2f>> f = features;
        const int rc = DevicePass(dets, f, out, nullptr, false, 0);
        if (rc) return rc;
        BackwardEnd(out, features);
        return PSN_LK_OK;
    }
    std::vector<Chain> chains;
    BackwardBegin(dets, features, out, chains);
    std::vector<Job> jobs;
    for (int step = 1; StepAvailable(step); step++) {
        jobs.clear();
        BackwardJobs(step, cams_[0].ring, scale_, chains, out, jobs);
        if (jobs.empty()) break;
        int rc = RunJobs(jobs);
        if (rc) return rc;
        BackwardStepDone(chains, out, scale_);
    }
    BackwardEnd(out, features);
    return PSN_LK_OK;
}

int Tracker2DFlow::ForwardTrackingAndGetMatchingScore(const std::vector<Tracker2D *> &trackers,
                                                      const std::vector<DetectedObject> &dets,
                                                      std::vector<float> &cost) {
    if (!lk_) return PSN_LK_ERR_ARG;
    std::vector<std::vector<uint8_t>> status;
    std::vector<Job> jobs;
    if (!trackers.empty() && !StepAvailable(1)) return PSN_LK_ERR_SLOT;  // no frame t-1
    ForwardJobs(cams_[0].ring, scale_, trackers, status, jobs);
    int rc = RunJobs(jobs);
    if (rc) return rc;
    ForwardDone(trackers, status, dets, cost, scale_);
    return PSN_LK_OK;
}

// GridFAST + backward chains + forward in one device pass (device chain mode):
// the forward launch goes first on its own stream; GridFAST writes every
// detection's features straight into the chain inputs (the host never sees
// them before the chains run); counts below the minimum are gated to 0 on the
// device; one sync at the end. Results are those of DetectFeatures +
// TrackFrame.
int Tracker2DFlow::TrackFrameDetect(const std::vector<Detection> &dets, uint32_t seed,
                                    std::vector<std::vector<Point2f>> &features, std::vector<DetectedObject> &out,
                                    const std::vector<Tracker2D *> &trackers, std::vector<float> &cost) {
    if (!lk_) return PSN_LK_ERR_ARG;
    if (!device_chain_) {
        const int rc = DetectFeatures(dets, seed, features);
        return rc ? rc : TrackFrame(dets, features, out, trackers, cost);
    }
    if (!trackers.empty() && !StepAvailable(1)) return PSN_LK_ERR_SLOT;
    std::vector<std::vector<uint8_t>> fstatus;
    std::vector<Job> fwd;
    ForwardJobs(cams_[0].ring, scale_, trackers, fstatus, fwd);
    const int rc = DevicePass(dets, features, out, &fwd, true, seed);
    if (rc) return rc;
    BackwardEnd(out, features);
    ForwardDone(trackers, fstatus, out, cost, scale_);
    return PSN_LK_OK;
}

int Tracker2DFlow::TrackFrame(const std::vector<Detection> &dets, const std::vector<std::vector<Point2f>> &features,
                              std::vector<DetectedObject> &out, const std::vector<Tracker2D *> &trackers,
                              std::vector<float> &cost) {
    if (!lk_ || features.size() != dets.size()) return PSN_LK_ERR_ARG;
    if (!trackers.empty() && !StepAvailable(1)) return PSN_LK_ERR_SLOT;
    std::vector<std::vector<uint8_t>> fstatus;
    std::vector<Job> jobs;
    if (device_chain_) {
        ForwardJobs(cams_[0].ring, scale_, trackers, fstatus, jobs);
        std::vector<std::vector<Point2f>> f = features;
        const int rc = DevicePass(dets, f, out, &jobs, false, 0);
        if (rc) return rc;
        BackwardEnd(out, features);
        ForwardDone(trackers, fstatus, out, cost, scale_);
        return PSN_LK_OK;
    }
    std::vector<Chain> chains;
    BackwardBegin(dets, features, out, chains);
    // launch 1: backward step 1 of every detection + every forward call
    if (StepAvailable(1)) BackwardJobs(1, cams_[0].ring, scale_, chains, out, jobs);
    const size_t nb = jobs.size();
    ForwardJobs(cams_[0].ring, scale_, trackers, fstatus, jobs);
    int rc = RunJobs(jobs);
    if (rc) return rc;
    if (nb) BackwardStepDone(chains, out, scale_);
    for (int step = 2; nb && StepAvailable(step); step++) {
        jobs.clear();
        BackwardJobs(step, cams_[0].ring, scale_, chains, out, jobs);
        if (jobs.empty()) break;
        rc = RunJobs(jobs);
        if (rc) return rc;
        BackwardStepDone(chains, out, scale_);
    }
    BackwardEnd(out, features);
    ForwardDone(trackers, fstatus, out, cost, scale_);
    return PSN_LK_OK;
}

// ---------------------------------------------------------------------------
// CPSNWhere_Tracker2D::Run of every camera (:251-373), batched
// ---------------------------------------------------------------------------

// Adopt every camera's staged frame as frame t (the ring advances: the oldest
// slot becomes the next staging slot; Run's buffer circulation, :310-316) and
// set up the pass over io (forward calls not yet attached).
int Tracker2DFlow::AdoptFrames(std::vector<CamFrame> &io, bool gridfast, std::vector<PassCam> &pass,
                               unsigned frameIdx) {
    if (io.size() != cams_.size()) return PSN_LK_ERR_ARG;
    for (size_t c = 0; c < cams_.size(); c++) {
        if (cams_[c].nstaged == 0) {
            err_ = "camera " + std::to_string(c) + ": no frame staged";
            return PSN_LK_ERR_SLOT;
        }
        if (!gridfast && io[c].features.size() != io[c].dets.size()) return PSN_LK_ERR_ARG;
    }
    pass.assign(cams_.size(), PassCam());
    for (size_t c = 0; c < cams_.size(); c++) {
        Cam &cam = cams_[c];
        // the first staged frame joins the ring as frame t; the oldest ring slot
        // becomes the last staging slot (a later push into it waits for its readers)
        const int oldest = cam.ring[0];
        std::rotate(cam.ring, cam.ring + 1, cam.ring + kT2dInterval);
        cam.ring[kT2dInterval - 1] = cam.spares[0];
        std::rotate(cam.spares, cam.spares + 1, cam.spares + kT2dStaging);
        cam.spares[kT2dStaging - 1] = oldest;
        cam.nstaged--;
        slot_frame_[(size_t)cam.ring[kT2dInterval - 1]] = (long long)frameIdx;
        PassCam &p = pass[c];
        p.cam = c;
        p.dets = &io[c].dets;
        p.features = &io[c].features;
        p.out = &io[c].objects;
        p.fwd = nullptr;
        io[c].objects.clear();
    }
    return PSN_LK_OK;
}

int Tracker2DFlow::SlotOfFrame(size_t cam, unsigned frameIdx, int *slot) {
    if (cam >= cams_.size() || !slot) return PSN_LK_ERR_ARG;
    for (int i = kT2dInterval - 1; i >= 0; i--) {
        const int s = cams_[cam].ring[i];
        if (filled_[(size_t)s] && slot_frame_[(size_t)s] == (long long)frameIdx) {
            *slot = s;
            return PSN_LK_OK;
        }
    }
    err_ = "camera " + std::to_string(cam) + ": frame " + std::to_string(frameIdx) + " is not in the ring";
    return PSN_LK_ERR_SLOT;
}

void Tracker2DFlow::UnadoptFrames() {
    for (Cam &cam : cams_) {
        const int newest = cam.ring[kT2dInterval - 1];
        std::rotate(cam.ring, cam.ring + kT2dInterval - 1, cam.ring + kT2dInterval);
        cam.ring[0] = cam.spares[kT2dStaging - 1];
        std::rotate(cam.spares, cam.spares + kT2dStaging - 1, cam.spares + kT2dStaging);
        cam.spares[0] = newest;
        cam.nstaged++;
    }
}

// Enqueue frame t's device work for every camera: one pass over all cameras
// (features, backward chains, forward calls of every active tracker). When
// RunComplete(t-1, next = frame t) has launched frame t already, this only
// confirms it.
int Tracker2DFlow::RunLaunch(unsigned frameIdx, std::vector<CamFrame> &io, bool gridfast, uint32_t seed) {
    if (!lk_ || io.size() != cams_.size()) return PSN_LK_ERR_ARG;
    if (launched_ahead_) {
        if (&io != pre_io_ || frameIdx != run_frame_ || gridfast != run_gridfast_) {
            err_ = "RunLaunch: frame " + std::to_string(frameIdx) + " is not the frame launched ahead (" +
                   std::to_string(run_frame_) + ")";
            return PSN_LK_ERR_ARG;
        }
        launched_ahead_ = false;
        pre_io_ = nullptr;
        return PSN_LK_OK;
    }
    int rc = AdoptFrames(io, gridfast, run_pass_, frameIdx);
    if (rc) return rc;
    run_frame_ = frameIdx;
    run_gridfast_ = gridfast;
    // frame t's forward calls from frame t-1's chain pass (when it left trackers),
    // then frame t's features and chains
    bool any = false;
    for (const Cam &cam : cams_) any = any || !cam.active.empty();
    const Cursor saved = sched_.cur;
    rc = any ? LaunchForwardFromChains(run_pass_, sched_.trk_rb, true) : PSN_LK_OK;
    if (!rc) rc = PassLaunchChains(run_pass_, gridfast, seed);
    if (rc) {  // nothing of the frame stays in flight; the result blocks as before
        SyncChains();
        SyncForward();
        run_pass_.clear();
        sched_.cur = saved;
    }
    return rc;
}


// Wait for the frame's device work, then per camera: overlap flags (:824-835),
// matching costs + majority gate (:906-1022), assignment and tracker update
// (:1038-1164), result packaging (:1099-1101, :1144-1146).
int Tracker2DFlow::RunComplete(std::vector<CamFrame> &io) { return RunComplete(io, nullptr, 0, false, 0); }

// With next: frame t+1 is launched from here. Its features and backward chains
// (its frames staged) are enqueued as soon as frame t's device work is done,
// before the host part of frame t, so the GPU runs them while the host matches
// frame t; its forward calls follow frame t's tracker update. Frame t+1's
// chains read only its detections and the ring, never frame t's trackers, so
// the results are those of RunLaunch(t+1) after RunComplete(t).
int Tracker2DFlow::RunComplete(std::vector<CamFrame> &io, std::vector<CamFrame> *next, unsigned nextFrameIdx,
                               bool nextGridfast, uint32_t nextSeed) {
    if (!lk_ || io.size() != cams_.size() || run_pass_.size() != cams_.size() || launched_ahead_ || &io == next)
        return PSN_LK_ERR_ARG;
    // The next frame's chains are enqueued right behind this frame's result copies
    // (stream order keeps them from overwriting what is copied; their inputs go
    // through the other staging set), then this frame is waited for and
    // unpacked while they run. If they need larger chain buffers, the regrow
    // waits, so this frame is unpacked first.
    using clk = std::chrono::steady_clock;
    const clk::time_point t0 = clk::now();
    auto stamp = [&](int i) { host_us_[i] += std::chrono::duration<double, std::micro>(clk::now() - t0).count(); };
    frame_completed_ = false;
    const int cur_rb = run_pass_.empty() ? -1 : run_pass_[0].rb;
    std::vector<size_t> cur_k0(cams_.size(), 0);
    for (const PassCam &p : run_pass_) cur_k0[p.cam] = p.k0;
    int rc = PassCopy(run_pass_);
    const bool early = !rc && next && ChainsFit(*next);
    int prc = PSN_LK_OK;
    std::vector<PassCam> pre;
    const Cursor saved = sched_.cur;
    // a next frame that cannot be launched leaves no trace: its work drained, its
    // frames staged again (the rings as before), frame t still completed
    auto abandon_next = [&]() {
        SyncChains();
        SyncForward();
        UnadoptFrames();
        sched_.cur.next_rb = saved.next_rb;  // the staging set stays flipped: the sets are interchangeable
        sched_.cur.last_rb = saved.last_rb;
        pre.clear();
    };
    // frame t+1: its forward calls straight from frame t's chains (every detection
    // of frame t becomes a tracker), then its features and chains
    auto prelaunch = [&]() {
        prc = AdoptFrames(*next, nextGridfast, pre, nextFrameIdx);
        if (prc) {
            pre.clear();
            return;
        }
        prc = LaunchForwardFromChains(pre, cur_rb, false);
        if (!prc) prc = PassLaunchChains(pre, nextGridfast, nextSeed);
        if (prc) abandon_next();
    };
    if (early) prelaunch();
    stamp(0);  // copies + next frame's forward + chains enqueued
    if (!rc) rc = PassSync();
    stamp(1);  // device work done
    if (!rc) rc = PassFeatures(run_pass_, run_gridfast_);
    if (rc) {
        run_pass_.clear();
        if (next && early && !prc) abandon_next();  // frame t failed: nothing of t+1 stays in flight
        return rc;
    }
    PassUnpack(run_pass_);
    run_pass_.clear();
    if (next && !early) prelaunch();
    stamp(2);  // unpacked
    // a tracker whose box window the forward LK cannot run (CV_Assert in the
    // reference) fails the frame before any camera is updated
    for (size_t c = 0; c < cams_.size(); c++)
        for (const Tracker2D *tr : cams_[c].trackers) {
            const Rect b = tr->boxes.back().scale(scale_);
            const int we = WindowError((int)(b.w * kWinSizeRatio), (int)(b.h * kWinSizeRatio));
            if (we) {
                err_ = "camera " + std::to_string(c) + ": tracker " + std::to_string(tr->id) + " forward window";
                if (next && !prc && !pre.empty()) abandon_next();
                return we;
            }
        }
    for (size_t c = 0; c < cams_.size(); c++) {
        Cam &cam = cams_[c];
        CamFrame &f = io[c];
        clk::time_point p = clk::now();
        auto part = [&](int i) {
            const clk::time_point q = clk::now();
            host_us_[5 + i] += std::chrono::duration<double, std::micro>(q - p).count();
            p = q;
        };
        BackwardEnd(f.objects, f.features);
        part(0);
        ForwardDone(cam.trackers, cam.fstatus, f.objects, f.cost, scale_);
        part(1);
        const std::vector<int> match = AssignDetections(f.cost, f.objects.size(), cam.trackers.size());
        part(2);
        MatchingAndUpdating(f.objects, cam.active, cam.storage, match, run_frame_, cam.newTrackerID, f.result);
        part(3);
        f.result.camID = cam.camID;
        // the next frame's forward calls (launched from this frame's chains): these trackers
        cam.trackers.assign(cam.active.begin(), cam.active.end());
        cam.fwd_k0 = cur_k0[c];
    }
    sched_.trk_rb = cur_rb;  // the trackers' set 0
    stamp(3);  // matched, trackers updated
    host_calls_++;
    frame_completed_ = true;
    if (!next || prc) return prc;
    stamp(4);
    run_pass_ = std::move(pre);
    run_frame_ = nextFrameIdx;
    run_gridfast_ = nextGridfast;
    pre_io_ = next;
    launched_ahead_ = true;
    return PSN_LK_OK;
}

}  // namespace psn
