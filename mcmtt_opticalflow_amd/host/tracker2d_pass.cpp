// Tracker2DFlow's device pass (see tracker2d_flow.hpp): buffers, launches on the
// chain and forward streams, result copies, completion poll and unpacking.
// Reference lines cited are in psn_where/PSNWhere_Tracker2D.cpp.
#include <sched.h>

#include <algorithm>
#include <cstring>

#include "tracker2d_flow.hpp"

namespace psn {

void Tracker2DFlow::SyncChains() {
    for (const Stream &cs : chain_streams_) cs.sync();
}

void Tracker2DFlow::SyncForward() {
    for (const Stream &fs : fwd_streams_) fs.sync();
}

void Tracker2DFlow::Chk(hipError_t e, const char *what, int &rc) {
    if (e != hipSuccess && !rc) {
        err_ = std::string(what) + ": " + hipGetErrorString(e);
        rc = PSN_LK_ERR_HIP;
    }
}

// A calcOpticalFlowPyrLK call with the reference's defaults -- maxLevel 3,
// (COUNT|EPS, 30, 0.01), minEig 1e-4 -- and the default window, which every
// caller with points to track replaces (:782, :877). Every Tracker2D launch is
// built from this query (chain steps, forward, RunJobs, LaunchForwardFromChains)
// and passes an err array, as the reference does (:781, :876), for the level-0
// bounds re-check that err brings with it; the reference only clears and passes
// featureErrors / pointError and nothing here reads an err value, so the queries
// ask for the re-check alone (PSN_LK_ERR_STATUS_ONLY).
psn_lk_query Tracker2DFlow::Query(int prev_slot, int next_slot, size_t first_pt, size_t num_pts) {
    psn_lk_query q;
    q.prev_slot = prev_slot;
    q.next_slot = next_slot;
    q.first_pt = (int)first_pt;
    q.num_pts = (int)num_pts;
    psn_lk_default_params(&q.params);
    q.params.flags |= PSN_LK_ERR_STATUS_ONLY;
    return q;
}

// cv::Rect((int)x, (int)y, (int)w, (int)h) of the cropped, scaled box (:736)
void Tracker2DFlow::Roi(size_t cam, const Rect &box, int *roi) const {
    const Rect r = box.scale(scale_).cropWithSize(cams_[cam].lk_w, cams_[cam].lk_h);
    roi[0] = (int)r.x;
    roi[1] = (int)r.y;
    roi[2] = (int)r.w;
    roi[3] = (int)r.h;
}

// Error of a w x h window the LK cannot run: CV_Assert(winSize > 2) in the
// reference, or outside the LK's window limits (psn_lk_window_supported: the
// same predicate psn_lk_track applies). A chain's window is the square of its
// box width (:782), a forward call's its box (:877).
int Tracker2DFlow::WindowError(int w, int h) {
    if (w <= 2 || h <= 2) return PSN_LK_ERR_WINSIZE;
    if (!psn_lk_window_supported(w, h)) return PSN_LK_ERR_UNSUPPORTED;
    return PSN_LK_OK;
}

// An LK launch on forward stream `par` (output block par): the context's stream
// is put back whatever happens; on success block par is the current one and
// `recorded` is the result of recording its end event.
template <class Launch>
int Tracker2DFlow::OnForwardStream(int par, Launch launch, hipError_t &recorded) {
    hipStream_t st = LkStream(), fs = FwdStream(par);
    int rc = psn_lk_set_stream(lk_, fs);
    if (!rc) rc = launch();
    const int rs = psn_lk_set_stream(lk_, st);
    if (rc || rs) return fail(rc ? rc : rs, "forward launch");
    sched_.fwd_par = par;
    recorded = sched_.fend[par].record(fs);
    return PSN_LK_OK;
}

// Chain buffers for nchains detections: grown only between passes (no chain in
// flight on the chain stream).
int Tracker2DFlow::EnsureChains(size_t nchains) {
    if (!dev_) dev_.reset(new DeviceBuffers());
    DeviceBuffers &b = *dev_;
    if (b.nchains >= nchains && b.sc[0].d_in) return PSN_LK_OK;
    if (lk_) psn_lk_sync(lk_);
    SyncChains();
    // a forward launch may still read a result block's set 0
    SyncForward();
    b.release_chains();
    for (int r = 0; r < kT2dResBlocks; r++) {
        sched_.chain_info[r].valid = false;
        sched_.fread[r].forget();
    }
    const size_t K = grow_cap(nchains, 16);
    const size_t cap = PSN_T2D_CHAIN_CAP, S = PSN_T2D_CHAIN_STEPS, npt = K * cap;
    Allocations &m = b.chain_mem;
    b.layout_in(K, cap);
    for (DeviceBuffers::Scratch &x : b.sc) {
        m.device(x.d_inblk, b.in_bytes);
        m.device(x.d_out, npt * 8);
        m.device(x.d_buf[0], npt * 8);
        m.device(x.d_buf[1], npt * 8);
        m.device(x.d_err, npt * 4);
        m.device(x.d_status, npt);
        m.device(x.d_tot, K * 4);
    }
    b.res_sets_off = DeviceBuffers::res_box_off(K, S) + K * S * 4 * 8;
    const size_t res_bytes = b.res_sets_off + K * S * cap * 8;
    for (char *&d : b.d_res) m.device(d, res_bytes);
    for (char *&h : b.h_res) m.pinned(h, res_bytes);
    for (DeviceBuffers::Stage &g : b.stage) {
        m.pinned(g.h_inblk, b.in_bytes);
        m.pinned(g.h_rawcnt, K * 4);
    }
    if (!m.ok) {
        b.release_chains();
        err_ = "chain buffers: allocation failed";
        return PSN_LK_ERR_NOMEM;
    }
    for (DeviceBuffers::Scratch &x : b.sc) b.carve_in(x.d_inblk, x.d_boxes, x.d_last, x.d_cnt, x.d_in);
    for (DeviceBuffers::Stage &g : b.stage) b.carve_in(g.h_inblk, g.h_boxes, g.h_last, g.h_cnt, g.h_in);
    b.nchains = K;
    return PSN_LK_OK;
}

// Forward buffers for nfwd_pts points in nfwd_jobs calls: the forward stream is
// the only device user, so growing them never waits for a chain in flight.
int Tracker2DFlow::EnsureForward(size_t nfwd_pts, size_t nfwd_jobs) {
    if (!dev_) dev_.reset(new DeviceBuffers());
    DeviceBuffers &b = *dev_;
    if (b.nfwd_pts >= nfwd_pts && b.nfwd_jobs >= nfwd_jobs && b.d_fin) return PSN_LK_OK;
    SyncForward();
    SyncChains();  // result copies of the forward blocks run on the chain streams
    // results of a pass not unpacked yet (its copy was enqueued) move to the new buffers
    std::vector<uint8_t> keep_st;
    std::vector<float> keep_pts;
    if (b.h_foblk) {
        keep_st.assign(b.h_fwd_st, b.h_fwd_st + b.nfwd_pts);
        keep_pts.assign(b.h_fwd_out, b.h_fwd_out + 2 * b.nfwd_pts);
    }
    b.release_forward();
    const size_t F = grow_cap(nfwd_pts, 1024), J = grow_cap(nfwd_jobs, 16);
    Allocations &m = b.fwd_mem;
    b.fi_off_pts = (J * 4 + 255) & ~(size_t)255;
    b.fo_off_pts = (F + 255) & ~(size_t)255;
    m.device(b.d_fiblk, b.fi_off_pts + F * 8);
    m.device(b.d_foblk[0], b.fo_off_pts + F * 8);
    m.device(b.d_foblk[1], b.fo_off_pts + F * 8);
    m.device(b.d_ferr[0], F * 4);
    m.device(b.d_ferr[1], F * 4);
    m.pinned(b.h_fiblk, b.fi_off_pts + F * 8);
    m.pinned(b.h_foblk, b.fo_off_pts + F * 8);
    if (!m.ok) {
        b.release_forward();
        err_ = "forward buffers: allocation failed";
        return PSN_LK_ERR_NOMEM;
    }
    b.d_fcnt = (int *)b.d_fiblk;
    b.d_fin = (float *)(b.d_fiblk + b.fi_off_pts);
    b.h_fcnt = (int *)b.h_fiblk;
    b.h_fin = (float *)(b.h_fiblk + b.fi_off_pts);
    for (int p = 0; p < 2; p++) {
        b.d_fstatus[p] = (uint8_t *)b.d_foblk[p];
        b.d_fout[p] = (float *)(b.d_foblk[p] + b.fo_off_pts);
    }
    b.h_fwd_st = (uint8_t *)b.h_foblk;
    b.h_fwd_out = (float *)(b.h_foblk + b.fo_off_pts);
    if (!keep_st.empty()) {
        std::memcpy(b.h_fwd_st, keep_st.data(), keep_st.size());
        std::memcpy(b.h_fwd_out, keep_pts.data(), keep_pts.size() * sizeof(float));
    }
    b.nfwd_pts = F;
    b.nfwd_jobs = J;
    return PSN_LK_OK;
}

// Enqueue one device pass over the cameras in pc (everything asynchronous, one
// host sync in PassComplete):
//   1. each detection's features at t: given (host points) or GridFAST on the
//      device straight into the chain inputs (:734-757), detections below the
//      feature minimum (:744) gated to count 0 on the device;
//   2. the backward chains (:763-811): per step ONE counted LK launch over every
//      detection of every camera (capacity PSN_T2D_CHAIN_CAP points each; a
//      stopped chain's count is 0, its workgroups exit at once) and one
//      LocalSearchKLT + inlier-compaction kernel writing the next step's points
//      and counts. A camera whose ring holds fewer past frames ends its chains
//      earlier (per-chain last step); its queries in later steps are empty.
//      The chain stream has the highest priority: its launches are the frame's
//      critical path;
//   3. the forward calls of every camera's trackers (:871-877): one counted LK
//      launch on the (lowest-priority) forward stream, enqueued after the chain
//      so that the chain's first kernels are dispatched before it.
// The device-to-host copies of the results are enqueued by PassComplete: a copy
// waiting for the pass would hold up, on the copy engine, the uploads of the
// next frames (StageFrame) that the caller enqueues in between.
int Tracker2DFlow::PassLaunch(std::vector<PassCam> &pc, bool gridfast, uint32_t seed) {
    const int rc = PassLaunchChains(pc, gridfast, seed);
    return rc ? rc : PassLaunchForward(pc);
}

// 1-2 of the pass: features and the backward chains, on the chain stream.
int Tracker2DFlow::PassLaunchChains(std::vector<PassCam> &pc, bool gridfast, uint32_t seed) {
    const size_t cap = PSN_T2D_CHAIN_CAP;
    size_t K = 0;
    for (PassCam &p : pc) {
        p.k0 = K;
        K += p.dets->size();
    }
    Cursor &cur = sched_.cur;
    const int si = cur.stage;  // this pass's staging set
    cur.stage ^= 1;
    // this pass's result block: neither the previous pass's (in flight) nor the
    // one the current trackers' set 0 lives in (their next forward call reads it
    // when a frame fails)
    int rb = cur.next_rb;
    while (rb == cur.last_rb || rb == sched_.trk_rb) rb = (rb + 1) % kT2dResBlocks;
    cur.next_rb = (rb + 1) % kT2dResBlocks;
    cur.last_rb = rb;
    for (PassCam &p : pc) {
        p.set = si;
        p.rb = rb;
    }
    std::vector<char> &win_bad_ = win_bad_sets_[si];
    win_bad_.assign(K, 0);
    // what the next frame's forward launch reads of this pass: per detection the
    // forward window of its box (the tracker it becomes keeps the box, :1087)
    ChainInfo &ci = sched_.chain_info[rb];
    ci.K = K;
    ci.valid = false;
    ci.k0.assign(cams_.size(), 0);
    ci.ndet.assign(cams_.size(), 0);
    ci.win.assign(K, {0, 0});
    for (PassCam &p : pc) {
        ci.k0[p.cam] = p.k0;
        ci.ndet[p.cam] = p.dets->size();
        for (size_t i = 0; i < p.dets->size(); i++) {
            const Rect box = (*p.dets)[i].box.scale(scale_);
            ci.win[p.k0 + i] = {(int)(box.w * kWinSizeRatio), (int)(box.h * kWinSizeRatio)};
        }
    }
    if (K == 0) {
        ci.valid = true;
        return PSN_LK_OK;
    }
    int rc = EnsureChains(K);
    if (rc) return rc;
    DeviceBuffers::Stage &b = dev_->stage[si];
    DeviceBuffers &dall = *dev_;
    DeviceBuffers::Scratch &db = dall.sc[si];
    // the pass's chain stream (consecutive passes alternate: frame t+1's chains run
    // beside frame t's tail); every LK launch of the pass goes to it
    hipStream_t st = ChainStream(si);
    rc = psn_lk_set_stream(lk_, st);
    if (rc) return fail(rc, "chain stream");
    int max_steps = 0;
    for (PassCam &p : pc) {
        const int steps = StepsAvailable(p.cam);
        for (size_t i = 0; i < p.dets->size(); i++) {
            const size_t k = p.k0 + i;
            const Rect box = (*p.dets)[i].box.scale(scale_);
            b.h_boxes[4 * k] = box.x;
            b.h_boxes[4 * k + 1] = box.y;
            b.h_boxes[4 * k + 2] = box.w;
            b.h_boxes[4 * k + 3] = box.h;
            const int win = (int)(box.w * kWinSizeRatio);
            win_bad_[k] = WindowError(win, win) != 0;
            b.h_last[k] = win_bad_[k] ? 0 : steps;
            if (!win_bad_[k]) max_steps = std::max(max_steps, steps);
        }
    }
    if (gridfast) {
        psn_gridfast_params gp;
        psn_gridfast_default_params(&gp);
        gp.cap = (int)cap;  // kT2dMaxFeatures
        std::vector<int> rois(4 * K), slots, nrois;
        // the detector's cell scratch lives in the LK context: the previous
        // pass's detections (on the other chain stream) are done with it first
        if (sched_.gf.recorded()) Chk(sched_.gf.wait_on(st), "gridfast scratch", rc);
        // every camera's detections in one detector launch (per camera in the
        // reference: sets of rois at consecutive k, outputs at p.k0)
        for (PassCam &p : pc) {
            const size_t n = p.dets->size();
            if (!n) continue;
            slots.push_back(cams_[p.cam].ring[kT2dInterval - 1]);
            nrois.push_back((int)n);
            for (size_t i = 0; i < n; i++) Roi(p.cam, (*p.dets)[i].box, &rois[4 * (p.k0 + i)]);
        }
        rc = psn_gridfast_detect_device_sets(lk_, (int)slots.size(), slots.data(), nrois.data(), rois.data(), &gp,
                                             seed, db.d_in, db.d_cnt, db.d_tot);
        if (rc) return fail(rc, "psn_gridfast_detect_device_sets");
        Chk(sched_.gf.record(st), "gridfast event", rc);
        if (!rc && ((rc = psn_t2d_download_device(b.h_rawcnt, db.d_cnt, K * 4, st)) ||
                    (rc = psn_t2d_download_device(b.h_in, db.d_in, K * cap * 8, st))))
            err_ = "features download";
        // boxes and last steps (GridFAST wrote the counts and points on the device)
        if (!rc && (rc = psn_t2d_upload_device(db.d_inblk, b.h_inblk, dall.in_off_cnt, st)))
            err_ = "chain boxes upload";
    } else {
        for (PassCam &p : pc)
            for (size_t i = 0; i < p.dets->size(); i++) {
                const size_t k = p.k0 + i;
                const std::vector<Point2f> &f = (*p.features)[i];
                const size_t n = std::min(f.size(), kT2dMaxFeatures);  // :753-757
                if (f.size() >= kT2dMinFeatures && win_bad_[k]) {
                    err_ = "detection " + std::to_string(i) + " window";
                    const int win = (int)(b.h_boxes[4 * k + 2] * kWinSizeRatio);
                    return WindowError(win, win);
                }
                for (size_t j = 0; j < n; j++) {
                    b.h_in[2 * (k * cap + j)] = f[j].x;
                    b.h_in[2 * (k * cap + j) + 1] = f[j].y;
                }
                b.h_cnt[k] = (int)n;
            }
        // boxes, last steps, counts and points in one copy (whole rows: a chain
        // row's unused tail is never read)
        // (a kernel reads the pinned block: psn_t2d_upload_device)
        if (!rc && (rc = psn_t2d_upload_device(db.d_inblk, b.h_inblk, dall.in_off_in + K * cap * 8, st)))
            err_ = "chain inputs upload";
    }
    if (rc) return rc;
    // the result block's last reader (a forward launch three frames back) first
    if (sched_.fread[rb].recorded()) Chk(sched_.fread[rb].wait_on(st), "result block reuse", rc);
    const DeviceBuffers::ResView rv = dall.view(dall.d_res[rb]);
    psn_t2d_chain_dev cd{};
    cd.ndet = (int)K;
    cd.cap = (int)cap;
    cd.boxes = db.d_boxes;
    cd.cnt = db.d_cnt;
    cd.cur = db.d_in;
    cd.out_boxes = rv.obox;
    cd.sets = rv.sets;
    cd.set_cnt = rv.setcnt;
    cd.nsteps = rv.nsteps;
    cd.last_step = db.d_last;
    cd.scale = scale_;
    // cleared counters, set 0 = the features at t, the feature-minimum gate: one launch
    if (!rc) rc = psn_t2d_chain_begin_device(&cd, (int)kT2dMinFeatures, st);
    if (rc) return rc;
    for (int step = 1; step <= max_steps; step++) {
        queries_.clear();
        for (PassCam &p : pc) {
            const Cam &cam = cams_[p.cam];
            for (size_t i = 0; i < p.dets->size(); i++) {
                const size_t k = p.k0 + i;
                // the chain has ended (count 0 on the device): an empty query
                psn_lk_query q = Query(cam.ring[kT2dInterval - 1], cam.ring[kT2dInterval - 1], k * cap, cap);
                if (step <= b.h_last[k]) {  // frame t-s+1 -> t-s with the square box-width window (:776-782)
                    q.prev_slot = cam.ring[kT2dInterval - step];
                    q.next_slot = cam.ring[kT2dInterval - 1 - step];
                    q.params.win_w = q.params.win_h = (int)(b.h_boxes[4 * k + 2] * kWinSizeRatio);
                }
                queries_.push_back(q);
            }
        }
        const float *in = step == 1 ? db.d_in : db.d_buf[step & 1];
        rc = psn_lk_track_device_counted(lk_, queries_.data(), (int)K, db.d_cnt, in, db.d_out, db.d_status, db.d_err);
        if (rc) return fail(rc, "psn_lk_track_device_counted");
        cd.cur = in;
        cd.nxt = db.d_out;
        cd.next_in = db.d_buf[(step + 1) & 1];
        rc = psn_t2d_chain_step_device(&cd, step, st);
        if (rc) return fail(rc, "psn_t2d_chain_step_device");
        // set 0 is final after step 1: the next frame's forward launch may read it
        if (step == 1) Chk(sched_.set0[rb].record(st), "set-0 event", rc);
    }
    if (max_steps == 0) Chk(sched_.set0[rb].record(st), "set-0 event", rc);
    ci.valid = rc == PSN_LK_OK;
    return rc;
}

// The forward calls of frame t+1 (:871-877) straight from frame t's chain pass
// (result block src_rb): every detection of frame t becomes an active tracker
// -- matched ones take the detection's box and its set 0, new ones start from
// them (:1087, :1104, :1112-1147) -- so their LK inputs are on the device before
// the host has matched frame t. One counted launch on the forward stream, after
// the pass's set 0 is final and the frames are built: query k reads set 0 of
// detection k (count = its set-0 count, 0 for a detection that is no tracker)
// with the window of its box; the outputs land at the same index in the forward
// result block. pc: the pass of frame t+1 (its frames adopted).
int Tracker2DFlow::LaunchForwardFromChains(std::vector<PassCam> &pc, int src_rb, bool host_fallback) {
    for (PassCam &p : pc) p.fwd_rb = -1;
    if (src_rb < 0 || !sched_.chain_info[src_rb].valid || sched_.chain_info[src_rb].K == 0 || !dev_ ||
        !dev_->d_res[src_rb]) {
        if (!host_fallback) return PSN_LK_OK;
        // the chain results are gone (the chain buffers grew since): the trackers'
        // set 0 from the host, one call per tracker; a window the LK cannot run is
        // a placeholder (the frame fails at its completion, as from the device)
        for (PassCam &p : pc) {
            Cam &cam = cams_[p.cam];
            cam.fwd.clear();
            ForwardJobs(cam.ring, scale_, cam.trackers, cam.fstatus, cam.fwd);
            for (Job &jb : cam.fwd)
                if (WindowError(jb.win_w, jb.win_h)) jb.win_w = jb.win_h = 3;
            p.fwd = &cam.fwd;
        }
        return PassLaunchForward(pc);
    }
    const ChainInfo &ci = sched_.chain_info[src_rb];
    const size_t cap = PSN_T2D_CHAIN_CAP, S = PSN_T2D_CHAIN_STEPS, K = ci.K;
    int rc = EnsureForward(K * S * cap, K);
    if (rc) return rc;
    DeviceBuffers &b = *dev_;
    const int par = sched_.fwd_par ^ 1;  // the block the last-but-one launch wrote: its copy waited for below
    hipStream_t fs = FwdStream(par);
    fwd_queries_.assign(K, psn_lk_query{});
    for (PassCam &p : pc) {
        if (p.cam >= ci.k0.size()) continue;
        const Cam &cam = cams_[p.cam];
        for (size_t i = 0; i < ci.ndet[p.cam]; i++) {
            const size_t k = ci.k0[p.cam] + i;
            psn_lk_query &q = fwd_queries_[k];
            q = Query(cam.ring[kT2dInterval - 2], cam.ring[kT2dInterval - 1], k * S * cap, cap);  // frame t -> t+1
            const int ww = ci.win[k].first, wh = ci.win[k].second;
            // a window the LK cannot run: a placeholder (the frame fails at its
            // completion if that detection became a tracker, as the reference's
            // CV_Assert would)
            const bool ok = WindowError(ww, wh) == PSN_LK_OK;
            q.params.win_w = ok ? ww : 3;
            q.params.win_h = ok ? wh : 3;
        }
    }
    const DeviceBuffers::ResView rv = b.view(b.d_res[src_rb]);
    if (sched_.set0[src_rb].wait_on(fs) != hipSuccess || sched_.fcopied[par].wait_on(fs) != hipSuccess) {
        err_ = "forward: set-0 / block events";
        return PSN_LK_ERR_HIP;
    }
    hipError_t recorded = hipSuccess;
    rc = OnForwardStream(par, [&] {
        return psn_lk_track_device_counted_strided(lk_, fwd_queries_.data(), (int)K, rv.setcnt, (int)S, rv.sets,
                                                   b.d_fout[par], b.d_fstatus[par], b.d_ferr[par]);
    }, recorded);
    if (rc) return rc;
    if (recorded != hipSuccess) {
        err_ = "forward: end event";
        return PSN_LK_ERR_HIP;
    }
    if (sched_.fread[src_rb].record(fs) != hipSuccess) {
        err_ = "forward: read event";
        return PSN_LK_ERR_HIP;
    }
    for (PassCam &p : pc) {
        p.fwd_rb = src_rb;
        p.fwd_n = K * S * cap;
        p.fwd_par = par;
    }
    return PSN_LK_OK;
}

// 3 of the pass: the forward calls of every camera's trackers, on the forward
// stream, in their own arrays (every LK launch waits for the builds of the
// slots it reads).
int Tracker2DFlow::PassLaunchForward(std::vector<PassCam> &pc) {
    size_t J = 0, F = 0;
    for (PassCam &p : pc) {
        p.j0 = J;
        p.f0 = F;
        if (p.fwd) {
            J += p.fwd->size();
            for (const Job &jb : *p.fwd) F += jb.in->size();
        }
    }
    if (J == 0) return PSN_LK_OK;
    int rc = EnsureForward(F, J);
    if (rc) return rc;
    DeviceBuffers &b = *dev_;
    const int par = sched_.fwd_par ^ 1;
    hipStream_t fs = FwdStream(par);
    size_t o = 0;
    fwd_queries_.clear();
    for (PassCam &p : pc) {
        if (!p.fwd) continue;
        for (const Job &jb : *p.fwd) {
            const std::vector<Point2f> &pts = *jb.in;
            psn_lk_query q = Query(jb.prev_slot, jb.next_slot, o, pts.size());
            q.params.win_w = jb.win_w;
            q.params.win_h = jb.win_h;
            b.h_fcnt[fwd_queries_.size()] = (int)pts.size();
            fwd_queries_.push_back(q);
            for (size_t i = 0; i < pts.size(); i++, o++) {
                b.h_fin[2 * o] = pts[i].x;
                b.h_fin[2 * o + 1] = pts[i].y;
            }
        }
    }
    // counts and points in one copy
    // (one input block: the other stream's last launch has read it)
    Chk(sched_.fend[par ^ 1].wait_on(fs), "forward input block event", rc);
    Chk(sched_.fcopied[par].wait_on(fs), "forward block event", rc);
    if (!rc && (rc = psn_t2d_upload_device(b.d_fiblk, b.h_fiblk, b.fi_off_pts + F * 8, fs)))
        err_ = "forward inputs upload";
    if (rc) return rc;
    hipError_t recorded = hipSuccess;
    rc = OnForwardStream(par, [&] {
        return psn_lk_track_device_counted(lk_, fwd_queries_.data(), (int)J, b.d_fcnt, b.d_fin, b.d_fout[par],
                                           b.d_fstatus[par], b.d_ferr[par]);
    }, recorded);
    if (rc) return rc;
    Chk(recorded, "forward end event", rc);
    for (PassCam &p : pc) p.fwd_par = par;
    return rc;
}

// Wait for the pass and unpack it: features (GridFAST mode), every valid
// detection's chain (boxes, point sets), the forward outputs.
int Tracker2DFlow::PassComplete(std::vector<PassCam> &pc, bool gridfast) {
    int rc = PassWait(pc);
    if (!rc) rc = PassFeatures(pc, gridfast);
    if (!rc) PassUnpack(pc);
    return rc;
}

// Enqueue the result copies and wait for the pass's device work.
int Tracker2DFlow::PassWait(std::vector<PassCam> &pc) {
    const int rc = PassCopy(pc);
    return rc ? rc : PassSync();
}

int Tracker2DFlow::PassCopy(std::vector<PassCam> &pc) {
    int rc = PSN_LK_OK;
    const size_t cap = PSN_T2D_CHAIN_CAP, S = PSN_T2D_CHAIN_STEPS;
    DeviceBuffers *bp = dev_.get();
    size_t K = 0, F = 0;
    for (PassCam &p : pc) {
        K += p.dets->size();
        if (p.fwd)
            for (const Job &jb : *p.fwd) F += jb.in->size();
    }
    hipStream_t st = pc.empty() ? LkStream() : ChainStream(pc[0].set),
                fs = FwdStream(pc.empty() ? sched_.fwd_par : pc[0].fwd_par);
    const int rb = pc.empty() ? -1 : pc[0].rb;
    if (K && bp && rb >= 0)
        if (!rc && (rc = psn_t2d_download_device(bp->h_res[rb], bp->d_res[rb], bp->res_sets_off + K * S * cap * 8, st)))
            err_ = "chain results download";
    if (!pc.empty() && pc[0].fwd_rb >= 0) F = pc[0].fwd_n;  // the forward launch from the previous frame's chains
    if (F && bp) {
        // status and points in one copy, on the chain stream after the forward
        // launch (the forward stream goes on with the next frame's launch)
        const int par = pc[0].fwd_par;
        Chk(sched_.fend[par].wait_on(st), "forward end wait", rc);
        if (!rc && (rc = psn_t2d_download_device(bp->h_foblk, bp->d_foblk[par], bp->fo_off_pts + F * 8, st)))
            err_ = "forward results download";
        Chk(sched_.fcopied[par].record(st), "forward copied event", rc);
    }
    // everything the pass enqueued precedes these records (the forward work of
    // a pass without result copy: the forward stream's record)
    Chk(sched_.chain_done.record(st), "chain results event", rc);
    Chk(sched_.fwd_done.record(fs), "forward results event", rc);
    if (rc) {  // PassSync waits for both or for neither
        sched_.chain_done.forget();
        sched_.fwd_done.forget();
    }
    return rc;
}

// Poll the completion events (a blocking stream sync sleeps and wakes ~0.1 ms
// late; the next frame's work is enqueued right after this returns). Past a
// short spin every poll yields the core: ranks sharing a GPU's CPU allotment
// keep their cores for the host work of their own frames.
int Tracker2DFlow::PassSync() {
    for (int i = 0; i < 2; i++) {
        Event &e = i ? sched_.fwd_done : sched_.chain_done;
        if (!e.recorded()) continue;
        hipError_t q;
        for (unsigned n = 0; (q = e.query()) == hipErrorNotReady; n++) {
            if (n < 256)
                __builtin_ia32_pause();
            else
                sched_yield();
        }
        e.forget();
        if (q != hipSuccess) {
            err_ = std::string(i ? "forward" : "chain") + " sync: " + hipGetErrorString(q);
            return PSN_LK_ERR_HIP;
        }
    }
    return PSN_LK_OK;
}

// After PassWait: GridFAST features (the pass's staging set) and window errors.
int Tracker2DFlow::PassFeatures(std::vector<PassCam> &pc, bool gridfast) {
    if (!gridfast || pc.empty() || !dev_) return PSN_LK_OK;
    const size_t cap = PSN_T2D_CHAIN_CAP;
    const DeviceBuffers::Stage *bp = &dev_->stage[pc[0].set];
    const std::vector<char> &win_bad_ = win_bad_sets_[pc[0].set];
    for (PassCam &p : pc) {
        const size_t n = p.dets->size();
        p.features->assign(n, {});
        for (size_t i = 0; i < n; i++) {
            const size_t k = p.k0 + i;
            const int m = bp->h_rawcnt[k];
            // a window the LK cannot run fails the frame only if the chain had to run it (:744)
            if (win_bad_[k] && (size_t)m >= kT2dMinFeatures) {
                err_ = "detection " + std::to_string(i) + " window";
                const int win = (int)(bp->h_boxes[4 * k + 2] * kWinSizeRatio);
                return WindowError(win, win);
            }
            const float *xy = bp->h_in + 2 * cap * k;
            (*p.features)[i].resize((size_t)m);
            for (int j = 0; j < m; j++) (*p.features)[i][(size_t)j] = Point2f{xy[2 * j], xy[2 * j + 1]};
        }
    }
    return PSN_LK_OK;
}

// After PassWait: the chains' boxes and point sets (h_res) and the forward
// outputs, which a next pass's chain launch leaves alone (unless it regrows the
// chain buffers: ChainsFit).
void Tracker2DFlow::PassUnpack(std::vector<PassCam> &pc) {
    const size_t cap = PSN_T2D_CHAIN_CAP, S = PSN_T2D_CHAIN_STEPS;
    DeviceBuffers *bp = dev_.get();
    for (PassCam &p : pc) {
        std::vector<Chain> chains;
        BackwardBegin(*p.dets, *p.features, *p.out, chains);  // valid detections, in order
        const DeviceBuffers::ResView hv = p.out->empty() ? DeviceBuffers::ResView{} : bp->view(bp->h_res[p.rb]);
        for (DetectedObject &ob : *p.out) {
            const size_t k = p.k0 + ob.id;  // the detection index = its device chain
            const int ns = hv.nsteps[k];
            for (int s2 = 1; s2 <= ns; s2++) {
                const double *r = hv.obox + (k * S + s2) * 4;
                ob.boxes.push_back(Rect(r[0], r[1], r[2], r[3]).scale(1.0 / scale_));
            }
            for (int r = 0; ns > 0 && r <= ns; r++) {
                const int m = hv.setcnt[k * S + r];
                const float *pp = hv.sets + (k * S + r) * cap * 2;
                std::vector<Point2f> v((size_t)m);
                for (int i = 0; i < m; i++) v[(size_t)i] = Point2f{pp[2 * i], pp[2 * i + 1]};
                ob.vecvecTrackedFeatures.push_back(std::move(v));
            }
        }
        if (p.fwd_rb >= 0) {  // forward outputs of the camera's trackers, at their source detection's index
            Cam &cam = cams_[p.cam];
            cam.fstatus.assign(cam.trackers.size(), {});
            for (size_t j = 0; j < cam.trackers.size(); j++) {
                Tracker2D *tr = cam.trackers[j];
                const size_t off = (cam.fwd_k0 + (size_t)tr->srcDet) * S * cap, m = tr->featurePoints.size();
                tr->trackedPoints.resize(m);
                cam.fstatus[j].resize(m);
                for (size_t i = 0; i < m; i++) {
                    tr->trackedPoints[i] = Point2f{bp->h_fwd_out[2 * (off + i)], bp->h_fwd_out[2 * (off + i) + 1]};
                    cam.fstatus[j][i] = bp->h_fwd_st[off + i];
                }
            }
            continue;
        }
        if (!p.fwd) continue;
        for (size_t j = 0, off = p.f0; j < p.fwd->size(); j++) {
            Job &jb = (*p.fwd)[j];
            const size_t m = jb.in->size();
            jb.out->resize(m);
            jb.status->resize(m);
            for (size_t i = 0; i < m; i++, off++) {
                (*jb.out)[i] = Point2f{bp->h_fwd_out[2 * off], bp->h_fwd_out[2 * off + 1]};
                (*jb.status)[i] = bp->h_fwd_st[off];
            }
        }
    }
}

bool Tracker2DFlow::ChainsFit(const std::vector<CamFrame> &io) const {
    size_t K = 0;
    for (const CamFrame &f : io) K += f.dets.size();
    return K == 0 || (dev_ && dev_->sc[0].d_in && dev_->nchains >= K);
}

// One camera (0), one pass, synchronous.
int Tracker2DFlow::DevicePass(const std::vector<Detection> &dets, std::vector<std::vector<Point2f>> &features,
                              std::vector<DetectedObject> &out, std::vector<Job> *fwd, bool gridfast, uint32_t seed) {
    std::vector<PassCam> pc(1);
    pc[0].cam = 0;
    pc[0].dets = &dets;
    pc[0].features = &features;
    pc[0].out = &out;
    pc[0].fwd = fwd;
    out.clear();
    int rc = PassLaunch(pc, gridfast, seed);
    if (rc) {  // drain what was enqueued before returning the error
        SyncChains();
        SyncForward();
        return rc;
    }
    return PassComplete(pc, gridfast);
}

}  // namespace psn
