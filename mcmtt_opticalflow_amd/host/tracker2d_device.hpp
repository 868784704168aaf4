// Device handles and buffers of Tracker2DFlow's device pass (tracker2d_pass.cpp):
// owning stream and event handles, and the device / pinned-host buffers.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <utility>
#include <vector>

#include "psn_t2d_device.h"
#include "tracker2d_steps.hpp"

namespace psn {

// A non-blocking stream with a priority; reset() drains and destroys it.
class Stream {
  public:
    Stream() = default;
    ~Stream() { reset(); }
    Stream(Stream &&o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    Stream &operator=(Stream &&o) noexcept {
        std::swap(s_, o.s_);
        return *this;
    }
    bool create(int priority) {
        reset();
        return hipStreamCreateWithPriority(&s_, hipStreamNonBlocking, priority) == hipSuccess;
    }
    void reset() {
        if (!s_) return;
        sync();
        (void)hipStreamDestroy(s_);
        s_ = nullptr;
    }
    void sync() const {
        if (s_) (void)hipStreamSynchronize(s_);
    }
    hipStream_t get() const { return s_; }

  private:
    hipStream_t s_ = nullptr;
};

// An event without timing that knows whether a record is outstanding: waits on
// an event never recorded (or already consumed: forget) are skipped by its users.
class Event {
  public:
    Event() = default;
    ~Event() { reset(); }
    Event(Event &&o) noexcept : e_(std::exchange(o.e_, nullptr)), recorded_(std::exchange(o.recorded_, false)) {}
    Event &operator=(Event &&o) noexcept {
        std::swap(e_, o.e_);
        std::swap(recorded_, o.recorded_);
        return *this;
    }
    bool create() {
        reset();
        return hipEventCreateWithFlags(&e_, hipEventDisableTiming) == hipSuccess;
    }
    void reset() {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
        recorded_ = false;
    }
    hipError_t record(hipStream_t s) {
        const hipError_t r = hipEventRecord(e_, s);
        recorded_ = r == hipSuccess;
        return r;
    }
    hipError_t wait_on(hipStream_t s) const { return hipStreamWaitEvent(s, e_, 0); }  // s waits for the event
    hipError_t query() const { return hipEventQuery(e_); }
    bool recorded() const { return recorded_; }
    void forget() { recorded_ = false; }

  private:
    hipEvent_t e_ = nullptr;
    bool recorded_ = false;
};

// The allocations of one buffer family, registered where they are made; once
// one fails the rest are not attempted (ok stays false until release).
struct Allocations {
    std::vector<void *> dev, host;
    bool ok = true;
    template <class T>
    void device(T *&p, size_t bytes) {
        void *q = nullptr;
        ok = ok && hipMalloc(&q, bytes) == hipSuccess;
        if (q) dev.push_back(q);
        p = (T *)q;
    }
    template <class T>
    void pinned(T *&p, size_t bytes) {
        void *q = nullptr;
        ok = ok && hipHostMalloc(&q, bytes, hipHostMallocCoherent) == hipSuccess;
        if (q) host.push_back(q);
        p = (T *)q;
    }
    void release() {
        for (void *p : dev) (void)hipFree(p);
        for (void *p : host) (void)hipHostFree(p);
        dev.clear();
        host.clear();
        ok = true;
    }
};

// Buffer capacities grow geometrically (powers of two from `floor`): a regrow
// drains the streams and reallocates pinned memory (milliseconds), so a
// tracker population that creeps up frame by frame regrows O(log n) times.
inline size_t grow_cap(size_t need, size_t floor) {
    size_t c = floor;
    while (c < need) c *= 2;
    return c;
}

// The backward chains' buffers, for nchains detections.
struct ChainBuffers {
    size_t nchains = 0;
    // per staging set (a pass and its chain stream): inputs, LK outputs, ping-pong
    // point sets, err/status -- consecutive passes run on the two chain streams at once
    struct Scratch {
        char *d_inblk = nullptr;
        float *d_in = nullptr, *d_out = nullptr, *d_buf[2] = {nullptr, nullptr}, *d_err = nullptr;
        uint8_t *d_status = nullptr;
        double *d_boxes = nullptr;
        int *d_cnt = nullptr, *d_tot = nullptr, *d_last = nullptr;
    } sc[2];
    // pinned staging of the chain inputs (and GridFAST features), two sets: a
    // pass's set is written by its launch and read back by its completion, and
    // the next frame's chains may be launched in between (RunComplete with next)
    // [boxes f64 x4 | last steps | counts | (256-B aligned) points] per chain, one block per
    // side so that one copy carries a pass's inputs (carve_in)
    struct Stage {
        char *h_inblk = nullptr;
        float *h_in = nullptr;
        double *h_boxes = nullptr;
        int *h_cnt = nullptr, *h_rawcnt = nullptr, *h_last = nullptr;
    } stage[2];
    size_t in_off_last = 0, in_off_cnt = 0, in_off_in = 0, in_bytes = 0;
    void layout_in(size_t K, size_t cap) {
        in_off_last = K * 32;
        in_off_cnt = in_off_last + K * 4;
        in_off_in = (in_off_cnt + K * 4 + 255) & ~(size_t)255;
        in_bytes = in_off_in + K * cap * 8;
    }
    void carve_in(char *base, double *&boxes, int *&last, int *&cnt, float *&in) const {
        boxes = (double *)base;
        last = (int *)(base + in_off_last);
        cnt = (int *)(base + in_off_cnt);
        in = (float *)(base + in_off_in);
    }
    // the chain's results live in one block per side, [nsteps | set counts | boxes | sets], so that
    // one memset clears the counters and one copy returns every used byte
    // Three result blocks, used by consecutive passes in turn: a pass's block is
    // read by the next frame's forward launch (its set 0: the trackers' features)
    // while the chains of the frame after write theirs.
    static constexpr int kResBlocks = kT2dResBlocks;
    char *d_res[kResBlocks] = {}, *h_res[kResBlocks] = {};
    size_t res_sets_off = 0;
    struct ResView {
        int *nsteps, *setcnt;
        double *obox;
        float *sets;
    };
    ResView view(char *base) const {
        ResView v{};
        v.nsteps = (int *)base;
        v.setcnt = v.nsteps + nchains;
        v.obox = (double *)(base + res_box_off(nchains, PSN_T2D_CHAIN_STEPS));
        v.sets = (float *)(base + res_sets_off);
        return v;
    }
    static size_t res_box_off(size_t K, size_t S) { return (K * (1 + S) * 4 + 255) & ~(size_t)255; }
};

// The forward calls' buffers, for nfwd_pts points in nfwd_jobs calls.
struct ForwardBuffers {
    size_t nfwd_pts = 0, nfwd_jobs = 0;
    // inputs [counts | (256-B aligned) points], outputs [status | (aligned) points] (one copy each)
    float *d_fin = nullptr, *d_fout[2] = {nullptr, nullptr}, *d_ferr[2] = {nullptr, nullptr};
    uint8_t *d_fstatus[2] = {nullptr, nullptr};
    int *d_fcnt = nullptr;
    char *d_fiblk = nullptr, *d_foblk[2] = {nullptr, nullptr}, *h_fiblk = nullptr, *h_foblk = nullptr;
    size_t fi_off_pts = 0, fo_off_pts = 0;
    // pinned staging: forward inputs, then results
    float *h_fin = nullptr, *h_fwd_out = nullptr;
    uint8_t *h_fwd_st = nullptr;
    int *h_fcnt = nullptr;
};

// Device and pinned-host buffers of a device pass (grown on demand by
// EnsureChains / EnsureForward). The backward chains and the forward calls have
// separate arrays: a frame's chains may run (launched ahead, RunComplete with a
// next frame) while its forward inputs are staged and, if need be, its forward
// buffers regrown. The caller drains the streams that use a family before
// releasing it.
struct DeviceBuffers : ChainBuffers, ForwardBuffers {
    Allocations chain_mem, fwd_mem;
    DeviceBuffers() = default;
    DeviceBuffers(const DeviceBuffers &) = delete;
    DeviceBuffers &operator=(const DeviceBuffers &) = delete;
    ~DeviceBuffers() {
        release_chains();
        release_forward();
    }
    void release_chains() {
        chain_mem.release();
        static_cast<ChainBuffers &>(*this) = ChainBuffers();
    }
    void release_forward() {
        fwd_mem.release();
        static_cast<ForwardBuffers &>(*this) = ForwardBuffers();
    }
};

}  // namespace psn
