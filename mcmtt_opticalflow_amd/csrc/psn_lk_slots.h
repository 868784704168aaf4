// The ordering of a context's ring slots between streams.
//
// Pyramid builds may run on their own streams (ingest overlap), ordered against
// the launches that read a slot by per-slot events: READY after every build
// (waited for by every launch that reads the slot, on whatever stream it runs),
// FREE after the reads (one event per reading stream, all waited for by the
// next build into the slot).
#pragma once

#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <utility>
#include <vector>

#include "psn_lk_plan.h"

// A failed HIP call: its text into `err` (std::string), PSN_LK_ERR_HIP to the caller.
#define PSN_HIPCHK(err, expr)                                                                          \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return psn::set_err((err), PSN_LK_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                __FILE__, __LINE__);                                                   \
    } while (0)

namespace psn {

// slot events only order streams of one device: a device-scope release suffices
constexpr unsigned kSlotEventFlags = hipEventDisableTiming | hipEventReleaseToDevice;

class SlotOrder {
public:
    // Events of `nslots` slots; failures put their text into *err (the context's).
    int init(int nslots, std::string *err) {
        err_ = err;
        nslots_ = nslots;
        slot_ready_.assign(nslots, nullptr);
        slot_free_.assign(nslots, {});
        ready_rec_.assign(nslots, 0);
        build_gen_.assign(nslots, 0);
        waited_.assign(nslots, {});
        copy_done_.assign(nslots, nullptr);
        for (int i = 0; i < nslots; i++) {
            if (hipEventCreateWithFlags(&slot_ready_[i], kSlotEventFlags) != hipSuccess) return PSN_LK_ERR_HIP;
            if (hipEventCreateWithFlags(&copy_done_[i], kSlotEventFlags) != hipSuccess) return PSN_LK_ERR_HIP;
        }
        return PSN_LK_OK;
    }
    void destroy() {
        for (auto *v : {&slot_ready_, &copy_done_})
            for (auto e : *v)
                if (e) (void)hipEventDestroy(e);
        slot_free_.clear();
        for (auto *se : ev_all_) {
            (void)hipEventDestroy(se->e);
            delete se;
        }
        ev_all_.clear();
        ev_free_.clear();
    }

    // A build of `slot` was just enqueued on s: its ready event is recorded there.
    int mark_built(int slot, hipStream_t s) {
        PSN_HIPCHK(*err_, hipEventRecord(slot_ready_[slot], s));
        ready_rec_[slot] = 1;
        build_gen_[slot]++;
        bool mine = false;  // the building stream is ordered after the build
        for (auto &w : waited_[slot])
            if (w.first == s) w.second = build_gen_[slot], mine = true;
        if (!mine) waited_[slot].emplace_back(s, build_gen_[slot]);
        return PSN_LK_OK;
    }
    // The slot's next build is deferred (a fused-mode push): it runs first on the
    // LK stream, so readers wait for it by stream order, not by an event.
    void defer(int slot) { ready_rec_[slot] = 0; }
    bool has_build(int slot) const { return ready_rec_[slot] != 0; }
    // Make s wait for the last build of `slot` (a no-op on the device when the
    // build ran earlier on the same stream or has completed).
    int wait_ready(int slot, hipStream_t s) {
        if (slot < 0 || slot >= nslots_ || !ready_rec_[slot]) return PSN_LK_OK;
        // a stream that has waited for this build already is ordered after it
        for (auto &w : waited_[slot])
            if (w.first == s) {
                if (w.second == build_gen_[slot]) return PSN_LK_OK;
                PSN_HIPCHK(*err_, hipStreamWaitEvent(s, slot_ready_[slot], 0));
                w.second = build_gen_[slot];
                return PSN_LK_OK;
            }
        PSN_HIPCHK(*err_, hipStreamWaitEvent(s, slot_ready_[slot], 0));
        waited_[slot].emplace_back(s, build_gen_[slot]);
        return PSN_LK_OK;
    }
    // Make s wait for the slot's last recorded build (it may run on another
    // ingest stream and still read the slot's staging buffer or write its pyramid).
    int wait_prev_build(int slot, hipStream_t s) {
        if (ready_rec_[slot]) PSN_HIPCHK(*err_, hipStreamWaitEvent(s, slot_ready_[slot], 0));
        return PSN_LK_OK;
    }
    // Make s wait until every recorded read of `slot` is done (before a new build into it).
    int wait_free(int slot, hipStream_t s) {
        for (auto &se : slot_free_[slot])
            if (se.first != s) PSN_HIPCHK(*err_, hipStreamWaitEvent(s, se.second->e, 0));
        return PSN_LK_OK;
    }
    // Make stream `on` wait for the reads of `slot` recorded on stream `reader`.
    int wait_free_of(int slot, hipStream_t reader, hipStream_t on) {
        for (auto &se : slot_free_[slot])
            if (se.first == reader) PSN_HIPCHK(*err_, hipStreamWaitEvent(on, se.second->e, 0));
        return PSN_LK_OK;
    }
    // After a launch on s read `slots`: ONE event recorded behind it becomes that
    // stream's free event of every slot read (a later build into one of them waits
    // for it). An event returns to the pool when no slot refers to it;
    // re-recording a pooled event never moves a live reference.
    int record_free(const int *slots, int n, hipStream_t s) {
        SharedEv *e = nullptr;
        if (!ev_free_.empty()) {
            e = ev_free_.back();
            ev_free_.pop_back();
        } else {
            e = new (std::nothrow) SharedEv();
            if (!e) return set_err(*err_, PSN_LK_ERR_NOMEM, "slot event");
            if (hipEventCreateWithFlags(&e->e, kSlotEventFlags) != hipSuccess) {
                delete e;
                return set_err(*err_, PSN_LK_ERR_HIP, "hipEventCreateWithFlags (slot event)");
            }
            ev_all_.push_back(e);
        }
        PSN_HIPCHK(*err_, hipEventRecord(e->e, s));
        for (int i = 0; i < n; i++) {
            const int slot = slots[i];
            if (slot < 0 || slot >= nslots_) continue;
            bool found = false;
            for (auto &se : slot_free_[slot])
                if (se.first == s) {
                    if (se.second != e) {
                        e->refs++;
                        unref(se.second);
                        se.second = e;
                    }
                    found = true;
                    break;
                }
            if (!found) {
                e->refs++;
                slot_free_[slot].emplace_back(s, e);
            }
        }
        if (e->refs == 0) ev_free_.push_back(e);
        return PSN_LK_OK;
    }
    // psn_lk_push_frame_async: recorded behind the upload into the slot's staging buffer
    hipEvent_t copy_done(int slot) const { return copy_done_[slot]; }

private:
    std::string *err_ = nullptr;
    int nslots_ = 0;
    std::vector<hipEvent_t> slot_ready_, copy_done_;
    std::vector<char> ready_rec_;
    // per slot: its build generation (slot_ready re-recorded), and per stream the
    // generation that stream has waited for already (no repeated waits)
    std::vector<unsigned> build_gen_;
    std::vector<std::vector<std::pair<hipStream_t, unsigned>>> waited_;
    // per slot: per stream the event of the last launch on it that read the slot;
    // one event per launch, shared by every slot it read (refcounted, pooled)
    struct SharedEv {
        hipEvent_t e = nullptr;
        int refs = 0;
    };
    std::vector<SharedEv *> ev_all_, ev_free_;
    std::vector<std::vector<std::pair<hipStream_t, SharedEv *>>> slot_free_;
    void unref(SharedEv *e) {
        if (e && --e->refs == 0) ev_free_.push_back(e);
    }
};

}  // namespace psn
