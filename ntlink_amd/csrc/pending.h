/*
 * Lazy completion of a context's result handles: host code over the HIP runtime's events, nothing of the context in it.
 * A call that makes a sketch or a map result only queues device work; the handle embeds a Pending and the context owns one PendingQueue.
 *   PendingQueue  setup / destroy; event_get / event_put: the free list of ordering events (every user of the context: batch `ready`,
 *                 index `built`, mask `clean`, the throttle, main_wait, window -> emit); slot_get / slot_put: the page-locked slots the
 *                 kernels write sizes and sums into, slot_dev / slot_dsums: a slot's device view and its entry of the device-side array;
 *                 reap(block): the orphans whose event has passed, in queue order; async_err: the first failure reap met (ntl_ctx_sync).
 *   Pending       done, slot, pending, failed, and the holds: what the queued kernels still read, as {pointer, release} pairs.
 *                 arm: event + slot (false: none to be had, nothing kept).  wait: for `done`.  settle: event, slot and holds go back NOW
 *                 and are nulled (idempotent) -- the caller knows the work has run, or that the device is idle.  orphan: the handle is
 *                 being destroyed; while `pending`, event, slot and holds move onto the queue with a check, and reap settles them once
 *                 the event has passed; else settle.
 *   a check       reads the slot of an orphan whose work has run (results nobody looked at still must not have failed silently): the
 *                 message for async_err, or NULL; it may store the batch's hit fraction.
 * THREADS: queue and handles belong to the thread that drives the context.  Nothing here is locked.  The one foreign-thread path stays
 * where it was: a hold's release gets the REAPING queue's owner, and index_unref(ix, by) sends the blocks of an index that another
 * context built through DevPool::free_uncached.
 * INVARIANT: a slot (and an event, and what the holds keep alive) is reused only after the event of its previous holder has passed, or
 * after both streams were drained (the error paths: settle behind sync_both).
 * As found, and kept (ntl_hip.hip): a destroyed pending SKETCH lets go of its batch at once (the batch's blocks return stream-ordered)
 * and holds only the index; a destroyed pending MAP RESULT holds index and batch until reaped (the map kernels read d_seq_len);
 * sketch_finalize settles on completion, not on destroy (thousands of completed handles live on 512 slots); the nfound_owed hand-over
 * records `done` a second time, behind the kernel that took the count over; slot_get, with no slot free, waits for the OLDEST orphan
 * only; once async_err is set, later orphans are settled unchecked.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <chrono>
#include <deque>
#include <memory>
#include <string>
#include <vector>

struct PinSlot { uint64_t w[8]; }; /* 64 page-locked bytes a device-side size lands in */

typedef const char *(*PendingCheck)(const PinSlot &, uint64_t arg, std::atomic<float> *hitf);
struct Hold { const void *p = nullptr; void (*release)(const void *p, void *by) = nullptr; }; /* by: the owner of the queue that lets go */

struct PendingQueue;

struct Pending {
    hipEvent_t done = nullptr;
    PinSlot *slot = nullptr;
    bool pending = false;
    int failed = 0; /* sticky error code of the completion */
    Hold holds[2];

    inline bool arm(PendingQueue &q);
    inline void settle(PendingQueue &q);
    inline void orphan(PendingQueue &q, PendingCheck check, uint64_t arg, const std::shared_ptr<std::atomic<float>> &hitf = nullptr);
    /* Waits for an event the host needs NOW: polls for a while before it blocks -- a blocking wait is woken by an interrupt some tens
       of microseconds after the event has passed. */
    hipError_t wait() const
    {
        static const int spin_us = [] { const char *v = getenv("NTL_SYNC_SPIN_US"); return v ? atoi(v) : 100; }();
        if (spin_us > 0) {
            const auto t0 = std::chrono::steady_clock::now();
            for (;;) {
                const hipError_t q = hipEventQuery(done);
                if (q == hipSuccess) return hipSuccess;
                if (q != hipErrorNotReady) return q;
                if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > spin_us) break;
            }
        }
        return hipEventSynchronize(done);
    }
};

struct PendingQueue {
    std::string async_err; /* first failure of work whose handle was already gone */

    /* n slots: host[i] as the host reads it, dev[i] as the kernels address it, dsums[i] its entry of the device-side array */
    void setup(PinSlot *host, PinSlot *dev, PinSlot *dsums, uint32_t n, void *owner_)
    {
        slots = host; slots_dev = dev; dslots = dsums; owner = owner_;
        for (uint32_t i = 0; i < n; i++) slot_free.push_back(n - 1 - i);
    }
    /* ordering events come from a free list (creating one costs tens of microseconds) */
    hipEvent_t event_get()
    {
        hipEvent_t e = nullptr;
        if (!ev_free.empty()) { e = ev_free.back(); ev_free.pop_back(); return e; }
        /* hipEventBlockingSync: a host thread that waits on such an event sleeps until the interrupt instead of spinning -- the pair
           driver's worker threads wait for uploads and results most of the time, and on a host that grants the process 16 cores
           every spinning thread is a parser thread less */
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventBlockingSync) != hipSuccess) return nullptr;
        return e;
    }
    void event_put(hipEvent_t e) { if (e) ev_free.push_back(e); }
    /* a zeroed slot; none free: the oldest orphan is waited for */
    PinSlot *slot_get()
    {
        if (slot_free.empty()) reap(true);
        if (slot_free.empty()) return nullptr;
        PinSlot *p = slots + slot_free.back();
        slot_free.pop_back();
        memset(p, 0, sizeof *p);
        return p;
    }
    void slot_put(PinSlot *p) { if (p) slot_free.push_back((uint32_t)(p - slots)); }
    PinSlot *slot_dev(const PinSlot *p) const { return slots_dev + (p - slots); }
    PinSlot *slot_dsums(const PinSlot *p) const { return dslots + (p - slots); }

    /* orphans whose work has finished: check what they carried, settle them.  block: wait for the oldest one. */
    void reap(bool block)
    {
        while (!zombies.empty()) {
            Zombie &z = zombies.front();
            hipError_t q = hipEventQuery(z.what.done);
            if (q == hipErrorNotReady) {
                if (!block) return;
                q = hipEventSynchronize(z.what.done);
                block = false;
            }
            if (q != hipSuccess && async_err.empty()) async_err = std::string("device work failed: ") + hipGetErrorString(q);
            if (q == hipSuccess && z.what.slot && async_err.empty())
                if (const char *m = z.check(*z.what.slot, z.arg, z.hitf.get())) async_err = m;
            Pending what = z.what;
            zombies.pop_front();
            what.settle(*this);
        }
    }
    /* the end of the context: every orphan is waited for, the events go */
    void destroy()
    {
        while (!zombies.empty()) reap(true);
        for (auto e : ev_free) (void)hipEventDestroy(e);
        ev_free.clear();
    }

private:
    friend struct Pending;
    /* what is left of a handle that was destroyed before the device had finished its work */
    struct Zombie {
        Pending what;
        PendingCheck check;
        uint64_t arg;
        std::shared_ptr<std::atomic<float>> hitf; /* where a map result's hit fraction goes: the index itself may be gone */
    };
    PinSlot *slots = nullptr, *slots_dev = nullptr, *dslots = nullptr;
    void *owner = nullptr;
    std::vector<uint32_t> slot_free;
    std::vector<hipEvent_t> ev_free;
    std::deque<Zombie> zombies;
};

inline bool Pending::arm(PendingQueue &q)
{
    done = q.event_get();
    slot = q.slot_get();
    if (done && slot) return true;
    q.event_put(done); done = nullptr;
    q.slot_put(slot); slot = nullptr;
    return false;
}

inline void Pending::settle(PendingQueue &q)
{
    q.event_put(done); done = nullptr;
    q.slot_put(slot); slot = nullptr;
    for (Hold &h : holds) {
        const Hold was = h;
        h = Hold();
        if (was.p) was.release(was.p, q.owner);
    }
}

inline void Pending::orphan(PendingQueue &q, PendingCheck check, uint64_t arg, const std::shared_ptr<std::atomic<float>> &hitf)
{
    if (!pending) { settle(q); return; }
    q.zombies.push_back({*this, check, arg, hitf});
    *this = Pending();
}
