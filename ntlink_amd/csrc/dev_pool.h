/*
 * The device block allocator of a context: host code over the HIP runtime, nothing of the context in it.
 *   take / give             the stream-ordered block cache: a block goes back while kernels that use it may still be queued, and is handed
 *                           out again to work queued BEHIND them on the same stream (no wait); one that was used on several streams goes
 *                           back with an event per stream, and whoever takes it next must not run ahead of the other streams'.
 *   streams                 MAIN, the window stage's (WINDOW) and the side stream of its give-up passes (SIDE); a stream that is not there
 *                           (one-stream contexts, no side stream) counts as the one in front of it: SIDE as WINDOW, WINDOW as MAIN.
 *   alloc_ / free_uncached  what the cache is filled from: blocks up to SLAB_MAX_REQ are cut from slabs of SLAB_BYTES (a hipMalloc costs
 *                           4-9 ms of host time whatever its size, and a context's first read batch asked for seventy: 0.6 s per context of
 *                           a process's first pass, profiles/r04_first_pass.txt); larger ones are the driver's own.
 * A pool belongs to the thread that drives its context; free_uncached alone may be called from another thread (see there).
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <chrono>
#include <deque>
#include <map>
#include <mutex>
#include <unordered_map>
#include <vector>

struct DevPool {
    enum { MAIN = 0, WINDOW = 1, SIDE = 2, NSID = 3 };
    static constexpr int OK = 0, NOMEM = -3; /* NTL_OK, NTL_ENOMEM of include/ntlink_amd.h */
    static constexpr size_t SLAB_BYTES = (size_t)1 << 30, SLAB_MAX_REQ = (size_t)192 << 20;
    /* the cache's misses that reached the driver, and their host time: ntl_prof_get(ctx, "hipMalloc") -- what a process's first pass pays once */
    uint64_t driver_allocs = 0;
    double driver_ms = 0;

    /* window == main: one stream, every request is MAIN's; side == NULL: none, its requests are WINDOW's.  cache_bound: upper bound of
       the bytes the cache holds. */
    void setup(hipStream_t main, hipStream_t window, size_t cache_bound, bool slabs, hipStream_t side = nullptr)
    {
        st[MAIN] = main; st[WINDOW] = window; st[SIDE] = window != main ? side : nullptr;
        pool_cap = cache_bound;
        use_slabs = slabs;
        trace = getenv("NTL_POOL_TRACE") != nullptr; /* diagnostics: every hipMalloc / hipFree of the block cache on stderr */
    }

    /* The window stream becomes MAIN (window == main) or its own stream again -- and the side stream goes or comes with it -- at a quiet
       point: everything queued has run, so every cached block is free on every stream and they all move to MAIN's cache.  (Switching off,
       WINDOW's blocks would otherwise lie stranded -- counted, never handed out; switching on, the window stage's first requests miss
       its own cache once.) */
    void set_window_stream(hipStream_t window, hipStream_t side = nullptr)
    {
        st[WINDOW] = window; st[SIDE] = window != st[MAIN] ? side : nullptr;
        for (int o = WINDOW; o < NSID; o++) {
            for (auto &kv : pool[o]) pool[MAIN].insert(kv);
            pool[o].clear();
        }
        for (auto &kv : xpool) {
            pool[MAIN].insert({kv.first, kv.second.p});
            for (int o = 0; o < NSID; o++) ev_put(kv.second.ev[o]);
        }
        xpool.clear();
    }
    int sid(int want) const
    {
        if (want == SIDE && !st[SIDE]) want = WINDOW;
        return want == WINDOW && st[WINDOW] == st[MAIN] ? (int)MAIN : want;
    }

    /* A block of at least `n` bytes for work queued on stream `sid` from now on; *true_size is what give() wants back. */
    int take(size_t n, int sid_, void **out, size_t *true_size)
    {
        const int sid = this->sid(sid_);
        size_t want = n ? n : 256;
        want = (want + 255) & ~(size_t)255;
        /* Size classes (32 per power of two, at most 3 % over the request): consecutive read batches ask for arrays whose
           sizes differ in the fourth digit, and a cached block a hair smaller than the request is useless -- without classes
           every batch allocated its largest arrays anew while the cache filled with near-misses up to its bound and then
           evicted (hipFree: a device-wide wait) exactly the blocks the next batch wanted (C5: 2.6 s per step instead of 0.45). */
        if (want >= ((size_t)1 << 20)) {
            size_t step = (size_t)1 << 15;
            while ((step << 6) <= want) step <<= 1; /* step = 2^(floor(log2 want) - 5) */
            want = (want + step - 1) & ~(step - 1);
        }
        const size_t most = want + want / 4 + (1 << 20);
        /* look for a cached block; its true size is the map key */
        auto it = pool[sid].lower_bound(want);
        if (it != pool[sid].end() && it->first <= most) {
            *out = it->second; *true_size = it->first;
            pool_bytes -= it->first;
            pool[sid].erase(it);
            return OK;
        }
        /* A block that was used on several streams: one whose work on the OTHER streams has run by now is taken as it is; else a
           new block is made rather than this stream made to wait (two or three blocks per size then go round);
           only when no memory is to be had does the taker wait. */
        auto first = xpool.lower_bound(want), pick = xpool.end();
        for (auto xt = first; xt != xpool.end() && xt->first <= most; ++xt) {
            bool ready = true;
            for (int o = 0; o < NSID; o++)
                if (o != sid && xt->second.ev[o] && hipEventQuery(xt->second.ev[o]) != hipSuccess) { ready = false; break; }
            if (ready) { pick = xt; break; }
        }
        (void)hipGetLastError(); /* (hipErrorNotReady is not an error) */
        if (pick == xpool.end()) {
            const bool busy = first != xpool.end() && first->first <= most; /* a block that fits, still in use on the other stream */
            if (busy ? carve(want, out) : (alloc_uncached(want, out) == OK)) { *true_size = want; return OK; }
            *out = nullptr;
            if (!busy) return NOMEM;
            pick = first; /* out of memory: the oldest candidate, and a wait (alloc_uncached would have dropped it with the cache) */
        }
        XBlock &x = pick->second;
        for (int o = 0; o < NSID; o++) {
            if (o != sid && x.ev[o]) (void)hipStreamWaitEvent(st[sid], x.ev[o], 0);
            ev_put(x.ev[o]);
        }
        *out = x.p; *true_size = pick->first;
        pool_bytes -= pick->first;
        xpool.erase(pick);
        return OK;
    }
    /* A block of take() goes back into the cache; used: bit per stream id that work on the block was queued on. */
    void give(void *p, size_t bytes, unsigned used_)
    {
        if (!p) return;
        unsigned used = 0, n_used = 0; /* as the streams stand now (a block may outlive a switch of set_window_stream) */
        int only = MAIN;
        for (int o = 0; o < NSID; o++)
            if ((used_ & (1u << o)) && !(used & (1u << sid(o)))) { used |= 1u << sid(o); n_used++; only = sid(o); }
        if (n_used == 1) pool[only].insert({bytes, p}); /* one stream: its own cache */
        else {
            XBlock x;
            x.p = p;
            for (int o = 0; o < NSID; o++) {
                if (!(used & (1u << o))) continue;
                x.ev[o] = ev_get();
                if (x.ev[o]) (void)hipEventRecord(x.ev[o], st[o]);
                else (void)hipStreamSynchronize(st[o]); /* no event to be had: the slow, safe way */
            }
            xpool.insert({bytes, x});
        }
        pool_bytes += bytes;
        /* the cache is bounded (half of the device memory unless NTL_POOL_MAX_BYTES says otherwise; a bound below the
           working set of a batch -- tens of GB for 4-Gbases HiFi batches -- turns every release into an eviction): the
           largest blocks go first, they are the least likely to be asked for again at exactly their size */
        while (pool_bytes > pool_cap) {
            std::multimap<size_t, void *> *big = nullptr;
            for (int i = 0; i < NSID; i++)
                if (!pool[i].empty() && (!big || std::prev(pool[i].end())->first > std::prev(big->end())->first)) big = &pool[i];
            if (big && (xpool.empty() || std::prev(big->end())->first >= std::prev(xpool.end())->first)) {
                auto it = std::prev(big->end());
                if (trace) fprintf(stderr, "ntl pool: over the bound, hipFree %.1f MB\n", it->first / 1e6);
                /* safe whatever is still queued: a slab block waits in limbo for every stream, a single block's hipFree for the device */
                free_uncached(it->second, it->first);
                pool_bytes -= it->first;
                big->erase(it);
            } else if (!xpool.empty()) {
                auto it = std::prev(xpool.end());
                free_uncached(it->second.p, it->first);
                for (int o = 0; o < NSID; o++) ev_put(it->second.ev[o]);
                pool_bytes -= it->first;
                xpool.erase(it);
            } else break;
        }
    }
    /* A block that does not come from the cache: a dropped slab block of this size, the slab's next bytes, or the driver's (carve).
       When the driver refuses, the cache is dropped and the request made once more. */
    int alloc_uncached(size_t bytes, void **out)
    {
        if (carve(bytes, out)) return OK;
        drop_cache();
        return hipMalloc(out, bytes) == hipSuccess ? OK : NOMEM;
    }
    /* Gives a block of alloc_uncached (of `bytes`, as asked for there) back.  A single block: hipFree, which waits for the device.  A slab
       block is not waited for: an event is recorded behind each of the streams and the block goes into limbo; it joins the slabs'
       free list when the events have passed (limbo_poll).
       THE ONE METHOD THAT A THREAD OTHER THAN THE POOL'S OWNER MAY CALL: it makes its own events (ev_free is the owner's) and touches only
       what slab_mu guards -- slabs, slab_free, slab_size, slab_limbo (slab_cur / slab_end are not guarded: the owner alone reads and moves
       them).  slab_mu is held around the bookkeeping only, not across the calls that record the events. */
    void free_uncached(void *p, size_t bytes)
    {
        if (!p) return;
        Limbo L = {};
        {
            std::lock_guard<std::mutex> g(slab_mu);
            if (slab_of(p)) {
                L.p = p;
                auto ts = slab_size.find(p);
                L.bytes = ts != slab_size.end() ? ts->second : ((bytes + 255) & ~(size_t)255);
            }
        }
        if (!L.p) { (void)hipFree(p); return; }
        /* what is still queued on the block: an event behind each of the streams; no event to be had: the slow, safe way */
        hipStream_t s[NSID] = {st[MAIN], st[WINDOW] != st[MAIN] ? st[WINDOW] : nullptr, st[SIDE]};
        bool ok = true;
        for (int i = 0; i < NSID && ok; i++)
            if (s[i]) ok = hipEventCreateWithFlags(&L.ev[i], hipEventDisableTiming) == hipSuccess && hipEventRecord(L.ev[i], s[i]) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            for (int i = 0; i < NSID; i++) if (L.ev[i]) { (void)hipEventDestroy(L.ev[i]); L.ev[i] = nullptr; }
            for (int i = 0; i < NSID; i++) if (s[i]) (void)hipStreamSynchronize(s[i]);
        }
        /* (the slab is looked up again: alloc_uncached may have added one meanwhile; this block's own slab stays, it still counts as live) */
        std::lock_guard<std::mutex> g(slab_mu);
        Slab *sl = slab_of(p);
        if (sl && sl->live) sl->live--;
        slab_limbo.push_back(L);
        limbo_poll(false);
    }

    /* Everything cached goes back -- single blocks to the driver, slab blocks to their free list -- and the slabs that hold no live
       block to the driver (after a wait for what is in limbo: memory has run out, its slabs may go). */
    void drop_cache()
    {
        for (int i = 0; i < NSID; i++) {
            for (auto &kv : pool[i]) free_uncached(kv.second, kv.first);
            pool[i].clear();
        }
        for (auto &kv : xpool) {
            free_uncached(kv.second.p, kv.first);
            for (int o = 0; o < NSID; o++) ev_put(kv.second.ev[o]);
        }
        xpool.clear();
        pool_bytes = 0;
        std::lock_guard<std::mutex> g(slab_mu);
        limbo_poll(true);
        for (size_t i = 0; i < slabs.size();) {
            const Slab sl = slabs[i];
            if (sl.live) { i++; continue; }
            auto inside = [&](const void *q) { return (const char *)q >= sl.base && (const char *)q < sl.base + sl.size; };
            for (auto it = slab_free.begin(); it != slab_free.end();) it = inside(it->second) ? slab_free.erase(it) : std::next(it);
            for (auto it = slab_size.begin(); it != slab_size.end();) it = inside(it->first) ? slab_size.erase(it) : std::next(it);
            if (slab_cur >= sl.base && slab_cur <= sl.base + sl.size) slab_cur = slab_end = nullptr;
            (void)hipFree(sl.base);
            slabs.erase(slabs.begin() + (long)i);
        }
    }
    /* The end of the context: its streams are idle and nobody holds a block any more, so every slab counts as empty and goes */
    void destroy()
    {
        for (auto &sl : slabs) sl.live = 0;
        drop_cache();
        for (auto e : ev_free) (void)hipEventDestroy(e);
        ev_free.clear();
    }

private:
    /* a cached block that was used on several streams: whoever takes it waits for the events of the streams it is not on (nullptr: not used there) */
    struct XBlock { void *p = nullptr; hipEvent_t ev[NSID] = {}; };
    struct Slab { char *base; size_t size; size_t live; };
    struct Limbo { void *p; size_t bytes; hipEvent_t ev[NSID]; }; /* a slab block that was given back while work on it may still be queued */
    hipStream_t st[NSID] = {};
    bool use_slabs = true, trace = false;
    /* the cache: owner thread only */
    std::multimap<size_t, void *> pool[NSID]; /* cached blocks by size, per stream they were last used on */
    std::multimap<size_t, XBlock> xpool;      /* ... and those that were used on both */
    size_t pool_bytes = 0;
    size_t pool_cap = (size_t)32 << 30;       /* upper bound of pool_bytes */
    std::vector<hipEvent_t> ev_free;          /* the ordering events of xpool (creating one costs tens of microseconds) */
    /* the slabs: slab_mu guards the next four */
    std::mutex slab_mu;
    std::vector<Slab> slabs;
    std::multimap<size_t, void *> slab_free;      /* dropped slab blocks by size */
    std::unordered_map<void *, size_t> slab_size; /* every slab block's TRUE size (a reused block may be up to 25 % larger than what was asked for) */
    std::deque<Limbo> slab_limbo;                 /* join slab_free when their events have passed (polled by alloc_uncached): no stream is waited for */
    char *slab_cur = nullptr, *slab_end = nullptr; /* the bump pointer: owner thread only (written under slab_mu where slab_free changes with it) */

    hipEvent_t ev_get()
    {
        hipEvent_t e = nullptr;
        if (!ev_free.empty()) { e = ev_free.back(); ev_free.pop_back(); }
        else if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr;
        return e;
    }
    void ev_put(hipEvent_t e) { if (e) ev_free.push_back(e); }
    static hipError_t timed_malloc(void **out, size_t bytes, double *ms)
    {
        const auto t0 = std::chrono::steady_clock::now();
        const hipError_t e = hipMalloc(out, bytes);
        *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return e;
    }
    /* alloc_uncached without its second try */
    bool carve(size_t bytes, void **out)
    {
        if (use_slabs && bytes <= SLAB_MAX_REQ) {
            const size_t need = (bytes + 255) & ~(size_t)255;
            {   /* a dropped slab block of this size (whatever was queued on it has run: limbo_poll) */
                std::lock_guard<std::mutex> g(slab_mu);
                if (!slab_limbo.empty()) limbo_poll(false);
                auto it = slab_free.lower_bound(need);
                if (it != slab_free.end() && it->first <= need + need / 4) {
                    *out = it->second;
                    if (Slab *sl = slab_of(it->second)) sl->live++;
                    slab_free.erase(it);
                    return true;
                }
            }
            if (!slab_cur || (size_t)(slab_end - slab_cur) < need) {
                void *sl = nullptr;
                double ms;
                if (timed_malloc(&sl, SLAB_BYTES, &ms) == hipSuccess) {
                    driver_ms += ms; driver_allocs++;
                    std::lock_guard<std::mutex> g(slab_mu);
                    /* what is left of the slab before it, as a free block (else it would be lost while one of its blocks lives) */
                    if (slab_cur && slab_end - slab_cur >= 256) {
                        slab_free.insert({(size_t)(slab_end - slab_cur) & ~(size_t)255, slab_cur});
                        slab_size[slab_cur] = (size_t)(slab_end - slab_cur) & ~(size_t)255;
                    }
                    slabs.push_back({(char *)sl, SLAB_BYTES, 0});
                    slab_cur = (char *)sl; slab_end = (char *)sl + SLAB_BYTES;
                } else (void)hipGetLastError(); /* no room for a slab: single blocks as before */
            }
            if (slab_cur && (size_t)(slab_end - slab_cur) >= need) {
                std::lock_guard<std::mutex> g(slab_mu);
                *out = slab_cur;
                slab_size[slab_cur] = need;
                if (Slab *sl = slab_of(slab_cur)) sl->live++;
                slab_cur += need;
                return true;
            }
        }
        double ms;
        hipError_t e = timed_malloc(out, bytes, &ms);
        driver_ms += ms; driver_allocs++;
        if (trace)
            fprintf(stderr, "ntl pool: hipMalloc %.1f MB -> %s in %.3f ms (cached %.1f MB of %.1f)\n", bytes / 1e6, e == hipSuccess ? "ok" : "FAILED",
                    ms, pool_bytes / 1e6, pool_cap / 1e6);
        return e == hipSuccess;
    }
    /* the slab a block lies in (slab_mu held), or NULL */
    Slab *slab_of(const void *p)
    {
        for (auto &sl : slabs)
            if ((const char *)p >= sl.base && (const char *)p < sl.base + sl.size) return &sl;
        return nullptr;
    }
    /* limbo blocks whose events have passed go onto the free list (wait: all of them, after waiting); slab_mu held */
    void limbo_poll(bool wait)
    {
        for (auto it = slab_limbo.begin(); it != slab_limbo.end();) {
            bool done = true;
            for (int i = 0; i < NSID && done; i++)
                if (it->ev[i]) {
                    const hipError_t q = wait ? hipEventSynchronize(it->ev[i]) : hipEventQuery(it->ev[i]);
                    if (q == hipErrorNotReady) done = false;
                }
            if (!done) { ++it; continue; }
            (void)hipGetLastError();
            for (int i = 0; i < NSID; i++) if (it->ev[i]) (void)hipEventDestroy(it->ev[i]);
            slab_free.insert({it->bytes, it->p});
            it = slab_limbo.erase(it);
        }
        (void)hipGetLastError(); /* (hipErrorNotReady is not an error) */
    }
};
