/*
 * Host side of libntlink_hip.so: the C ABI of include/ntlink_amd.h over the HIP kernels.
 * One context = one device + two streams (MAIN, and the window stage's unless NTL_PIPELINE=0) + the device block allocator
 * (dev_pool.h).  All launches are asynchronous; the host waits only where a caller asks for a count or a record of a handle that
 * the device has not finished yet.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <deque>
#include <map>
#include <unordered_map>
#include <mutex>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ntlink_amd.h"
#include "dev_common.h"
#include "dev_pool.h"
#include "pending.h"
#include "scan_kernels.h"
#include "sketch_kernels.h"
#include "sketch2_kernels.h"
#include "sketch_small_kernels.h"
#include "window_plan.h"
#include "map_kernels.h"
#include "group_kernels.h"
#include "gap_kernels.h"
#include "gap_select_kernels.h"
#include "pack_kernels.h"
#include "synth_kernels.h"
#include "mask_kernels.h"
#include "stitch_kernels.h"
#include "count_kernels.h"
#include "overlap_kernels.h"
#include "overlap_cut_kernels.h"
#include "path_kernels.h"
#include "format_kernels.h"
#include "sketch_text_kernels.h"
#include "liftover_kernels.h"
#include "pair_kernels.h"
#include "tally_view.h"

#define NTL_END_PAD 4096u /* bases of padding behind the last sequence (rolling over-reads) */
#define SK_NT 256
#define SK_NT_LONG 512 /* lanes of 16 k-mers of the 8192-ordinal strips (window_plan) */
#define NTL_MAX_W (16 * (SK_NT - 4) + 31) /* 16 k-mers per lane, a + 2 <= SK_NT - 2 halo lanes: w <= 4063 */

/* ------------------------------------------------------------------ context ------------- */

/*
 * Streams.  A context owns the MAIN stream (uploads, the emit / lookup / map / compaction kernels, downloads) and -- unless
 * NTL_PIPELINE=0 -- a second one for the WINDOW stage of a sketch (strip tables + the VALU-bound window kernels).  The window
 * stage of read batch i+1 depends on nothing the rest of batch i produces, so it is queued on its own stream and runs beside
 * batch i's latency-bound kernels; hipEvents carry the two real dependencies (window stage -> emit of the same batch; emit ->
 * the next user of the bitmask it read and cleared).  No call of the hot path waits on the host: sizes stay on the device,
 * result handles are completed lazily (sketch_finalize / mapres_finalize) when a count or a record is asked for.
 * A third stream for a sketch's preparation (the per-sequence tables, the strip scan, the strip table) was measured twice and
 * removed: the step got longer (profiles/HISTORY.md, profiles/r04_prep_stream.jsonl); those kernels run on the window stream.
 * The SIDE stream (NTL_SIDE_STREAM=1, with the pipeline on; not the default: DESIGN.md 4.6 has the measurement) takes what follows a sketch's first window kernel -- the
 * block-minima pass over the strips it gave up and the exact passes: about one strip in a hundred, needed only by the emit kernel of
 * the same sketch on MAIN -- so that the window kernels of consecutive sketches follow each other on the window stream with nothing
 * but the next sketch's preparation between them.  NTL_SIDE_STREAM=2 queues that preparation on the side stream too
 * (A/B: the side stream is one queue, so it then stands behind the previous sketch's passes).
 */
enum { SID_MAIN = 0, SID_W = 1, SID_S = 2, NTL_NSID = 3 };
static_assert(SID_MAIN == DevPool::MAIN && SID_W == DevPool::WINDOW && SID_S == DevPool::SIDE && NTL_NSID == DevPool::NSID, "the pool's stream ids are the context's");
static_assert(NTL_OK == DevPool::OK && NTL_ENOMEM == DevPool::NOMEM, "the pool's return codes are the C ABI's");

struct ProfEntry {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> spans;
    double done_ms = 0;
    uint64_t launches = 0;
};

/* a zero-filled minimizer bitmask whose last reader (emit_kernel) cleared what the window stage had set */
struct CleanMask {
    void *p = nullptr;
    size_t bytes = 0;
    hipEvent_t clean = nullptr; /* on MAIN: the clearing kernel has run */
};

struct ntl_ctx {
    int device = 0;
    hipStream_t stream = nullptr;  /* MAIN */
    hipStream_t wstream = nullptr; /* window stage; == stream when the pipeline is off */
    hipStream_t wstream_own = nullptr; /* the second stream itself (ntl_ctx_set_pipeline switches wstream between it and MAIN) */
    hipStream_t sstream = nullptr; /* side stream of the window stage's give-up passes; NULL while the pipeline is off, or without one */
    hipStream_t sstream_own = nullptr;
    bool side_prep = false;        /* NTL_SIDE_STREAM=2: a sketch's preparation on the side stream as well */
    bool pipelined = false;
    std::string err;
    std::string devname;
    int n_cu = 1;                  /* compute units of the device: the grid of a kernel whose wavefronts stay resident */
    std::map<const void *, int> occ; /* kernel -> workgroups one CU holds (hipOccupancyMaxActiveBlocksPerMultiprocessor, asked once) */
    bool prof = false;
    std::map<std::string, ProfEntry> profs;
    std::vector<hipEvent_t> ev_free;    /* timing events (profiling spans) */
    void *g4 = nullptr;                 /* device copy of the four-base init table */
    void *g8 = nullptr;                 /* device copy of the eight-base init table (1 MB) */
    std::map<int, void *> g8k;          /* k -> the two k-dependent ring forms of g8 the fast window pass reads (1 MB per k, sketch2_kernels.h) */
    DevPool mem;                        /* every device block of the context but the tables above (dev_pool.h) */
    std::deque<CleanMask> masks;
    void *host_tmp = nullptr;           /* page-locked bounce buffer for record downloads (grows, never shrinks) */
    size_t host_tmp_cap = 0;
    PinSlot *slots = nullptr;           /* the page-locked slots, and ... */
    PinSlot *dslots = nullptr;          /* ... device memory, one entry per slot: a map result's sums (MapSums), zero while the slot is free */
    PendingQueue pq;                    /* the slots, the ordering events and the handles destroyed before their work had run (pending.h) */
    hipEvent_t throttle[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    uint64_t n_enqueued = 0;            /* sketches queued so far: the host runs at most 8 of them ahead of the device */
    hipStream_t s(int sid) const { return sid == SID_S ? sstream : (sid == SID_W ? wstream : stream); }
    int sid(int want) const { return !pipelined ? SID_MAIN : (want == SID_S && !sstream ? SID_W : want); }
};
#define NTL_NSLOTS 512u

/* Page-locked host memory.  Large blocks are an anonymous mapping on 2-MB boundaries that asks for transparent huge pages and is then
 * registered with the runtime: 6.5 ms per 146-MB staging buffer against 33-38 ms for hipHostMalloc, same DMA rate (54 GB/s) --
 * tools/pin_bench.py, profiles/r04_pin_bench.txt; a process's first pass page-locks 1.4 GB of them.  Small blocks, and whatever the
 * mapping or the registration refuses: hipHostMalloc. */
#ifndef NTL_SIM
#include <sys/mman.h>
static std::mutex g_pin_mu;
static std::map<void *, std::pair<void *, size_t>> g_pin_maps; /* registered pointer -> (mapping, its length) */
#endif

static hipError_t pin_alloc(void **out, size_t bytes)
{
#ifndef NTL_SIM
    static const bool off = getenv("NTL_PIN_HOSTMALLOC") != nullptr; /* A/B */
    if (bytes >= ((size_t)4 << 20) && !off) {
        const size_t huge = (size_t)2 << 20, len = ((bytes + huge - 1) & ~(huge - 1)) + huge;
        void *base = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (base != MAP_FAILED) {
            void *p = (void *)(((uintptr_t)base + huge - 1) & ~(uintptr_t)(huge - 1));
            (void)madvise(p, len - huge, MADV_HUGEPAGE);
            if (hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess) {
                std::lock_guard<std::mutex> g(g_pin_mu);
                g_pin_maps[p] = {base, len};
                *out = p;
                return hipSuccess;
            }
            (void)hipGetLastError();
            munmap(base, len);
        }
    }
#endif
    return hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
}

static void pin_free(void *p)
{
    if (!p) return;
#ifndef NTL_SIM
    {
        std::unique_lock<std::mutex> g(g_pin_mu);
        auto it = g_pin_maps.find(p);
        if (it != g_pin_maps.end()) {
            const std::pair<void *, size_t> m = it->second;
            g_pin_maps.erase(it);
            g.unlock();
            (void)hipHostUnregister(p);
            munmap(m.first, m.second);
            return;
        }
    }
#endif
    (void)hipHostFree(p);
}

static int host_tmp(ntl_ctx *c, size_t bytes, void **out)
{
    if (c->host_tmp_cap < bytes) {
        if (c->host_tmp) pin_free(c->host_tmp);
        c->host_tmp = nullptr; c->host_tmp_cap = 0;
        const size_t cap = bytes + bytes / 4 + 4096;
        if (pin_alloc(&c->host_tmp, cap) != hipSuccess) {
            c->host_tmp = nullptr;
            c->err = "hipHostMalloc failed";
            return NTL_ENOMEM;
        }
        c->host_tmp_cap = cap;
    }
    *out = c->host_tmp;
    return NTL_OK;
}

static int fail(ntl_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg;
    return code;
}

#define HIPCHK(ctx, expr)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(ctx, NTL_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)

/* waits until everything queued on MAIN so far has finished -- on an event, so that the thread sleeps (hipStreamSynchronize
   spins for a while first) */
static hipError_t main_wait(ntl_ctx *c)
{
    hipEvent_t e = c->pq.event_get();
    if (!e) return hipStreamSynchronize(c->stream);
    hipError_t rc = hipEventRecord(e, c->stream);
    if (rc == hipSuccess) rc = hipEventSynchronize(e);
    c->pq.event_put(e);
    return rc;
}

/* A device buffer that returns to the context's block cache (dev_pool.h): the RAII handle over take / give.  touch() notes a second
 * stream that work on the buffer is queued on. */
struct DevBuf {
    ntl_ctx *c = nullptr;
    void *p = nullptr;
    size_t bytes = 0;
    mutable uint8_t used = 0; /* bit per stream id */
    DevBuf() {}
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    int alloc(ntl_ctx *ctx, size_t n, int sid = SID_MAIN)
    {
        release();
        c = ctx;
        sid = c->sid(sid);
        if (c->mem.take(n, sid, &p, &bytes) != DevPool::OK) { p = nullptr; bytes = 0; return fail(c, NTL_ENOMEM, "hipMalloc failed"); }
        used = (uint8_t)(1u << sid);
        return NTL_OK;
    }
    void touch(int sid) const { if (c) used |= (uint8_t)(1u << c->sid(sid)); }
    void release()
    {
        if (p && c) c->mem.give(p, bytes, used);
        p = nullptr; bytes = 0; used = 0;
    }
    ~DevBuf() { release(); }
    template <typename T> T *as() const { return (T *)p; }
};

struct ProfSpan {
    ntl_ctx *c;
    const char *name;
    hipStream_t st;
    hipEvent_t a = nullptr, b = nullptr;
    ProfSpan(ntl_ctx *ctx, const char *nm, int sid = SID_MAIN) : c(ctx), name(nm), st(ctx->s(sid))
    {
        if (!c->prof) return;
        auto get = [&](hipEvent_t &e) {
            if (!c->ev_free.empty()) { e = c->ev_free.back(); c->ev_free.pop_back(); }
            else if (hipEventCreate(&e) != hipSuccess) e = nullptr;
        };
        get(a); get(b);
        if (a) (void)hipEventRecord(a, st);
    }
    ~ProfSpan()
    {
        if (!c->prof || !a || !b) return;
        (void)hipEventRecord(b, st);
        ProfEntry &P = c->profs[name];
        P.spans.push_back({a, b});
        P.launches++;
    }
};

static void make_g4(uint64_t g4[256][2]);
static void make_g8(std::vector<uint64_t> &g8);

static void ctx_prime(ntl_ctx *c); /* behind the kernels' launch helpers */

extern "C" int ntl_ctx_create(int device, ntl_ctx **out)
{
    if (!out) return NTL_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return NTL_EDEVICE;
    ntl_ctx *c = new ntl_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete c; return NTL_EDEVICE; }
    /* NTL_PIPELINE=0: one stream, every kernel behind the previous one (what a per-kernel profile wants);
       NTL_PIPELINE_PRIO: 1 (default) the MAIN stream's short latency-bound kernels get free CU slots first, 2 the window
       stage does, 0 no priorities */
    c->pipelined = true;
    if (const char *e = getenv("NTL_PIPELINE")) c->pipelined = atoi(e) != 0;
    int prio = 1;
    if (const char *e = getenv("NTL_PIPELINE_PRIO")) prio = atoi(e);
    int least = 0, greatest = 0;
    if (!c->pipelined || prio == 0 || hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess || least == greatest) prio = 0;
    hipError_t e1 = prio ? hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio == 1 ? greatest : least)
                         : hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e1 != hipSuccess) { delete c; return NTL_EDEVICE; }
    c->wstream = c->stream;
    if (c->pipelined) {
        hipError_t e2 = prio ? hipStreamCreateWithPriority(&c->wstream, hipStreamNonBlocking, prio == 2 ? greatest : least)
                             : hipStreamCreateWithFlags(&c->wstream, hipStreamNonBlocking);
        if (e2 != hipSuccess) { c->wstream = c->stream; c->pipelined = false; }
        else c->wstream_own = c->wstream;
    }
    /* NTL_SIDE_STREAM: 1 the give-up passes of a sketch on a third stream, 2 its preparation too, 0 (default) everything on the
       window stream.  Off by default: measured on C3 the step is 0.3 ms shorter with it, inside the run-to-run spread */
    int side = 0;
    if (const char *e = getenv("NTL_SIDE_STREAM")) side = atoi(e);
    if (c->pipelined && side > 0) {
        /* its kernels are short and MAIN's emit kernel waits for them: MAIN's priority (NTL_SIDE_PRIO=0: the window stream's, A/B) */
        bool as_main = true;
        if (const char *e = getenv("NTL_SIDE_PRIO")) as_main = atoi(e) != 0;
        hipError_t e3 = prio ? hipStreamCreateWithPriority(&c->sstream, hipStreamNonBlocking, (prio == 2) != as_main ? greatest : least)
                             : hipStreamCreateWithFlags(&c->sstream, hipStreamNonBlocking);
        if (e3 != hipSuccess) { c->sstream = nullptr; (void)hipGetLastError(); }
        c->sstream_own = c->sstream;
        c->side_prep = side == 2;
    }
    {
        uint64_t g4[256][2];
        make_g4(g4);
        if (hipMalloc(&c->g4, sizeof g4) != hipSuccess || hipMemcpy(c->g4, g4, sizeof g4, hipMemcpyHostToDevice) != hipSuccess) {
            delete c;
            return NTL_EDEVICE;
        }
        std::vector<uint64_t> g8;
        make_g8(g8);
        if (hipMalloc(&c->g8, g8.size() * 8) != hipSuccess ||
            hipMemcpy(c->g8, g8.data(), g8.size() * 8, hipMemcpyHostToDevice) != hipSuccess) {
            delete c;
            return NTL_EDEVICE;
        }
        /* Kernels write the sizes and sums that come back to the host straight into the slots (ntl_host_store32/64): the slots are
           mapped into the device's address space and coherent (fine-grained: a device store goes to host memory, not into the
           device's L2), whatever HIP_HOST_COHERENT says -- hipHostMallocDefault leaves coherence to that variable. */
        PinSlot *slots_dev = nullptr; /* the same slots as the kernels address them */
#ifdef NTL_SIM
        if (hipHostMalloc((void **)&c->slots, NTL_NSLOTS * sizeof(PinSlot), hipHostMallocDefault) != hipSuccess) {
            delete c;
            return NTL_EDEVICE;
        }
        slots_dev = c->slots;
#else
        if (hipHostMalloc((void **)&c->slots, NTL_NSLOTS * sizeof(PinSlot), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            hipHostGetDevicePointer((void **)&slots_dev, c->slots, 0) != hipSuccess) {
            delete c;
            return NTL_EDEVICE;
        }
#endif
        if (hipMalloc((void **)&c->dslots, NTL_NSLOTS * sizeof(PinSlot)) != hipSuccess ||
            hipMemset(c->dslots, 0, NTL_NSLOTS * sizeof(PinSlot)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
            delete c;
            return NTL_EDEVICE;
        }
        uint32_t nslots = NTL_NSLOTS; /* NTL_NSLOTS (tests): fewer, so that a handful of handles reaches the bound */
        if (const char *e = getenv("NTL_NSLOTS")) nslots = (uint32_t)std::min<long>(NTL_NSLOTS, std::max<long>(2, atol(e)));
        c->pq.setup(c->slots, slots_dev, c->dslots, nslots, c);
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        size_t cache_bound = std::max<size_t>((size_t)prop.totalGlobalMem / 2, (size_t)256 << 20);
        if (const char *e = getenv("NTL_POOL_MAX_BYTES")) { const long long v = atoll(e); if (v >= 0) cache_bound = (size_t)v; }
#ifdef NTL_SIM
        const bool slabs = false; /* the mock's blocks stay single allocations: the CPU sanitizers see every array's ends */
#else
        const char *se = getenv("NTL_SLABS");
        const bool slabs = !se || atoi(se) != 0;
#endif
        c->mem.setup(c->stream, c->wstream, cache_bound, slabs, c->sstream);
        char buf[256];
        snprintf(buf, sizeof buf, "%s %s %d CUs %.0f GiB", prop.name, prop.gcnArchName, prop.multiProcessorCount,
                 (double)prop.totalGlobalMem / (1024.0 * 1024.0 * 1024.0));
        c->devname = buf;
        c->n_cu = prop.multiProcessorCount;
    }
    ctx_prime(c);
    *out = c;
    return NTL_OK;
}

static hipError_t sync_both(ntl_ctx *c)
{
    hipError_t e = hipStreamSynchronize(c->stream);
    if (c->wstream != c->stream) { const hipError_t e2 = hipStreamSynchronize(c->wstream); if (e == hipSuccess) e = e2; }
    if (c->sstream) { const hipError_t e3 = hipStreamSynchronize(c->sstream); if (e == hipSuccess) e = e3; }
    return e;
}

extern "C" void ntl_ctx_destroy(ntl_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)sync_both(c);
    c->pq.reap(true);
    for (auto &m : c->masks) { c->mem.free_uncached(m.p, m.bytes); c->pq.event_put(m.clean); }
    c->mem.destroy();
    (void)hipFree(c->g4);
    (void)hipFree(c->g8);
    for (auto &kv : c->g8k) (void)hipFree(kv.second);
    if (c->host_tmp) pin_free(c->host_tmp);
    if (c->slots) (void)hipHostFree(c->slots);
    if (c->dslots) (void)hipFree(c->dslots);
    for (auto &kv : c->profs)
        for (auto &sp : kv.second.spans) { (void)hipEventDestroy(sp.first); (void)hipEventDestroy(sp.second); }
    for (auto e : c->ev_free) (void)hipEventDestroy(e);
    for (auto &e : c->throttle) c->pq.event_put(e);
    c->pq.destroy();
    if (c->sstream_own) (void)hipStreamDestroy(c->sstream_own);
    if (c->wstream_own) (void)hipStreamDestroy(c->wstream_own);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" const char *ntl_last_error(const ntl_ctx *c) { return c ? c->err.c_str() : "no context"; }
extern "C" const char *ntl_ctx_device_name(const ntl_ctx *c) { return c ? c->devname.c_str() : ""; }
extern "C" int ntl_ctx_pipelined(const ntl_ctx *c) { return c && c->pipelined ? 1 : 0; }

/* Switches the window stage between its own stream and MAIN at a quiet point (both streams are drained first).  bench.py
 * times the pipelined steps, then a few serial ones whose per-kernel durations are those of kernels running alone. */
extern "C" int ntl_ctx_set_pipeline(ntl_ctx *c, int on)
{
    if (!c) return NTL_EINVAL;
    (void)hipSetDevice(c->device);
    HIPCHK(c, sync_both(c));
    c->pq.reap(true);
    if (on && !c->wstream_own) return fail(c, NTL_EINVAL, "this context was created without a window stream (NTL_PIPELINE=0)");
    c->pipelined = on != 0;
    c->wstream = on ? c->wstream_own : c->stream;
    c->sstream = on ? c->sstream_own : nullptr;
    c->mem.set_window_stream(c->wstream, c->sstream); /* (the streams were drained above: every cached block moves to MAIN's cache) */
    return NTL_OK;
}

/* 1 while the window stage's give-up passes are queued on the side stream (the pipeline is on and NTL_SIDE_STREAM was 1 or 2) */
extern "C" int ntl_ctx_side_stream(const ntl_ctx *c) { return c && c->pipelined && c->sstream ? 1 : 0; }

extern "C" int ntl_ctx_sync(ntl_ctx *c)
{
    if (!c) return NTL_EINVAL;
    (void)hipSetDevice(c->device);
    HIPCHK(c, sync_both(c));
    c->pq.reap(true);
    if (!c->pq.async_err.empty()) {
        const std::string m = c->pq.async_err;
        c->pq.async_err.clear();
        return fail(c, NTL_EINTERNAL, m);
    }
    return NTL_OK;
}

extern "C" int ntl_prof_enable(ntl_ctx *c, int on)
{
    if (!c) return NTL_EINVAL;
    c->prof = on != 0;
    return NTL_OK;
}

static void prof_collect(ntl_ctx *c)
{
    (void)sync_both(c);
    for (auto &kv : c->profs) {
        for (auto &sp : kv.second.spans) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, sp.first, sp.second) == hipSuccess) kv.second.done_ms += ms;
            c->ev_free.push_back(sp.first);
            c->ev_free.push_back(sp.second);
        }
        kv.second.spans.clear();
    }
}

extern "C" int ntl_prof_reset(ntl_ctx *c)
{
    if (!c) return NTL_EINVAL;
    prof_collect(c);
    for (auto &kv : c->profs) { kv.second.done_ms = 0; kv.second.launches = 0; }
    c->mem.driver_allocs = 0; c->mem.driver_ms = 0;
    return NTL_OK;
}

extern "C" int ntl_prof_get(ntl_ctx *c, const char *name, double *total_ms, uint64_t *launches)
{
    if (!c || !name) return NTL_EINVAL;
    prof_collect(c);
    if (!strcmp(name, "hipMalloc")) { /* host time of the block cache's misses, counted by the allocator itself */
        if (total_ms) *total_ms = c->mem.driver_ms;
        if (launches) *launches = c->mem.driver_allocs;
        return NTL_OK;
    }
    auto it = c->profs.find(name);
    if (total_ms) *total_ms = it == c->profs.end() ? 0.0 : it->second.done_ms;
    if (launches) *launches = it == c->profs.end() ? 0 : it->second.launches;
    return NTL_OK;
}

/* ------------------------------------------------------------------ scan helper ---------- */

/* `batch` independent exclusive scans of equal length in one set of launches: array y is in + y*(n+1) ->
 * out + y*(n+1), out[n] of each = its sum (arrays hold n+1 entries; in may equal out).  With total_host the
 * sums also come back to the host (one stream sync); without it nothing waits. */
static int device_scan(ntl_ctx *c, const uint32_t *in, uint32_t *out, uint64_t n, uint32_t *total_host, unsigned batch = 1,
                       uint32_t *sums_dev = nullptr, int sid = SID_MAIN)
{
    const uint64_t tiles = scan_tile_count(n);
    DevBuf tile;
    int rc;
    hipStream_t st = c->s(sid);
    if ((rc = tile.alloc(c, tiles * 4 * batch, sid))) return rc;
    scan_launch(st, in, out, n, batch, tile.as<uint32_t>(), sums_dev);
    HIPCHK(c, hipGetLastError());
    if (total_host) {
        for (unsigned y = 0; y < batch; y++)
            HIPCHK(c, hipMemcpyAsync(total_host + y, out + y * (n + 1) + n, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    return NTL_OK;
}

/* ------------------------------------------------------------------ batch ---------------- */

struct ntl_batch {
    ntl_ctx *c;
    std::atomic<int> refs{1}; /* the caller's + one per sketch that may still have to be redone from it (sketch_finalize) */
    uint64_t nseq = 0, bases = 0, nruns = 0, total_gpos = 0, nwords_packed = 0;
    bool any_multi = false; /* some sequence has more than one ACGT run */
    bool pure = false;      /* every sequence is one ACGT run from its first base to its last (so none is empty): decided where the
                               batch is made, read by ntl_batch_download and ntl_synth_slices */
    DevBuf packed, seq_base, seq_run_first, run_start, run_len;
    DevBuf seq_len_dev;             /* u32[nseq]: the `--len` column of the batch's sequences (unset where run_len already is that) */
    const uint32_t *d_seq_len = nullptr;
    std::vector<uint32_t> seq_len;
    /* a batch whose creating call returned without waiting (the synthetic ones): recorded on MAIN behind its last kernel;
       the window stream waits for it once */
    hipEvent_t ready = nullptr;
    mutable bool w_waited = false;
};

static void batch_unref(const ntl_batch *cb)
{
    ntl_batch *b = const_cast<ntl_batch *>(cb);
    if (b && --b->refs == 0) {
        (void)hipSetDevice(b->c->device);
        b->c->pq.event_put(b->ready);
        delete b;
    }
}

/* the window stage reads the batch on its own stream */
static void batch_on_wstream(ntl_ctx *c, const ntl_batch *b)
{
    if (!c->pipelined) return;
    if (b->ready && !b->w_waited) { (void)hipStreamWaitEvent(c->wstream, b->ready, 0); b->w_waited = true; }
    /* (the side stream's passes read it too, behind the window kernel -- so behind this wait; its preparation: sketch_prepare) */
    for (int sid : {(int)SID_W, (int)SID_S}) {
        b->packed.touch(sid); b->seq_base.touch(sid); b->seq_run_first.touch(sid); b->run_start.touch(sid); b->run_len.touch(sid);
    }
}

/* a batch of nseq sequences and `bases` bases whose packed stream spans `span` positions behind the lead pad */
static std::unique_ptr<ntl_batch> batch_new(ntl_ctx *c, uint64_t nseq, uint64_t bases, uint64_t span)
{
    std::unique_ptr<ntl_batch> b(new ntl_batch());
    b->c = c; b->nseq = nseq; b->bases = bases;
    b->total_gpos = NTL_LEAD_PAD + span;
    b->nwords_packed = (NTL_LEAD_PAD + span + NTL_END_PAD + 15) / 16 + 2;
    return b;
}

/* the `--len` column on the device, from b->seq_len (queued on MAIN: b->seq_len outlives the copy) */
static int batch_upload_seq_len(ntl_ctx *c, ntl_batch *b)
{
    int rc;
    if ((rc = b->seq_len_dev.alloc(c, (b->nseq + 1) * 4))) return rc;
    if (b->nseq) HIPCHK(c, hipMemcpyAsync(b->seq_len_dev.p, b->seq_len.data(), b->nseq * 4, hipMemcpyHostToDevice, c->stream));
    b->d_seq_len = b->seq_len_dev.as<uint32_t>();
    return NTL_OK;
}

/* the device tables of a batch that arrives packed with its run tables: allocated, uploaded and waited for (the caller's arrays are free again) */
static int batch_upload_packed(ntl_ctx *c, ntl_batch *b, const uint32_t *packed, const std::vector<uint64_t> &seq_base,
                               const uint32_t *seq_run_first, const uint32_t *run_start, const uint32_t *run_len)
{
    const uint64_t nseq = b->nseq, nruns = b->nruns;
    int rc;
    (void)hipSetDevice(c->device);
    if ((rc = b->packed.alloc(c, b->nwords_packed * 4)) || (rc = b->seq_base.alloc(c, (nseq + 1) * 8)) ||
        (rc = b->seq_run_first.alloc(c, (nseq + 1) * 4)) || (rc = b->run_start.alloc(c, (nruns + 1) * 4)) ||
        (rc = b->run_len.alloc(c, (nruns + 1) * 4)))
        return rc;
    {
        ProfSpan span(c, "batch_pack");
        HIPCHK(c, hipMemcpyAsync(b->packed.p, packed, b->nwords_packed * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(b->seq_base.p, seq_base.data(), (nseq + 1) * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(b->seq_run_first.p, seq_run_first, (nseq + 1) * 4, hipMemcpyHostToDevice, c->stream));
        if ((rc = batch_upload_seq_len(c, b))) return rc;
        if (nruns) {
            HIPCHK(c, hipMemcpyAsync(b->run_start.p, run_start, nruns * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(b->run_len.p, run_len, nruns * 4, hipMemcpyHostToDevice, c->stream));
        }
    }
    HIPCHK(c, main_wait(c));
    return NTL_OK;
}

/* Host arrays in, device layout out: the bases travel as they are (one byte each) and are packed and
 * scanned for ACGT runs on the device (pack_kernels.h).  Pinned memory from ntl_host_alloc makes the
 * copy a single DMA; anything else goes through the runtime's staging buffers. */
extern "C" int ntl_batch_create(ntl_ctx *c, const char *seqs, const uint64_t *off, uint64_t nseq, ntl_batch **out)
{
    if (!c || !out || (!seqs && nseq) || !off) return NTL_EINVAL;
    *out = nullptr;
    if (nseq >= ((uint64_t)1 << 31)) return fail(c, NTL_EINVAL, "too many sequences in one batch");
    for (uint64_t i = 0; i < nseq; i++) {
        if (off[i + 1] < off[i]) return fail(c, NTL_EINVAL, "offsets must be non-decreasing");
        if (off[i + 1] - off[i] >= 0xFFFFFFF0ull) return fail(c, NTL_EINVAL, "sequence longer than 2^32 bases");
    }
    const uint64_t o0 = nseq ? off[0] : 0;
    const uint64_t total = nseq ? off[nseq] - o0 : 0;
    std::unique_ptr<ntl_batch> b = batch_new(c, nseq, total, total);
    const uint64_t nwords = b->nwords_packed;
    std::vector<uint64_t> seq_base(nseq + 1);
    b->seq_len.resize(nseq);
    for (uint64_t i = 0; i <= nseq; i++) seq_base[i] = NTL_LEAD_PAD + ((i < nseq ? off[i] : off[nseq]) - o0);
    for (uint64_t i = 0; i < nseq; i++) b->seq_len[i] = (uint32_t)(off[i + 1] - off[i]);

    const uint64_t n32 = (NTL_LEAD_PAD + total + 31) / 32; /* threads = 32-position groups that hold data */
    int rc;
    (void)hipSetDevice(c->device);
    DevBuf raw, valid32, ss32, starts32, rank, flags;
    if ((rc = b->packed.alloc(c, nwords * 4)) || (rc = b->seq_base.alloc(c, (nseq + 1) * 8)) ||
        (rc = b->seq_run_first.alloc(c, (nseq + 1) * 4)) || (rc = raw.alloc(c, total + 64)) ||
        (rc = valid32.alloc(c, (n32 + 2) * 4)) || (rc = ss32.alloc(c, (n32 + 2) * 4)) ||
        (rc = starts32.alloc(c, (n32 + 2) * 4)) || (rc = rank.alloc(c, (n32 + 2) * 4)) || (rc = flags.alloc(c, 4)))
        return rc;
    uint32_t nruns = 0, seen = 0;
    DevBuf start_g, end_g;
    {
    ProfSpan span(c, "batch_pack");
    if (total) HIPCHK(c, hipMemcpyAsync(raw.p, seqs + o0, total, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b->seq_base.p, seq_base.data(), (nseq + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if ((rc = batch_upload_seq_len(c, b.get()))) return rc;
    HIPCHK(c, hipMemsetAsync(b->packed.p, 0, nwords * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(valid32.p, 0, (n32 + 2) * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(ss32.p, 0, (n32 + 2) * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(starts32.p, 0, (n32 + 2) * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(rank.p, 0, (n32 + 2) * 4, c->stream)); /* counts; scanned in place */
    HIPCHK(c, hipMemsetAsync(flags.p, 0, 4, c->stream));
    const unsigned g32 = (unsigned)((n32 + PACK_NT - 1) / PACK_NT);
    const unsigned gseq = (unsigned)((nseq + 1 + PACK_NT - 1) / PACK_NT);
    if (n32) {
        hipLaunchKernelGGL(pack_kernel, dim3(g32), dim3(PACK_NT), 0, c->stream, raw.as<uint8_t>(), total, b->packed.as<uint32_t>(),
                           valid32.as<uint32_t>(), n32);
        hipLaunchKernelGGL(seq_mark_kernel, dim3(gseq), dim3(PACK_NT), 0, c->stream, b->seq_base.as<uint64_t>(), (uint32_t)nseq,
                           ss32.as<uint32_t>());
        hipLaunchKernelGGL(run_count_kernel, dim3(g32), dim3(PACK_NT), 0, c->stream, valid32.as<uint32_t>(), ss32.as<uint32_t>(), n32,
                           starts32.as<uint32_t>(), rank.as<uint32_t>());
        HIPCHK(c, hipGetLastError());
    }
    /* n32 + 1 counts (the last is the zero padding word) so that rank[n32] exists for seq_base[nseq] */
    if ((rc = device_scan(c, rank.as<uint32_t>(), rank.as<uint32_t>(), n32 + 1, &nruns))) return rc;
    if (nruns >= 0xFFFFFFF0u) return fail(c, NTL_EINVAL, "too many ACGT runs in one batch");
    b->nruns = nruns;
    if ((rc = b->run_start.alloc(c, ((uint64_t)nruns + 1) * 4)) || (rc = b->run_len.alloc(c, ((uint64_t)nruns + 1) * 4)) ||
        (rc = start_g.alloc(c, ((uint64_t)nruns + 1) * 8)) || (rc = end_g.alloc(c, ((uint64_t)nruns + 1) * 8)))
        return rc;
    if (nruns) {
        hipLaunchKernelGGL(run_fill_kernel, dim3(g32), dim3(PACK_NT), 0, c->stream, valid32.as<uint32_t>(), ss32.as<uint32_t>(),
                           starts32.as<uint32_t>(), rank.as<uint32_t>(), n32, start_g.as<uint64_t>(), end_g.as<uint64_t>());
        hipLaunchKernelGGL(run_finish_kernel, dim3((nruns + PACK_NT - 1) / PACK_NT), dim3(PACK_NT), 0, c->stream, start_g.as<uint64_t>(),
                           end_g.as<uint64_t>(), nruns, b->seq_base.as<uint64_t>(), (uint32_t)nseq, b->run_start.as<uint32_t>(),
                           b->run_len.as<uint32_t>());
    }
    hipLaunchKernelGGL(seq_runs_kernel, dim3(gseq), dim3(PACK_NT), 0, c->stream, starts32.as<uint32_t>(), rank.as<uint32_t>(),
                       b->seq_base.as<uint64_t>(), (uint32_t)nseq, b->run_len.as<uint32_t>(), b->seq_run_first.as<uint32_t>(),
                       flags.as<uint32_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(&seen, flags.p, 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream)); /* the caller's arrays and seq_base are free again */
    b->any_multi = (seen & SEQ_RUNS_MULTI) != 0;
    b->pure = (seen & SEQ_RUNS_IMPURE) == 0;
    *out = b.release();
    return NTL_OK;
}

/* ntl_batch::pure of a run table that arrives from the host (seq_run_first checked: non-decreasing, ends at the run count) */
static bool host_runs_pure(const uint32_t *len, uint64_t nseq, const uint32_t *seq_run_first, const uint32_t *run_len)
{
    for (uint64_t i = 0; i < nseq; i++)
        if (seq_run_first[i + 1] - seq_run_first[i] != 1u || run_len[seq_run_first[i]] != len[i]) return false;
    return true;
}

/* The same batch from bases that are already packed (ntl_fastx_copy_packed + ntl_fastx_runs: the parser threads pack
 * while they copy): a quarter of the bytes cross PCIe and the pack / run-table kernels are not needed. */
extern "C" int ntl_batch_create_packed(ntl_ctx *c, const uint32_t *packed, const uint64_t *off, uint64_t nseq,
                                       const uint32_t *seq_run_first, const uint32_t *run_start, const uint32_t *run_len,
                                       uint64_t nruns, ntl_batch **out)
{
    if (!c || !out || !packed || !off || !seq_run_first || (nruns && (!run_start || !run_len))) return NTL_EINVAL;
    *out = nullptr;
    if (nseq >= ((uint64_t)1 << 31)) return fail(c, NTL_EINVAL, "too many sequences in one batch");
    if (nruns >= 0xFFFFFFF0ull) return fail(c, NTL_EINVAL, "too many ACGT runs in one batch");
    if (off[0] != 0) return fail(c, NTL_EINVAL, "offsets[0] must be 0 for a packed batch");
    std::unique_ptr<ntl_batch> b = batch_new(c, nseq, off[nseq], off[nseq]);
    b->seq_len.resize(nseq);
    std::vector<uint64_t> seq_base(nseq + 1);
    bool multi = false;
    for (uint64_t i = 0; i < nseq; i++) {
        if (off[i + 1] < off[i]) return fail(c, NTL_EINVAL, "offsets must be non-decreasing");
        if (off[i + 1] - off[i] >= 0xFFFFFFF0ull) return fail(c, NTL_EINVAL, "sequence longer than 2^32 bases");
        if (seq_run_first[i + 1] < seq_run_first[i]) return fail(c, NTL_EINVAL, "seq_run_first must be non-decreasing");
        multi |= seq_run_first[i + 1] - seq_run_first[i] > 1u;
        b->seq_len[i] = (uint32_t)(off[i + 1] - off[i]);
        seq_base[i] = NTL_LEAD_PAD + off[i];
    }
    if (seq_run_first[0] != 0 || seq_run_first[nseq] != nruns) return fail(c, NTL_EINVAL, "seq_run_first does not match the run count");
    seq_base[nseq] = NTL_LEAD_PAD + off[nseq];
    b->nruns = nruns; b->any_multi = multi;
    b->pure = host_runs_pure(b->seq_len.data(), nseq, seq_run_first, run_len);
    if (int rc = batch_upload_packed(c, b.get(), packed, seq_base, seq_run_first, run_start, run_len)) return rc;
    *out = b.release();
    return NTL_OK;
}

/* The same from a packed stream in which the sequences need not be contiguous (ntl_fastx_parse_span: a one-pass reader puts
 * every parser thread's sequences at an upper bound of their place): sequence i = lengths[i] bases from base position
 * positions[i] of the stream (non-decreasing, non-overlapping), which spans span_positions positions in all; the words between
 * sequences are never interpreted. */
extern "C" int ntl_batch_create_packed_at(ntl_ctx *c, const uint32_t *packed, uint64_t span_positions, const uint64_t *positions,
                                          const uint32_t *lengths, uint64_t nseq, const uint32_t *seq_run_first, const uint32_t *run_start,
                                          const uint32_t *run_len, uint64_t nruns, ntl_batch **out)
{
    if (!c || !out || !packed || (nseq && (!positions || !lengths)) || !seq_run_first || (nruns && (!run_start || !run_len))) return NTL_EINVAL;
    *out = nullptr;
    if (nseq >= ((uint64_t)1 << 31)) return fail(c, NTL_EINVAL, "too many sequences in one batch");
    if (nruns >= 0xFFFFFFF0ull) return fail(c, NTL_EINVAL, "too many ACGT runs in one batch");
    if (span_positions >= 0xFFFFFFF0ull - NTL_END_PAD) return fail(c, NTL_EINVAL, "packed stream longer than 2^32 positions");
    std::vector<uint64_t> seq_base(nseq + 1);
    bool multi = false;
    uint64_t total = 0, prev_end = 0;
    for (uint64_t i = 0; i < nseq; i++) {
        if (positions[i] < prev_end || positions[i] + lengths[i] > span_positions) return fail(c, NTL_EINVAL, "sequence positions must be non-overlapping, in order and inside the stream");
        if (seq_run_first[i + 1] < seq_run_first[i]) return fail(c, NTL_EINVAL, "seq_run_first must be non-decreasing");
        multi |= seq_run_first[i + 1] - seq_run_first[i] > 1u;
        seq_base[i] = NTL_LEAD_PAD + positions[i];
        prev_end = positions[i] + lengths[i];
        total += lengths[i];
    }
    if (seq_run_first[0] != 0 || seq_run_first[nseq] != nruns) return fail(c, NTL_EINVAL, "seq_run_first does not match the run count");
    seq_base[nseq] = NTL_LEAD_PAD + span_positions;
    std::unique_ptr<ntl_batch> b = batch_new(c, nseq, total, span_positions);
    b->seq_len.assign(lengths, lengths + nseq);
    b->nruns = nruns; b->any_multi = multi;
    b->pure = host_runs_pure(lengths, nseq, seq_run_first, run_len);
    if (int rc = batch_upload_packed(c, b.get(), packed, seq_base, seq_run_first, run_start, run_len)) return rc;
    *out = b.release();
    return NTL_OK;
}

extern "C" void ntl_batch_destroy(ntl_batch *b) { batch_unref(b); }

extern "C" int ntl_host_alloc(ntl_ctx *c, uint64_t bytes, void **out)
{
    if (!c || !out) return NTL_EINVAL;
    *out = nullptr;
    (void)hipSetDevice(c->device);
    HIPCHK(c, pin_alloc(out, bytes));
    return NTL_OK;
}

extern "C" void ntl_host_free(ntl_ctx *c, void *p)
{
    if (!c || !p) return;
    (void)hipSetDevice(c->device);
    pin_free(p);
}
extern "C" uint64_t ntl_batch_nseq(const ntl_batch *b) { return b ? b->nseq : 0; }
extern "C" uint64_t ntl_batch_bases(const ntl_batch *b) { return b ? b->bases : 0; }

/* ------------------------------------------------------------------ synthetic batches ----- */

/* device layout of a batch whose sequences are pure ACGT: every sequence is one run */
static int synth_layout(ntl_ctx *c, const uint32_t *len, uint64_t nseq, std::unique_ptr<ntl_batch> &b, std::vector<uint64_t> &seq_base)
{
    if (nseq >= ((uint64_t)1 << 31)) return fail(c, NTL_EINVAL, "too many sequences in one batch");
    seq_base.resize(nseq + 1);
    uint64_t total = 0;
    for (uint64_t i = 0; i < nseq; i++) {
        if (len[i] == 0 || len[i] >= 0xFFFFFFF0u) return fail(c, NTL_EINVAL, "synthetic sequences must hold 1..2^32-17 bases");
        seq_base[i] = NTL_LEAD_PAD + total;
        total += len[i];
    }
    seq_base[nseq] = NTL_LEAD_PAD + total;
    b = batch_new(c, nseq, total, total);
    b->seq_len.assign(len, len + nseq);
    b->nruns = nseq;
    b->pure = true;
    int rc;
    if ((rc = b->packed.alloc(c, b->nwords_packed * 4)) || (rc = b->seq_base.alloc(c, (nseq + 1) * 8)) ||
        (rc = b->seq_run_first.alloc(c, (nseq + 1) * 4)) || (rc = b->run_start.alloc(c, (nseq + 1) * 4)) ||
        (rc = b->run_len.alloc(c, (nseq + 1) * 4)))
        return rc;
    std::vector<uint32_t> iota(nseq + 1);
    for (uint64_t i = 0; i <= nseq; i++) iota[i] = (uint32_t)i;
    HIPCHK(c, hipMemcpyAsync(b->seq_base.p, seq_base.data(), (nseq + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b->seq_run_first.p, iota.data(), (nseq + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(b->run_start.p, 0, (nseq + 1) * 4, c->stream));
    if (nseq) HIPCHK(c, hipMemcpyAsync(b->run_len.p, len, nseq * 4, hipMemcpyHostToDevice, c->stream));
    b->d_seq_len = b->run_len.as<uint32_t>(); /* one run per sequence: the run lengths are the sequence lengths */
    HIPCHK(c, hipStreamSynchronize(c->stream)); /* iota and seq_base are stack/host temporaries */
    return NTL_OK;
}

extern "C" int ntl_synth_genome(ntl_ctx *c, uint64_t seed, const uint32_t *len, uint64_t nseq, ntl_batch **out)
{
    if (!c || !out || (!len && nseq)) return NTL_EINVAL;
    *out = nullptr;
    (void)hipSetDevice(c->device);
    std::unique_ptr<ntl_batch> b;
    std::vector<uint64_t> seq_base;
    int rc = synth_layout(c, len, nseq, b, seq_base);
    if (rc) return rc;
    const uint64_t nw = b->nwords_packed;
    hipLaunchKernelGGL(synth_genome_kernel, dim3((unsigned)((nw / 2 + 256) / 256)), dim3(256), 0, c->stream, b->packed.as<uint32_t>(), nw, seed);
    HIPCHK(c, hipGetLastError());
    if (c->pipelined && (b->ready = c->pq.event_get())) HIPCHK(c, hipEventRecord(b->ready, c->stream));
    *out = b.release();
    return NTL_OK;
}

extern "C" int ntl_synth_slices(ntl_ctx *c, const ntl_batch *src, uint64_t seed, uint64_t n, const uint32_t *src_seq,
                                const uint32_t *src_start, const uint32_t *out_len, const uint8_t *reverse,
                                double sub, double ins, double del, ntl_batch **out)
{
    if (!c || !src || !out || (n && (!src_seq || !src_start || !out_len))) return NTL_EINVAL;
    *out = nullptr;
    if (!src->pure) return fail(c, NTL_EINVAL, "the source batch must be pure ACGT");
    if (sub < 0 || ins < 0 || del < 0 || sub > 0.5 || ins + del > 0.5) return fail(c, NTL_EINVAL, "error rates out of range");
    const bool errors = sub > 0 || ins > 0 || del > 0;
    for (uint64_t i = 0; i < n; i++) {
        if (src_seq[i] >= src->nseq) return fail(c, NTL_EINVAL, "source sequence index out of range");
        const uint64_t need = errors ? synth_span(out_len[i]) : (uint64_t)out_len[i];
        if ((uint64_t)src_start[i] + need > src->seq_len[src_seq[i]]) return fail(c, NTL_EINVAL, "slice does not fit its source sequence");
    }
    (void)hipSetDevice(c->device);
    std::unique_ptr<ntl_batch> b;
    std::vector<uint64_t> seq_base;
    int rc = synth_layout(c, out_len, n, b, seq_base);
    if (rc) return rc;
    DevBuf d_seq, d_start, d_rev;
    if ((rc = d_seq.alloc(c, (n + 1) * 4)) || (rc = d_start.alloc(c, (n + 1) * 4)) || (rc = d_rev.alloc(c, n + 1))) return rc;
    HIPCHK(c, hipMemsetAsync(b->packed.p, 0, b->nwords_packed * 4, c->stream));
    if (n) {
        HIPCHK(c, hipMemcpyAsync(d_seq.p, src_seq, n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_start.p, src_start, n * 4, hipMemcpyHostToDevice, c->stream));
        if (reverse) HIPCHK(c, hipMemcpyAsync(d_rev.p, reverse, n, hipMemcpyHostToDevice, c->stream));
        SliceArgs A;
        A.src_packed = src->packed.as<uint32_t>(); A.src_seq_base = src->seq_base.as<uint64_t>(); A.n_src = (uint32_t)src->nseq;
        A.dst_packed = b->packed.as<uint32_t>(); A.dst_seq_base = b->seq_base.as<uint64_t>();
        A.src_seq = d_seq.as<uint32_t>(); A.src_start = d_start.as<uint32_t>(); A.reverse = reverse ? d_rev.as<uint8_t>() : nullptr;
        A.n = n; A.seed = seed;
        const double S = 16777216.0; /* 24-bit draws */
        A.t_ins = (uint32_t)(ins * S); A.t_del = (uint32_t)((ins + del) * S); A.t_sub = (uint32_t)(sub * S);
        if (errors && A.t_del == 0 && A.t_sub == 0) A.t_sub = 1; /* keeps the error path (and its source span) selected */
        hipLaunchKernelGGL(synth_slices_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, A);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipStreamSynchronize(c->stream)); /* the caller's arrays are free again */
    *out = b.release();
    return NTL_OK;
}

extern "C" int ntl_batch_download(const ntl_batch *b, char *seqs, uint64_t *off)
{
    if (!b || (!seqs && b->bases) || !off) return NTL_EINVAL;
    ntl_ctx *c = b->c;
    if (!b->pure) return fail(c, NTL_EINVAL, "only pure-ACGT batches can be downloaded");
    (void)hipSetDevice(c->device);
    uint64_t t = 0;
    for (uint64_t i = 0; i < b->nseq; i++) { off[i] = t; t += b->seq_len[i]; }
    off[b->nseq] = t;
    if (t != b->bases) return fail(c, NTL_EINVAL, "only pure-ACGT batches can be downloaded");
    const uint64_t CH = (uint64_t)1 << 28; /* 256 Mbases of ASCII per piece */
    DevBuf tmp;
    int rc = tmp.alloc(c, std::min<uint64_t>(CH, b->bases) + 16);
    if (rc) return rc;
    for (uint64_t p0 = 0; p0 < b->bases; p0 += CH) {
        const uint64_t m = std::min<uint64_t>(CH, b->bases - p0);
        hipLaunchKernelGGL(unpack_kernel, dim3((unsigned)((m / 16 + 256) / 256)), dim3(256), 0, c->stream,
                           (const uint32_t *)b->packed.as<uint32_t>(), (uint64_t)NTL_LEAD_PAD + p0, m, tmp.as<uint8_t>());
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(seqs + p0, tmp.p, m, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return NTL_OK;
}

/* ------------------------------------------------------------------ masked copies --------- */

/* N-masked full-length copies of resident records (mask_kernels.h; print_masked_sequences of the reference,
 * bin/ntlink_patch_gaps.py:346-389, without its two files).  Waits for the device before it returns: the number of runs comes back
 * to the host for the run tables' size in the middle of it, and the caller's arrays are free afterwards. */
extern "C" int ntl_batch_mask(ntl_ctx *c, const ntl_batch *src, uint64_t n, const uint32_t *src_seq, const uint32_t *keep_lo,
                              const uint32_t *keep_hi, ntl_batch **out)
{
    if (!c || !src || !out || (n && (!src_seq || !keep_lo || !keep_hi))) return NTL_EINVAL;
    *out = nullptr;
    if (n >= ((uint64_t)1 << 31)) return fail(c, NTL_EINVAL, "too many sequences in one batch");
    std::vector<uint64_t> seq_base(n + 1);
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (src_seq[i] >= src->nseq)
            return fail(c, NTL_EINVAL, "record " + std::to_string(i) + ": source sequence index " + std::to_string(src_seq[i]) + " out of range (" +
                                       std::to_string(src->nseq) + " sequences)");
        if (keep_lo[i] > keep_hi[i])
            return fail(c, NTL_EINVAL, "record " + std::to_string(i) + ": keep_lo " + std::to_string(keep_lo[i]) + " is above keep_hi " +
                                       std::to_string(keep_hi[i]));
        if (keep_hi[i] > src->seq_len[src_seq[i]])
            return fail(c, NTL_EINVAL, "record " + std::to_string(i) + ": keep_hi " + std::to_string(keep_hi[i]) + " is beyond the source sequence's " +
                                       std::to_string(src->seq_len[src_seq[i]]) + " bases");
        seq_base[i] = NTL_LEAD_PAD + total;
        total += src->seq_len[src_seq[i]];
    }
    seq_base[n] = NTL_LEAD_PAD + total;
    if (total >= 0xFFFFFFF0ull - NTL_END_PAD) return fail(c, NTL_EINVAL, "masked batch longer than 2^32 positions");
    (void)hipSetDevice(c->device);
    std::unique_ptr<ntl_batch> b = batch_new(c, n, total, total);
    b->seq_len.resize(n);
    for (uint64_t i = 0; i < n; i++) b->seq_len[i] = src->seq_len[src_seq[i]];
    int rc;
    DevBuf d_seq, d_lo, d_hi, d_first, d_stats;
    if ((rc = b->packed.alloc(c, b->nwords_packed * 4)) || (rc = b->seq_base.alloc(c, (n + 1) * 8)) ||
        (rc = b->seq_run_first.alloc(c, (n + 1) * 4)) || (rc = d_seq.alloc(c, (n + 1) * 4)) || (rc = d_lo.alloc(c, (n + 1) * 4)) ||
        (rc = d_hi.alloc(c, (n + 1) * 4)) || (rc = d_first.alloc(c, (n + 1) * 4)) || (rc = d_stats.alloc(c, 16)))
        return rc;
    if (src->ready) HIPCHK(c, hipStreamWaitEvent(c->stream, src->ready, 0));
    MaskArgs A;
    A.src_packed = src->packed.as<uint32_t>(); A.src_seq_base = src->seq_base.as<uint64_t>();
    A.src_seq_run_first = src->seq_run_first.as<uint32_t>(); A.src_run_start = src->run_start.as<uint32_t>();
    A.src_run_len = src->run_len.as<uint32_t>(); A.n_src = (uint32_t)src->nseq;
    A.src_seq = d_seq.as<uint32_t>(); A.keep_lo = d_lo.as<uint32_t>(); A.keep_hi = d_hi.as<uint32_t>(); A.n = n;
    A.dst_packed = b->packed.as<uint32_t>(); A.dst_seq_base = b->seq_base.as<uint64_t>();
    A.cnt = b->seq_run_first.as<uint32_t>(); A.first = d_first.as<uint32_t>(); A.dst_seq_run_first = b->seq_run_first.as<uint32_t>();
    A.dst_run_start = nullptr; A.dst_run_len = nullptr; A.stats = d_stats.as<unsigned long long>();
    const unsigned g_lane = (unsigned)((n + MASK_NT - 1) / MASK_NT), g_wave = (unsigned)((n + MASK_NT / 64 - 1) / (MASK_NT / 64));
    unsigned long long stats[2] = {0, 0};
    {
        ProfSpan span(c, "batch_mask");
        HIPCHK(c, hipMemcpyAsync(b->seq_base.p, seq_base.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
        if ((rc = batch_upload_seq_len(c, b.get()))) return rc;
        HIPCHK(c, hipMemsetAsync(b->packed.p, 0, b->nwords_packed * 4, c->stream));
        HIPCHK(c, hipMemsetAsync(b->seq_run_first.p, 0, (n + 1) * 4, c->stream)); /* counts; scanned in place */
        HIPCHK(c, hipMemsetAsync(d_stats.p, 0, 16, c->stream));
        if (n) {
            HIPCHK(c, hipMemcpyAsync(d_seq.p, src_seq, n * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(d_lo.p, keep_lo, n * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(d_hi.p, keep_hi, n * 4, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(nmask_count_kernel, dim3(g_lane), dim3(MASK_NT), 0, c->stream, A);
            hipLaunchKernelGGL(nmask_copy_kernel, dim3(g_wave), dim3(MASK_NT), 0, c->stream, A);
            HIPCHK(c, hipGetLastError());
        }
        if ((rc = device_scan(c, b->seq_run_first.as<uint32_t>(), b->seq_run_first.as<uint32_t>(), n, nullptr))) return rc;
        HIPCHK(c, hipMemcpyAsync(stats, d_stats.p, 16, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream)); /* the run count: the size of the run tables */
    if (stats[0] >= 0xFFFFFFF0ull) return fail(c, NTL_EINVAL, "too many ACGT runs in one batch");
    b->nruns = stats[0];
    b->any_multi = (stats[1] & NMASK_MULTI) != 0;
    b->pure = (stats[1] & NMASK_IMPURE) == 0;
    if ((rc = b->run_start.alloc(c, (b->nruns + 1) * 4)) || (rc = b->run_len.alloc(c, (b->nruns + 1) * 4))) return rc;
    if (b->nruns) {
        ProfSpan span(c, "batch_mask");
        A.dst_run_start = b->run_start.as<uint32_t>(); A.dst_run_len = b->run_len.as<uint32_t>();
        hipLaunchKernelGGL(nmask_fill_kernel, dim3(g_lane), dim3(MASK_NT), 0, c->stream, A);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipStreamSynchronize(c->stream)); /* the temporaries go back to the block cache; the caller's arrays are free again */
    *out = b.release();
    return NTL_OK;
}

/* ntl_batch_download for any batch: upper-case ASCII with N wherever no run covers a base */
extern "C" int ntl_batch_download_n(const ntl_batch *b, char *seqs, uint64_t *off)
{
    if (!b || (!seqs && b->bases) || !off) return NTL_EINVAL;
    ntl_ctx *c = b->c;
    (void)hipSetDevice(c->device);
    uint64_t t = 0;
    for (uint64_t i = 0; i < b->nseq; i++) { off[i] = t; t += b->seq_len[i]; }
    off[b->nseq] = t;
    if (t == 0) return NTL_OK;
    DevBuf tmp, d_off;
    int rc;
    if ((rc = tmp.alloc(c, t + 16)) || (rc = d_off.alloc(c, (b->nseq + 1) * 8))) return rc;
    if (b->ready) HIPCHK(c, hipStreamWaitEvent(c->stream, b->ready, 0));
    HIPCHK(c, hipMemsetAsync(tmp.p, 'N', t, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_off.p, off, (b->nseq + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (b->nruns) {
        hipLaunchKernelGGL(unpack_runs_kernel, dim3((unsigned)((b->nruns + MASK_NT / 64 - 1) / (MASK_NT / 64))), dim3(MASK_NT), 0, c->stream,
                           (const uint32_t *)b->packed.as<uint32_t>(), (const uint64_t *)b->seq_base.as<uint64_t>(),
                           (const uint32_t *)b->seq_run_first.as<uint32_t>(), (uint32_t)b->nseq, (const uint32_t *)b->run_start.as<uint32_t>(),
                           (const uint32_t *)b->run_len.as<uint32_t>(), (uint64_t)b->nruns, (const uint64_t *)d_off.as<uint64_t>(),
                           tmp.as<uint8_t>());
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(seqs, tmp.p, t, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return NTL_OK;
}

/* ------------------------------------------------------------------ resident bytes, the stitch ---------- */

/* Records resident as the bytes they were read as (a batch keeps neither lower case nor IUPAC codes): the sources of ntl_stitch. */
struct ntl_ascii {
    ntl_ctx *c;
    std::vector<uint64_t> off; /* [nrec + 1], from 0 */
    DevBuf bytes;
};

extern "C" int ntl_ascii_create(ntl_ctx *c, const char *bytes, const uint64_t *off, uint64_t nrec, ntl_ascii **out)
{
    if (!c || !out || !off || (!bytes && nrec)) return NTL_EINVAL;
    *out = nullptr;
    for (uint64_t i = 0; i < nrec; i++) {
        if (off[i + 1] < off[i]) return fail(c, NTL_EINVAL, "offsets must be non-decreasing");
        if (off[i + 1] - off[i] >= 0xFFFFFFFFull) return fail(c, NTL_EINVAL, "record " + std::to_string(i) + " is longer than 2^32 bytes");
    }
    std::unique_ptr<ntl_ascii> a(new ntl_ascii());
    a->c = c;
    a->off.resize(nrec + 1);
    for (uint64_t i = 0; i <= nrec; i++) a->off[i] = off[i] - off[0];
    const uint64_t total = a->off[nrec];
    (void)hipSetDevice(c->device);
    if (int rc = a->bytes.alloc(c, total + 16)) return rc;
    if (total) {
        ProfSpan span(c, "ascii_upload");
        HIPCHK(c, hipMemcpyAsync(a->bytes.p, bytes + off[0], total, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, main_wait(c)); /* the caller's arrays are free again */
    *out = a.release();
    return NTL_OK;
}

extern "C" void ntl_ascii_destroy(ntl_ascii *a)
{
    if (!a) return;
    (void)hipSetDevice(a->c->device);
    delete a; /* the block returns to MAIN's cache: whatever is queued there and reads it runs first */
}
extern "C" uint64_t ntl_ascii_nrec(const ntl_ascii *a) { return a ? a->off.size() - 1 : 0; }
extern "C" uint64_t ntl_ascii_bytes(const ntl_ascii *a) { return a ? a->off.back() : 0; }

struct ntl_stitched {
    ntl_ctx *c;
    uint64_t total = 0;
    DevBuf out, aux;
    std::vector<uint64_t> host_aux; /* source of the asynchronous upload: outlives it (`queued`) */
    hipEvent_t queued = nullptr;    /* on MAIN behind the kernel */
};

/* The output text of the segments, in order (stitch_kernels.h).  Only queues: the stores may be destroyed at once, the result is
 * waited for by ntl_stitched_copy. */
extern "C" int ntl_stitch(ntl_ctx *c, const ntl_ascii *const *stores, uint32_t n_stores, const ntl_stitch_seg *segs, uint64_t n_segs,
                          ntl_stitched **out)
{
    if (!c || !out || (n_stores && !stores) || (n_segs && !segs)) return NTL_EINVAL;
    *out = nullptr;
    for (uint32_t i = 0; i < n_stores; i++)
        if (!stores[i] || stores[i]->c != c) return fail(c, NTL_EINVAL, "store " + std::to_string(i) + " is not a store of this context");
    std::unique_ptr<ntl_stitched> r(new ntl_stitched());
    r->c = c;
    /* the device's tables in one block: the complement table (256 bytes), off[n + 1], seg[n] -- n counts the non-empty segments */
    std::vector<uint64_t> &H = r->host_aux;
    std::vector<StitchSeg> dseg;
    H.assign(256 / 8, 0);
    {
        uint8_t *comp = (uint8_t *)H.data();
        for (int b = 0; b < 256; b++) comp[b] = (uint8_t)b;
        const char *from = "ACGTUNMRWSYKVHDBacgtunmrwsykvhdb", *to = "TGCAANKYWSRMBDHVtgcaankywsrmbdhv"; /* bin/ntlink_patch_gaps.py:50-53 */
        for (int j = 0; from[j]; j++) comp[(uint8_t)from[j]] = (uint8_t)to[j];
    }
    uint64_t total = 0;
    for (uint64_t i = 0; i < n_segs; i++) {
        const ntl_stitch_seg &g = segs[i];
        const std::string at = "segment " + std::to_string(i) + ": ";
        if (g.lo > g.hi) return fail(c, NTL_EINVAL, at + "lo " + std::to_string(g.lo) + " is above hi " + std::to_string(g.hi));
        StitchSeg d = {0, 0, 0};
        if (g.store == NTL_STITCH_FILL) {
            if (g.flags) return fail(c, NTL_EINVAL, at + "a fill takes no flags");
            if (g.rec > 255u) return fail(c, NTL_EINVAL, at + "the fill byte " + std::to_string(g.rec) + " is no byte");
            d.flags = STITCH_FILL | (g.rec << 8);
        } else {
            if (g.store >= n_stores) return fail(c, NTL_EINVAL, at + "store " + std::to_string(g.store) + " out of range (" + std::to_string(n_stores) + " stores)");
            const ntl_ascii *a = stores[g.store];
            if (g.rec >= a->off.size() - 1)
                return fail(c, NTL_EINVAL, at + "record " + std::to_string(g.rec) + " out of range (" + std::to_string(a->off.size() - 1) + " records)");
            const uint64_t len = a->off[g.rec + 1] - a->off[g.rec];
            if (g.hi > len) return fail(c, NTL_EINVAL, at + "hi " + std::to_string(g.hi) + " is beyond the record's " + std::to_string(len) + " bytes");
            if (g.flags & ~(uint32_t)(NTL_STITCH_REVCOMP | NTL_STITCH_LOWER | NTL_STITCH_LOWER_FIRST))
                return fail(c, NTL_EINVAL, at + "unknown flag bits " + std::to_string(g.flags));
            d.src = (uint64_t)(uintptr_t)a->bytes.as<uint8_t>() + a->off[g.rec] + g.lo;
            d.flags = g.flags;
        }
        if (g.hi == g.lo) continue; /* nothing to write, and nothing to lower */
        H.push_back(total);
        dseg.push_back(d);
        total += g.hi - g.lo;
    }
    H.push_back(total);
    const uint64_t n = dseg.size();
    if ((total + STITCH_TILE - 1) / STITCH_TILE >= 0x7FFFFFFFull) return fail(c, NTL_EINVAL, "more output than one stitch call holds");
    static_assert(sizeof(StitchSeg) == 16, "two words per device segment");
    H.resize(32 + n + 1 + 2 * n);
    if (n) memcpy(H.data() + 32 + n + 1, dseg.data(), n * sizeof(StitchSeg));
    r->total = total;
    (void)hipSetDevice(c->device);
    int rc;
    if ((rc = r->out.alloc(c, (total + 15) / 16 * 16 + 16)) || (rc = r->aux.alloc(c, H.size() * 8))) return rc;
    if (total) {
        HIPCHK(c, hipMemcpyAsync(r->aux.p, H.data(), H.size() * 8, hipMemcpyHostToDevice, c->stream));
        StitchArgs A;
        A.comp = r->aux.as<uint8_t>();
        A.off = r->aux.as<uint64_t>() + 32;
        A.seg = (const StitchSeg *)(r->aux.as<uint64_t>() + 32 + n + 1);
        A.n = n; A.total = total; A.out = r->out.as<uint8_t>();
        {
            ProfSpan span(c, "stitch");
            hipLaunchKernelGGL(stitch_kernel, dim3((unsigned)((total + STITCH_TILE - 1) / STITCH_TILE)), dim3(STITCH_NT), 0, c->stream, A);
        }
        HIPCHK(c, hipGetLastError());
        if ((r->queued = c->pq.event_get())) HIPCHK(c, hipEventRecord(r->queued, c->stream));
        else HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    *out = r.release();
    return NTL_OK;
}

extern "C" uint64_t ntl_stitched_bytes(const ntl_stitched *s) { return s ? s->total : 0; }

/* bytes [lo, hi) of the result into out (page-locked memory: one DMA); waits for them */
extern "C" int ntl_stitched_copy(const ntl_stitched *s, uint64_t lo, uint64_t hi, char *out)
{
    if (!s) return NTL_EINVAL;
    ntl_ctx *c = s->c;
    if (lo > hi || hi > s->total) return fail(c, NTL_EINVAL, "range [" + std::to_string(lo) + ", " + std::to_string(hi) + ") outside the result's " + std::to_string(s->total) + " bytes");
    if (lo == hi) return NTL_OK;
    if (!out) return NTL_EINVAL;
    (void)hipSetDevice(c->device);
    HIPCHK(c, hipMemcpyAsync(out, s->out.as<uint8_t>() + lo, hi - lo, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, main_wait(c));
    return NTL_OK;
}

extern "C" void ntl_stitched_destroy(ntl_stitched *s)
{
    if (!s) return;
    (void)hipSetDevice(s->c->device);
    if (s->queued) { (void)hipEventSynchronize(s->queued); s->c->pq.event_put(s->queued); } /* host_aux was the upload's source */
    delete s;
}

/* out[i] = the bytes of [rec_off[i], rec_off[i + 1]) of the text that are one of ACGTacgt (count_kernels.h).  Queued on MAIN behind
 * the stitch; waits: out is filled and rec_off free when the call returns. */
extern "C" int ntl_stitched_base_counts(const ntl_stitched *s, const uint64_t *rec_off, uint64_t n_rec, uint64_t *out)
{
    if (!s) return NTL_EINVAL;
    ntl_ctx *c = s->c;
    if (n_rec == 0) return NTL_OK;
    if (!rec_off || !out) return fail(c, NTL_EINVAL, "rec_off and out are needed");
    for (uint64_t i = 0; i < n_rec; i++)
        if (rec_off[i + 1] < rec_off[i])
            return fail(c, NTL_EINVAL, "rec_off descends at record " + std::to_string(i) + ": " + std::to_string(rec_off[i]) + " then " + std::to_string(rec_off[i + 1]));
    if (rec_off[n_rec] > s->total)
        return fail(c, NTL_EINVAL, "rec_off ends at " + std::to_string(rec_off[n_rec]) + ", beyond the result's " + std::to_string(s->total) + " bytes");
    CountArgs A;
    A.n_rec = n_rec; A.begin = rec_off[0]; A.end = rec_off[n_rec]; A.base = A.begin & ~15ull;
    if (A.begin == A.end) { memset(out, 0, n_rec * sizeof(uint64_t)); return NTL_OK; }
    const uint64_t tiles = (A.end - A.base + COUNT_TILE - 1) / COUNT_TILE;
    if (tiles >= 0x7FFFFFFFull) return fail(c, NTL_EINVAL, "more text than one count call holds");
    (void)hipSetDevice(c->device);
    DevBuf d_off, d_out;
    int rc;
    if ((rc = d_off.alloc(c, (n_rec + 1) * 8)) || (rc = d_out.alloc(c, n_rec * 8))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_off.p, rec_off, (n_rec + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_out.p, 0, n_rec * 8, c->stream));
    A.text = s->out.as<uint8_t>(); A.rec_off = d_off.as<uint64_t>(); A.out = d_out.as<unsigned long long>();
    {
        ProfSpan span(c, "base_count");
        hipLaunchKernelGGL(base_count_kernel, dim3((unsigned)tiles), dim3(COUNT_NT), 0, c->stream, A);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, d_out.p, n_rec * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, main_wait(c));
    return NTL_OK;
}

/* ------------------------------------------------------------------ sketch --------------- */

/* ------------------------------------------------------------------ index (type) --------- */

static std::atomic<uint64_t> g_index_gen{1};

struct ntl_index {
    ntl_ctx *c;
    /* the caller's + one per PENDING sketch / map result that was queued against it: their kernels read the table, and an
       overflowed sketch is made again from it (sketch_finalize, mapres_finalize).  ntl_index_destroy only drops the caller's. */
    mutable std::atomic<int> refs{1};
    uint64_t gen = 0;                    /* identity of this index: a sketch made for it remembers the number, not the address */
    int bits = 0;
    uint64_t nslots = 0;
    mutable uint64_t size = 0;
    mutable bool size_known = false;
    /* hit fraction of the last COMPLETED batch mapped against this index: picks the probe form of the next one.  Shared with
       results that are destroyed before they complete (their zombies report when their work is done). */
    std::shared_ptr<std::atomic<float>> hit_fraction = std::make_shared<std::atomic<float>>(0.0f);
    uint32_t n_ctg = 0;
    DevBuf slots, special, ctg_len, cnt; /* cnt: device-side count of kept keys, fetched on demand */
    DevBuf tags;                         /* one byte per slot (map_kernels.h index_tag) */
    std::vector<uint32_t> h_ctg_len;     /* source of the asynchronous upload: must outlive it */
    hipEvent_t built = nullptr;          /* on the building context's MAIN stream: other contexts' streams wait for it */
};

/* what emit_kernel leaves in the sketch's page-locked slot */
struct SketchSums { uint32_t total_mx, redo_n, fb_n, list_fail; unsigned long long nfound; }; /* redo_n, fb_n: one 8-byte copy; list_fail: the
                                                                                                      strips' lists ran out of pool (StripLists) */

struct ntl_sketch {
    ntl_ctx *c;
    std::atomic<int> refs{1};             /* the caller's + one per map result that may have to be redone from it */
    uint64_t nseq = 0;
    mutable uint64_t count = 0;           /* valid once !pending */
    mutable uint64_t strips = 0, redo_strips = 0; /* diagnostics: strips of the window pass, strips that also took the exact pass */
    mutable uint64_t fallback_strips = 0;  /* ... strips the threshold pass handed to the block-minima pass */
    mutable uint64_t nfound = 0;
    mutable DevBuf records; /* MxRecord[cap] */
    mutable DevBuf mx_off;  /* u32[nseq+1] */
    mutable std::vector<uint32_t> h_off; /* the host's copy of mx_off, or empty: fetched by the first ntl_sketch_format (the ranges'
                                            minimizer counts size its work), kept for the next ranges of the same sketch */
    mutable uint64_t cap = 0;             /* records the arrays can hold */
    /* ntl_sketch_run_indexed: the minimizers were looked up in index cand_gen while they were emitted */
    uint64_t cand_gen = 0;
    mutable DevBuf cand;    /* Cand[cap] */
    bool no_records = false; /* ntl_sketch_run_for_map: `records` stays empty */
    mutable bool from_lists = false; /* diagnostics: the last round of sketch_enqueue wrote lists */
    mutable ntl_plan_info plan = {};  /* diagnostics: the WindowPlan the last round of sketch_enqueue carried out (ntl_sketch_plan) */
    mutable bool no_lists = false; /* the window stage writes the bitmask whatever the window: the second round of a sketch whose lists ran out of pool */
    mutable DevBuf rpos;    /* u32[cap] beside cand: the minimizers' positions in their reads (their strands: bit 31 of Cand::meta) */
    mutable DevBuf sums;    /* SketchSums on the device: total (read by the map kernels: a sketch that overflowed its arrays is left alone) */
    /* the lookup's hit count has not reached the slot yet: the next kernel queued behind the lookup on MAIN copies it there -- the
       gather of the first map result on this sketch (map_enqueue), or sketch_nfound_kernel when the count is asked for first */
    mutable bool nfound_owed = false;
    mutable Pending lz;                   /* lazy completion (pending.h); holds[0]: the index the sketch was made for */
    mutable uint64_t gen = 0;             /* bumped when the sketch had to be made again with larger arrays */
    const ntl_batch *src = nullptr;       /* held (refs) while pending: a sketch that overflowed is redone from it */
    int k = 0, w = 0;
};

static int sketch_finalize(const ntl_sketch *s);

/* The last reference to an index goes.  Dropped by the context that built it: its device blocks return to that context's cache.
 * Dropped by ANOTHER context (a worker context completing or reaping work that outlived the caller's ntl_index_destroy): the
 * owner's cache and event lists belong to the owner's thread, so the blocks bypass the cache (DevPool::free_uncached, the one call
 * a foreign thread may make: a slab block waits in limbo for the owner's streams, a single block's hipFree for the device). */
static void index_unref(const ntl_index *cix, ntl_ctx *by)
{
    ntl_index *ix = const_cast<ntl_index *>(cix);
    if (!ix || --ix->refs != 0) return;
    (void)hipSetDevice(ix->c->device);
    if (by != ix->c) {
        for (DevBuf *b : {&ix->slots, &ix->special, &ix->ctg_len, &ix->cnt, &ix->tags}) {
            ix->c->mem.free_uncached(b->p, b->bytes);
            b->p = nullptr; b->bytes = 0;
        }
        if (ix->built) (void)hipEventDestroy(ix->built);
    } else ix->c->pq.event_put(ix->built);
    delete ix;
}

/* what a Pending holds for its queued kernels (pending.h) */
static void hold_index(const void *ix, void *by) { index_unref((const ntl_index *)ix, (ntl_ctx *)by); }
static void hold_batch(const void *b, void *) { batch_unref((const ntl_batch *)b); }

/* the check of a sketch that was destroyed before anybody asked for its count; arg: the records its arrays hold */
static const char *sketch_check(const PinSlot &slot, uint64_t cap, std::atomic<float> *)
{
    const SketchSums &hs = (const SketchSums &)slot;
    return hs.total_mx > cap || hs.list_fail ? "a sketch held more minimizers than its record array and was destroyed before anybody asked for its count" : nullptr;
}

/* An error path: whatever was queued must not outlive what the handle lets go, so the device is drained first; a map result's device
   sums (dsums) are in an unknown state then and are zeroed again for the slot's next holder. */
static int pending_abort(ntl_ctx *c, Pending &p, int rc, bool map_scrub = false)
{
    (void)sync_both(c);
    if (map_scrub && p.slot) (void)hipMemset(c->pq.slot_dsums(p.slot), 0, sizeof(PinSlot));
    p.pending = false;
    p.failed = rc;
    p.settle(c->pq);
    return rc;
}

static void sketch_unref(const ntl_sketch *cs)
{
    ntl_sketch *s = const_cast<ntl_sketch *>(cs);
    if (!s || --s->refs != 0) return;
    (void)hipSetDevice(s->c->device);
    /* nobody asked: the device blocks go back now (stream-ordered), event, slot and index when the work is done */
    s->lz.orphan(s->c->pq, sketch_check, s->cap);
    if (s->src) batch_unref(s->src);
    delete s;
}

static uint64_t h_srol1(uint64_t x)
{
    uint64_t m = ((x & 0x8000000000000000ull) >> 30) | ((x & 0x100000000ull) >> 32);
    return ((x << 1) & 0xFFFFFFFDFFFFFFFFull) | m;
}

/* sketch_fast_kernel's keys (sketch2_kernels.h, "exact" (3)) rely on this property of the ntHash seeds: a base and its
   complement have 31-bit rings (bits 33..63) whose set bits add up to an even number */
constexpr int ring31_bits(uint64_t s) { int n = 0; for (uint64_t r = s >> 33; r; r >>= 1) n += (int)(r & 1); return n; }
static_assert((ring31_bits(0x3c8bfbb395c60474ull) + ring31_bits(0x295549f54be24456ull)) % 2 == 0 &&
              (ring31_bits(0x3193c18562a02b4cull) + ring31_bits(0x20323ed082572324ull)) % 2 == 0,
              "the ring sum of fwd and rev could be 2^31 - 1: the 32-bit window pass would need a wrap check");

static void make_tables(int k, uint64_t roll[16][2], uint64_t seed[4][2])
{
    const uint64_t S[4] = {0x3c8bfbb395c60474ull, 0x3193c18562a02b4cull, 0x20323ed082572324ull, 0x295549f54be24456ull};
    uint64_t sk[4], sck[4];
    for (int c = 0; c < 4; c++) {
        uint64_t a = S[c], b = S[3 - c];
        for (int i = 0; i < k; i++) { a = h_srol1(a); b = h_srol1(b); }
        sk[c] = a; sck[c] = b;
        seed[c][0] = S[c]; seed[c][1] = S[3 - c];
    }
    for (int in = 0; in < 4; in++)
        for (int o = 0; o < 4; o++) {
            roll[in << 2 | o][0] = S[in] ^ sk[o];
            roll[in << 2 | o][1] = sck[in] ^ S[3 - o];
        }
}

static uint64_t h_sror1(uint64_t x)
{
    uint64_t m = ((x & 0x200000000ull) << 30) | ((x & 1ull) << 32);
    return ((x >> 1) & 0xFFFFFFFEFFFFFFFFull) | m;
}

/* four-base init table (k-independent), see dev_common.h hash_init */
static void make_g4(uint64_t g4[256][2])
{
    const uint64_t S[4] = {0x3c8bfbb395c60474ull, 0x3193c18562a02b4cull, 0x20323ed082572324ull, 0x295549f54be24456ull};
    for (int b = 0; b < 256; b++) {
        uint64_t f = 0, u = 0;
        for (int j = 0; j < 4; j++) {
            const int c = (b >> (2 * j)) & 3;
            f = h_srol1(f) ^ S[c];
            u = h_sror1(u) ^ S[3 - c];
        }
        g4[b][0] = f; g4[b][1] = u;
    }
}

static void make_g8(std::vector<uint64_t> &g8)
{
    const uint64_t S[4] = {0x3c8bfbb395c60474ull, 0x3193c18562a02b4cull, 0x20323ed082572324ull, 0x295549f54be24456ull};
    g8.resize(65536 * 2);
    for (int b = 0; b < 65536; b++) {
        uint64_t f = 0, u = 0;
        for (int j = 0; j < 8; j++) {
            const int c = (b >> (2 * j)) & 3;
            f = h_srol1(f) ^ S[c];
            u = h_sror1(u) ^ S[3 - c];
        }
        g8[2 * b] = f; g8[2 * b + 1] = u;
    }
}

/* calls f(std::integral_constant<int, v>()) for the v in [LO, HI) that `value` equals: a run-time value becomes a template argument */
template <int LO, int HI, typename F>
static void with_constant(int value, F &&f)
{
    if constexpr (LO < HI) {
        if (value == LO) f(std::integral_constant<int, LO>());
        else with_constant<LO + 1, HI>(value, f);
    }
}

/* exact 64-bit pass: over all strips (multi-run strips when `multi`), or -- redo != NULL -- over the strips the fast pass flagged */
template <int C, int NT, int R0>
static void launch_mask_r0(hipStream_t st, const SketchArgs &A, unsigned strips, bool single, bool multi)
{
    const unsigned grid = A.redo_list ? 2048u : ((strips + 7u) & ~7u);
    if (single) hipLaunchKernelGGL((sketch_mask_kernel<C, NT, false, R0>), dim3(grid), dim3(NT), 0, st, A);
    if (multi) hipLaunchKernelGGL((sketch_mask_kernel<C, NT, true, R0>), dim3((strips + 7u) & ~7u), dim3(NT), 0, st, A);
}

template <int C>
static void launch_mask(hipStream_t st, const SketchArgs &A, unsigned strips, bool single, bool multi, int nt)
{
    /* 16 k-mers per lane: one instantiation per strip width, R0 at run time (this is the redo / multi-run pass since the 32-bit
       window pass took over the common case); 4 and 1 k-mers per lane (w < 16): R0 as a template parameter */
    if (C == 16 && nt == 128) launch_mask_r0<C, 128, -1>(st, A, strips, single, multi);
    else if (C == 16 && nt == SK_NT_LONG) { if constexpr (C == 16) launch_mask_r0<16, SK_NT_LONG, -1>(st, A, strips, single, multi); }
    else if (C == 16) launch_mask_r0<C, SK_NT, -1>(st, A, strips, single, multi);
    else with_constant<0, C>(A.G.r0, [&](auto r0) { launch_mask_r0<C, SK_NT, decltype(r0)::value>(st, A, strips, single, multi); });
}

/* workgroups of `threads` lanes of a kernel that one CU holds at once */
template <typename K>
static int occupancy_blocks(K kern, int threads)
{
#ifdef NTL_SIM
    (void)kern; (void)threads;
    return 2;
#else
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, threads, 0) != hipSuccess || n < 1) n = 1;
    return n;
#endif
}

/* What a context would otherwise do inside its first sketch call, done when it is made: the first slab of device memory and
   the occupancy figures of the resident window kernels (the query loads the library's code object onto the device: some
   ten milliseconds, once per process).  Best effort: whatever fails here is tried again where it is needed. */
__global__ void ntl_noop_kernel() {}

static void ctx_prime(ntl_ctx *c)
{
#ifndef NTL_SIM
    hipLaunchKernelGGL(ntl_noop_kernel, dim3(1), dim3(64), 0, c->stream); /* the library's code object goes onto the device with its first launch */
    (void)hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
    {
        DevBuf first;
        (void)first.alloc(c, 1 << 20);
    }
    for (int s = 0; s < WS_DEFAULTS; s++)
        with_wave_kernel((WaveShape)s, [&](auto kern, unsigned threads) { c->occ[(const void *)kern] = occupancy_blocks(kern, (int)threads); });
    c->err.clear();
#else
    (void)c;
#endif
}

/* a zero-filled bitmask of at least `bytes` for the window stage (stream sid): one that an earlier emit kernel cleared
   behind itself, or a new one.  With the pipeline on, three masks rotate, so that the window stage of batch i+1 never
   waits for the emit kernel of batch i. */
static int mask_take(ntl_ctx *c, size_t bytes, int sid, CleanMask *out)
{
    const size_t want = (bytes + 255) & ~(size_t)255;
    const size_t keep = c->pipelined ? 2 : 0;
    if (c->masks.size() > keep) {
        for (size_t i = 0; i < c->masks.size() - keep; i++) {
            CleanMask m = c->masks[i];
            if (m.bytes >= want && m.bytes <= want + want / 4 + (1 << 20)) {
                c->masks.erase(c->masks.begin() + (long)i);
                if (m.clean && c->s(sid) != c->stream) (void)hipStreamWaitEvent(c->s(sid), m.clean, 0);
                c->pq.event_put(m.clean);
                m.clean = nullptr;
                *out = m;
                return NTL_OK;
            }
        }
    }
    while (c->masks.size() > 4) { /* other batch sizes came and went */
        c->mem.free_uncached(c->masks.front().p, c->masks.front().bytes);
        c->pq.event_put(c->masks.front().clean);
        c->masks.pop_front();
    }
    CleanMask m;
    if (c->mem.alloc_uncached(want, &m.p) != DevPool::OK) return fail(c, NTL_ENOMEM, "hipMalloc failed");
    m.bytes = want;
    HIPCHK(c, hipMemsetAsync(m.p, 0, want, c->s(sid)));
    *out = m;
    return NTL_OK;
}

static void launch_small(ntl_ctx *c, const SketchArgs &A, unsigned strips, bool multi)
{
    with_constant<2, 16>(A.G.w, [&](auto w) {
        constexpr int W = decltype(w)::value;
        const dim3 grid((strips + 7u) & ~7u);
        hipLaunchKernelGGL((sketch_small_kernel<W, false>), grid, dim3(256), 0, c->wstream, A);
        if (multi) hipLaunchKernelGGL((sketch_small_kernel<W, true>), grid, dim3(256), 0, c->wstream, A);
    });
}

#ifndef NTL_EMIT_DENSE_CAP
#define NTL_EMIT_DENSE_CAP 8192 /* emit_kernel's positions per round for the dense sketches of the small windows (sketch_kernels.h) */
#endif

/* geometry of the window pass for (k, w): k-mers per lane, lanes per strip.  `small`: it runs as sketch_small_kernel (2 <= w <= 15: the
   stages around `pair`); NTL_SKETCH_SMALL=0, or any setting of the k-mers-per-lane knob: the round-1 forms with four / one k-mer per
   lane (A/B, tests).  The knobs are read per call: the tests switch them inside one process.  long_strips: window_plan's second call,
   for strips of SK_NT_LONG lanes (w >= 16, sixteen k-mers per lane). */
static int sketch_geometry(ntl_ctx *c, int k, int w, SketchGeom &G, int &C, int &nt, bool &small, bool long_strips = false)
{
    if (k < 1 || k > 4096 || w < 1) return fail(c, NTL_EINVAL, "k must be in 1..4096 and w >= 1");
    C = w >= 16 ? 16 : (w >= 4 ? 4 : 1);
    G.k = k; G.w = w;
    const char *ce = getenv("NTL_SKETCH_C"); /* tuning knob: k-mers per lane (16, 4, 1) */
    small = w >= 2 && w <= 15 && !ce;
    if (const char *e = small ? getenv("NTL_SKETCH_SMALL") : nullptr) small = atoi(e) != 0;
    if (small) { /* sketch_small_kernel: 256 lanes x 16 k-mers, the minima of the 16 windows a lane starts in registers */
        C = 16; nt = SK_NT;
        G.a = 0; G.r0 = 0;
        G.LW = nt - 1;          /* the last lane only supplies the w - 1 elements behind the last window */
        G.NWO = G.LW * C - 1;
        return NTL_OK;
    }
    if (ce) {
        const int v = atoi(ce);
        if ((v == 16 || v == 4 || v == 1) && w >= v) C = v;
    }
    G.a = (w - C) / C; G.r0 = (w - C) % C;
    /* lanes per strip: 128-lane strips waste fewer lanes on the last strip of a ~10 kb read, 256-lane strips fewer on the halo
       (a+2 lanes) and fit eight workgroups of the 32-bit window pass on a CU.  Measured with that pass: 256 lanes +6 % at w=100
       (10 kb reads 675 -> 714 Gbases/s, 20 kb reads 696 -> 747); 128 lanes stay for the small windows (w < 64) */
    nt = (C == 16 && w < 64) ? 128 : SK_NT;
    if (const char *e = getenv("NTL_SKETCH_NT")) { /* tuning knob; ignored where it leaves no lane to own a window */
        const int v = atoi(e);
        if ((v == 256 || (v == 128 && C == 16)) && v - (G.a + 2) >= 2) nt = v;
    }
    if (long_strips && C == 16) nt = SK_NT_LONG;
    G.LW = nt - (G.a + 2);
    if (G.LW < 2 && C != 16) { /* a tuning knob (NTL_SKETCH_C) made the strip too short for this window: back to the default */
        C = 16;
        G.a = (w - C) / C; G.r0 = (w - C) % C;
        nt = SK_NT;
        G.LW = nt - (G.a + 2);
    }
    G.NWO = G.LW * C - 1;
    if (G.LW < 2 || G.NWO < 1) {
        char msg[160];
        snprintf(msg, sizeof msg, "window size w=%d is beyond this build's limit of w <= %d (a strip of %d x 16 k-mers must hold two windows' lanes)",
                 w, NTL_MAX_W, SK_NT);
        return fail(c, NTL_EINVAL, msg);
    }
    return NTL_OK;
}

/* The plan of one sketch (see WindowPlan): a pure function of (k, w), the batch's lengths, the number of streams, `no_lists` and the
   knobs -- every knob that takes part is read here and nowhere else, per call: the tests switch them inside one process.  Nothing is
   allocated or launched. */
static int window_plan(ntl_ctx *c, const ntl_batch *b, int k, int w, bool no_lists, WindowPlan &P)
{
    memset(&P, 0, sizeof P);
    bool small;
    int rc;
    if ((rc = sketch_geometry(c, k, w, P.G, P.C, P.nt, small))) return rc;
    const SketchGeom &G = P.G;
    auto count_strips = [&]() {
        P.strips = 0;
        for (uint64_t i = 0; i < b->nseq; i++) {
            const uint64_t len = b->seq_len[i];
            if (len + 2 > (uint64_t)k + (uint64_t)w) P.strips += (len - k - w + 2 + (uint64_t)G.NWO - 1) / (uint64_t)G.NWO;
        }
    };
    count_strips();
    if (P.strips >= 0x7FFFFFFFull) return fail(c, NTL_EINVAL, "batch too large: too many strips");
    /* 32-bit fast pass + exact pass over what it flags; the exact pass alone for small windows / huge k */
    bool fast = P.C == 16 && k <= 16 * SK2_QMAX && G.a + 2 <= SK2_PAD && !small;
    if (const char *e = getenv("NTL_SKETCH_FAST")) fast = fast && atoi(e) != 0; /* 0: exact pass only (A/B, tests) */
    P.pass = small ? WP_SMALL : WP_EXACT_ONLY;
    if (!fast) return NTL_OK;
    /* Threshold-sparsified windows where a strip's candidate list fits: keys below T = 2^32 * cpw / w are candidates,
       cpw = 10 of them per window -- fewer and more strips have a window without one (they take the exact pass: 0.7 % at 10, 2 % at 9),
       more and the list work grows (profiles/r03p_*).  NTL_SKETCH_THRESH=0: no threshold anywhere; = x: x candidates per window. */
    const char *te = getenv("NTL_SKETCH_THRESH");
    double cpw = te ? atof(te) : 10.0;
    if (cpw == 1.0) cpw = 10.0;
    if (cpw > 0 && P.nt != 128 && 4096.0 * cpw / w <= WP_FIT_THRESH) P.thresh = (uint32_t)std::min(4294967295.0, 4294967296.0 * cpw / w);
    if (const char *e = getenv("NTL_SKETCH_ABLATE")) P.dbg = atoi(e); /* tools/sketch_bench.py only: results are wrong */
    if (const char *e = getenv("NTL_SKETCH_FORCE_REDO")) P.force_redo = atoi(e); /* tests: every strip takes both passes */
    P.expected_per_strip = 4096.0 * (double)P.thresh / 4294967296.0; /* (per 4096 k-mers whatever the strip length: what the WP_FIT_* bounds are written for) */
    P.dense_windows = P.expected_per_strip > WP_FIT_15_6;
    const bool sparse = P.thresh && (P.dbg & ~24) == 0; /* (ablation bits 8 and 16 exist in the threshold and wave kernels too) */
    /* one wavefront per strip, 64 k-mers per lane (sketch_wave_kernel) where a lane's first k-mer lies in its own 64 bases and a strip's
       candidates fit its list: a window only enters its scans as a distance, so it goes up to the block-minima pass's w <= 1151, which
       decides the strips it gives up.  NTL_SKETCH_WAVE=0: the workgroup-per-strip forms; 4, 8, 16: wavefronts per workgroup (A/B, tests) */
    const char *we = getenv("NTL_SKETCH_WAVE");
    const int wave = we ? atoi(we) : 1;
    if (sparse && wave && k <= 64 && P.expected_per_strip <= WP_FIT_WAVE) {
        P.pass = WP_WAVE;
        P.big = G.a + 2 > 16;
    } else if (sparse && G.a + 2 <= 16) { /* the workgroup-per-strip passes' limit: w <= 255 */
        P.pass = WP_THRESH;
        const char *de = getenv("NTL_SKETCH_THRESH_DIRECT"); /* 1: the variant without staged keys for the large windows too (A/B) */
        P.direct = (de && atoi(de)) || P.expected_per_strip > WP_FIT_STAGED;
    } else {
        P.pass = WP_BLOCK_MINIMA; /* the 20-KB variants hold 128 searched windows per strip: about NWO / (w + 1) are expected (38 at w = 100) */
        P.big = G.a + 2 > 16 || w < 64;
    }
    if (P.pass != WP_WAVE) return NTL_OK;
    /* The strip length, one per sketch: every table, list and pass of it is made for P.nt lanes of 16 k-mers.  8192 ordinals -- 128
       k-mers per lane of sketch_wave_kernel, which halves what it pays per strip (the first k-mers from the tables, header, sentinels,
       window 0, the list's place) and the halo of w + 15 elements that two strips both roll -- exist for the windows whose
       4096-ordinal shape is <8, 11, 4>, and are NOT the default: measured on C3 (profiles/HISTORY.md, "8192-ordinal strips") the long
       shape issues 9 % fewer vector instructions per base, but alone its 24 wavefronts per CU are only 2.4 % faster than the short
       shape's 32 (1.80 against 1.84 ms per launch: under the 3 % that tells a gain from the boxes' wander), and beside the other
       stream's kernels, where both run 24, the step takes 60.2 ms against 58.0: 4096 won on both paths.  NTL_SKETCH_STRIP=8192: the long strips wherever they exist; 4096: the short ones (A/B, tests). */
    const bool long_range = P.expected_per_strip <= WP_FIT_11_4 && wave != 4 && wave != 16; /* (those two: A/B shapes of the short strips) */
    bool long_strips = false;
    if (const char *e = getenv("NTL_SKETCH_STRIP")) {
        const int v = atoi(e);
        if (v == 4096) long_strips = false;
        else if (v == 8192) long_strips = long_range;
    }
    if (long_strips) {
        if ((rc = sketch_geometry(c, k, w, P.G, P.C, P.nt, small, true))) return rc;
        count_strips();
    }
    /* Where the fast pass is sketch_wave_kernel (every window ntLink is run with) the passes write per-strip LISTS of minimizers
       (sketch_kernels.h, StripLists) and emit_list_kernel reads those; everywhere else, a bitmask of one bit per base and emit_kernel.
       NTL_SKETCH_LISTS=0: the bitmask everywhere (A/B, tests). */
    P.lists = b->nseq && P.strips && !no_lists;
    if (const char *e = getenv("NTL_SKETCH_LISTS")) P.lists = P.lists && atoi(e) != 0;
    if (P.lists) {
        /* a slot holds the expected 2 NWO / (w + 1) minimizers of a strip with room for their spread (what does not fit -- low-complexity
           sequence -- lives in the pool behind the slots); the pool: 32 entries per strip, at least a million */
        const double mean = 2.0 * (double)G.NWO / (double)(w + 1);
        uint64_t slot = ((uint64_t)(mean * 1.25 + 24.0) + 15u) & ~(uint64_t)15u;
        if (const char *e = getenv("NTL_LIST_SLOT")) slot = std::max<uint64_t>(1, (uint64_t)atoll(e)); /* tests: force strips into the pool */
        uint64_t pool = std::max<uint64_t>((uint64_t)1 << 20, 32 * P.strips);
        if (const char *e = getenv("NTL_LIST_POOL")) pool = (uint64_t)atoll(e);                      /* tests: make the pool run out */
        if ((P.strips + 1) * slot + pool >= 0xFFFFFFF0ull) P.lists = false; /* (entries are addressed with 32 bits) */
        else { P.slot = (uint32_t)slot; P.pool = (uint32_t)pool; }
    }
    /* Beside the other stream's kernels (two streams: the lookup / map kernels of the previous batch) the resident wavefronts take HALF the
       CU's 32 slots: with more, those kernels' workgroups wait for slots that never come free before the launch ends, and the step is as long as on
       one stream (C3, profiles/r04_window_grid_sweep.json: 16 per CU 77.6 ms per step, 24 89.5, 32 89.4; alone the launch takes 2.65 ms at 16 against 2.09 at 32). */
    P.beside = 16u;
    if (P.nt == SK_NT_LONG) { /* w >= 235, strips of 8192 */
        P.shape = WS_8_19_7_L128;
        if (P.lists) P.beside = 24u;
    } else if (P.expected_per_strip <= WP_FIT_11_4) { /* w >= 235 at ten candidates per window */
        /* (lists, round 5: the other stream's emit_list_kernel keeps to two resident workgroups per CU -- emit_grid --
           and the window stage takes 24 of the 32 wavefront slots: C3 70.7 ms per step against 75.9 at 16 and 82.5 at
           32, profiles/r05_share_sweep_C3.jsonl) */
        P.shape = wave == 4 ? WS_4_11_4 : (wave == 16 ? WS_16_11_4 : WS_8_11_4);
        if (wave != 16 && P.lists) P.beside = 24u;
    } else if (P.expected_per_strip <= WP_FIT_15_6) { /* w >= 137 */
        P.shape = WS_8_15_6;
    } else {                                          /* w >= 94 */
        /* (dense sketches: the other stream's lookup and map kernels are the longer half of a step, and twelve resident
           wavefronts per CU beside them make the shortest step -- C5: 8 / 12 / 16 / 24: 304.6 / 288.5 / 315.1 / 318.7 ms) */
        P.shape = wave == 4 || (c->pipelined && wave != 8) ? WS_4_19_8 : WS_8_19_8;
        if (P.shape == WS_4_19_8) P.beside = 12u;
    }
    if (const char *e = getenv("NTL_SKW_WGS_PER_CU")) P.wgs_per_cu = std::max(1, atoi(e)); /* tuning */
    if (const char *e = getenv("NTL_SKW_BUDGET")) P.chunk_budget = atoi(e) >= 2 ? (uint32_t)atoi(e) : 0u;
    return NTL_OK;
}

/* the 32-bit pass of the plan over the single-run strips (sketch2_kernels.h), on the window stream; true: it leaves a list of strips
   it gave up, for launch_give_up_pass */
static bool launch_window_pass(ntl_ctx *c, const WindowPlan &P, const Sketch2Args &B)
{
    const unsigned strips = B.A.nstrips;
    const dim3 grid((strips + 7u) & ~7u);
    switch (P.pass) {
    case WP_BLOCK_MINIMA:
        with_constant<0, 16>(P.G.r0, [&](auto r0) {
            constexpr int R0 = decltype(r0)::value;
            if (P.nt == 128 && P.big) hipLaunchKernelGGL((sketch_fast_kernel<128, R0, true>), grid, dim3(128), 0, c->wstream, B);
            else if (P.nt == 128) hipLaunchKernelGGL((sketch_fast_kernel<128, R0, false>), grid, dim3(128), 0, c->wstream, B);
            else if (P.big) hipLaunchKernelGGL((sketch_fast_kernel<SK_NT, R0, true>), grid, dim3(SK_NT), 0, c->wstream, B);
            else hipLaunchKernelGGL((sketch_fast_kernel<SK_NT, R0, false>), grid, dim3(SK_NT), 0, c->wstream, B);
        });
        return false;
    case WP_THRESH:
        if (P.direct) hipLaunchKernelGGL((sketch_thresh_kernel<256, true>), grid, dim3(256), 0, c->wstream, B);
        else hipLaunchKernelGGL((sketch_thresh_kernel<256, false>), grid, dim3(256), 0, c->wstream, B);
        break;
    case WP_WAVE:
        /* resident wavefronts that walk over their strips: as many workgroups as the device holds at once (a multiple of 8: one share of the strips per XCD) */
        with_wave_kernel(P.shape, [&](auto kern, unsigned threads) {
            int &per_cu = c->occ[(const void *)kern];
            if (!per_cu) per_cu = occupancy_blocks(kern, (int)threads);
            int use = c->pipelined ? std::min(per_cu, (int)(P.beside / (threads / 64u))) : per_cu;
            if (P.wgs_per_cu) use = std::min(per_cu, P.wgs_per_cu);
            unsigned wgs = (unsigned)std::max(1, use) * (unsigned)std::max(1, c->n_cu);
            wgs = std::min(wgs, (strips + threads / 64u - 1u) / (threads / 64u));
            wgs = (wgs + 7u) & ~7u;
            /* Two streams, NTL_SKW_BUDGET chunks per wavefront: short-lived workgroups, as many as it takes, that fill what
               the other stream's kernels leave free (those have the higher stream priority and a bounded number of
               resident workgroups: emit_grid) -- and the whole CU while that stream has nothing to run. */
            Sketch2Args Bq = B;
            if (P.chunk_budget) {
                const unsigned per_xcd_chunks = (((strips + 7u) >> 3) + SKW_CHUNK - 1u) / SKW_CHUNK;
                const unsigned per_wg = (threads / 64u) * P.chunk_budget;
                wgs = 8u * ((per_xcd_chunks + per_wg - 1u) / per_wg);
                Bq.chunk_budget = P.chunk_budget;
            }
            ProfSpan sp(c, "sketch_wave", SID_W); /* the window kernel alone (the span "sketch_mask" around this function also holds the block-minima pass) */
            hipLaunchKernelGGL(kern, dim3(wgs), dim3(threads), 0, c->wstream, Bq);
        });
        break;
    default: return false;
    }
    return true;
}

/* what the threshold and wave kernels gave up (a window without a candidate: 0.7 % of the strips): the block-minima pass over that list,
   on stream st behind them */
static void launch_give_up_pass(hipStream_t st, const WindowPlan &P, const Sketch2Args &B)
{
    const unsigned strips = B.A.nstrips;
    with_constant<0, 16>(P.G.r0, [&](auto r0) {
        constexpr int R0 = decltype(r0)::value;
        const dim3 lgrid(std::min(strips, 4096u));
        if (P.nt == SK_NT_LONG && P.big) hipLaunchKernelGGL((sketch_fast_list_kernel<SK_NT_LONG, R0, true>), lgrid, dim3(SK_NT_LONG), 0, st, B, (const uint32_t *)B.fb_list, (const uint32_t *)B.fb_count);
        else if (P.nt == SK_NT_LONG) hipLaunchKernelGGL((sketch_fast_list_kernel<SK_NT_LONG, R0>), lgrid, dim3(SK_NT_LONG), 0, st, B, (const uint32_t *)B.fb_list, (const uint32_t *)B.fb_count);
        else if (P.big) hipLaunchKernelGGL((sketch_fast_list_kernel<256, R0, true>), lgrid, dim3(256), 0, st, B, (const uint32_t *)B.fb_list, (const uint32_t *)B.fb_count);
        else hipLaunchKernelGGL((sketch_fast_list_kernel<256, R0>), lgrid, dim3(256), 0, st, B, (const uint32_t *)B.fb_list, (const uint32_t *)B.fb_count);
    });
}

/* What one sketch_enqueue holds between its stages.  The temporaries return to the context's cache when it ends: every later user of
 * those blocks is queued behind the kernels of this sketch on the stream they were used on, so no wait is needed -- and a block that
 * several streams used goes back with an event behind each (DevBuf::touch), so that the next sketch, whose window kernel runs beside
 * this one's give-up passes, gets it only once they have run, and another block until then. */
struct SketchWork {
    int wsid; hipStream_t ws, ms; /* the window stage's stream id (MAIN when the pipeline is off), its stream, MAIN */
    int ssid; hipStream_t ss;     /* the stream of the passes behind the first window kernel: the side stream, or the window stage's */
    int psid; hipStream_t ps;     /* the preparation's stream: the window stage's (NTL_SIDE_STREAM=2: the side stream) */
    hipStream_t last;             /* where the window stage's last kernel was queued: the emit stage on MAIN waits for it */
    /* queued on `on`; stream `then` goes on behind it */
    static int order(ntl_ctx *c, hipStream_t on, hipStream_t then);
    uint64_t nmask; /* words of the bitmask: one bit per base */
    DevBuf run_n, run_ord, seq_M, nstrips, strip_first, tile, redo, strip_tab; /* (nstrips / strip_first: nseq+1 entries, the scan leaves the total behind the last) */
    SeqTables T; StripLists Ls = {}; StripZero Z = {};
    DevBuf lcnt, lent, loff;
    struct Mask : CleanMask { /* error paths: the mask is not known to be clean any more, it is freed and not kept */
        ntl_ctx *c = nullptr;
        ~Mask() { if (p) c->mem.free_uncached(p, bytes); }
    } mask;
    DevBuf strip_lite;
};
static const uint64_t REDO_HEAD = 16 + 8 * 16; /* words in front of the two lists of `redo` */

int SketchWork::order(ntl_ctx *c, hipStream_t on, hipStream_t then)
{
    if (on == then) return NTL_OK;
    hipEvent_t e = c->pq.event_get();
    if (!e) return fail(c, NTL_EDEVICE, "hipEventCreate failed");
    HIPCHK(c, hipEventRecord(e, on));
    HIPCHK(c, hipStreamWaitEvent(then, e, 0));
    c->pq.event_put(e); /* the wait holds what it needs; the handle may be recorded again */
    return NTL_OK;
}

/* Preparation, on the window stream in front of the window kernels: the temporaries, the batch's tables, the strips' tables.  Every
   block is taken for the stream that writes it first (W.psid) and marked for the others that use it: the window kernel's (wsid), the
   give-up passes' (ssid), MAIN. */
static int sketch_prepare(ntl_ctx *c, const ntl_batch *b, int k, int w, const WindowPlan &P, ntl_sketch *s, SketchWork &W)
{
    const uint64_t nseq = b->nseq, ub_strips = P.strips;
    const int wsid = W.wsid, psid = W.psid;
    auto window_stage_uses = [&](const DevBuf &d) { d.touch(wsid); d.touch(W.ssid); }; /* the window kernel and the passes behind it */
    int rc;
    W.nmask = (b->total_gpos + 31) / 32 + 1;
    if ((rc = W.run_n.alloc(c, (b->nruns + 1) * 4, psid)) || (rc = W.run_ord.alloc(c, (b->nruns + 1) * 4, psid)) ||
        (rc = W.seq_M.alloc(c, (nseq + 1) * 4, psid)) || (rc = W.nstrips.alloc(c, (nseq + 1) * 4, psid)) ||
        (rc = W.strip_first.alloc(c, (nseq + 2) * 4, psid)) || (rc = s->mx_off.alloc(c, (nseq + 1) * 4)) ||
        (rc = s->sums.alloc(c, sizeof(SketchSums), psid))) return rc;
    window_stage_uses(W.run_n); window_stage_uses(W.run_ord); window_stage_uses(W.seq_M);
    s->sums.touch(SID_MAIN); /* zeroed by strip_table_kernel on the window stream, added to and read on MAIN */
    batch_on_wstream(c, b);
    if (W.ps != W.ws && b->ready) HIPCHK(c, hipStreamWaitEvent(W.ps, b->ready, 0));
    SeqTables &T = W.T;
    T.packed = b->packed.as<uint32_t>(); T.seq_base = b->seq_base.as<uint64_t>();
    T.seq_run_first = b->seq_run_first.as<uint32_t>(); T.run_start = b->run_start.as<uint32_t>();
    T.run_len = b->run_len.as<uint32_t>(); T.nseq = (uint32_t)nseq;
    StripLists &Ls = W.Ls;
    if (P.lists) {
        Ls.slot = P.slot; Ls.ovf_base = (uint32_t)((ub_strips + 1) * P.slot); Ls.ovf_cap = P.pool;
        /* cnt[ub_strips + 1] (+ the two control words behind it), zeroed: a strip nobody lists has none */
        if ((rc = W.lcnt.alloc(c, (ub_strips + 4) * 4, psid)) || (rc = W.lent.alloc(c, ((ub_strips + 1) * P.slot + P.pool) * 4, wsid)) || (rc = W.loff.alloc(c, (ub_strips + 2) * 4))) return rc;
        window_stage_uses(W.lcnt); window_stage_uses(W.lent); /* the lists, their pool and its fail flag (Ls.ctl): this sketch's alone until the emit kernel has read them */
        W.lcnt.touch(SID_MAIN); W.lent.touch(SID_MAIN);
        Ls.cnt = W.lcnt.as<uint32_t>(); Ls.ent = W.lent.as<uint32_t>(); Ls.ctl = Ls.cnt + ub_strips + 2;
    }
    /* the fast pass's counters and lists: [0] strips for the exact pass, [1] strips the threshold pass gave up, then the eight chunk
       counters of sketch_wave_kernel (one per XCD's share of the strips, 64 bytes apart), then the two lists.  Zeroed -- with the
       strips' counts -- by strip_table_kernel: one launch instead of three fills on the window stream's critical path (round 5) */
    StripZero &Z = W.Z;
    if (P.fast() && ub_strips) {
        if ((rc = W.redo.alloc(c, (REDO_HEAD + 2 * ub_strips + 4) * 4, psid))) return rc;
        window_stage_uses(W.redo);
        Z.head = W.redo.as<uint32_t>(); Z.nhead = (uint32_t)REDO_HEAD;
        Z.cnt = Ls.cnt; Z.ncnt = Ls.cnt ? (uint32_t)(ub_strips + 4) : 0u;
    }
    W.mask.c = c;
    if (!P.lists && (rc = mask_take(c, W.nmask * 4, wsid, &W.mask))) return rc;
    if ((rc = W.strip_tab.alloc(c, (ub_strips + 1) * sizeof(StripInfo), psid)) || (rc = W.strip_lite.alloc(c, (ub_strips + 1) * sizeof(StripLite), psid))) return rc;
    window_stage_uses(W.strip_tab); window_stage_uses(W.strip_lite);
    SketchSums *dsums = s->sums.as<SketchSums>();
    /* the device sums are zeroed by strip_table_kernel (StripZero), in front of the window kernels on their stream; every kernel that
       writes them runs on MAIN behind the window stage (sketch_enqueue's event; one stream when the pipeline is off).  No sequence, no kernel: a fill */
    Z.sums = (uint32_t *)dsums; Z.nsums = (uint32_t)(sizeof(SketchSums) / 4);
    if (!nseq) HIPCHK(c, hipMemsetAsync(dsums, 0, sizeof(SketchSums), W.ms));
    ProfSpan sp(c, "sketch_meta", psid);
    if (nseq) {
        KTables K;
        K.run_n = W.run_n.as<uint32_t>(); K.run_ord = W.run_ord.as<uint32_t>();
        K.seq_M = W.seq_M.as<uint32_t>(); K.seq_nstrips = W.nstrips.as<uint32_t>();
        hipLaunchKernelGGL(seq_meta_kernel, dim3((unsigned)((nseq + 255) / 256)), dim3(256), 0, W.ps, T, K, k, w, P.G.NWO);
        HIPCHK(c, hipGetLastError());
        if ((rc = device_scan(c, W.nstrips.as<uint32_t>(), W.strip_first.as<uint32_t>(), nseq, nullptr, 1, nullptr, psid))) return rc;
        hipLaunchKernelGGL(strip_table_kernel, dim3((unsigned)((ub_strips + 255) / 256 + 1)), dim3(256), 0, W.ps, T, (const uint32_t *)K.run_n,
                           (const uint32_t *)K.run_ord, (const uint32_t *)K.seq_M, (const uint32_t *)W.strip_first.as<uint32_t>(), P.G.NWO,
                           P.C * P.nt, W.strip_tab.as<StripInfo>(), (uint32_t)ub_strips + 1u, W.strip_lite.as<StripLite>(), Z);
        HIPCHK(c, hipGetLastError());
    }
    return NTL_OK;
}

/* the k-dependent ring forms of g8 and g4 that the fast window pass reads: built once per k and context, on the window stream in front of their first user */
static int g8k_for(ntl_ctx *c, int k, hipStream_t ws, uint32_t rev_a, uint32_t rev_b, const uint2 **out)
{
    auto it = c->g8k.find(k);
    if (it == c->g8k.end()) {
        if (c->g8k.size() >= 8) { /* a caller that sweeps k: start over */
            HIPCHK(c, sync_both(c));
            for (auto &kv : c->g8k) (void)hipFree(kv.second);
            c->g8k.clear();
        }
        void *t = nullptr;
        if (hipMalloc(&t, (size_t)(2 * 65536 + 1024) * sizeof(uint2)) != hipSuccess) return fail(c, NTL_ENOMEM, "hipMalloc failed");
        hipLaunchKernelGGL(g8k_build_kernel, dim3(256), dim3(256), 0, ws, (const uint64_t (*)[2])c->g8, (uint2 *)t, rev_a, rev_b);
        hipLaunchKernelGGL(g4k_build_kernel, dim3(1), dim3(256), 0, ws, (const uint64_t (*)[2])c->g4, (uint2 *)t + 2 * 65536, rev_a, rev_b); /* the four-base form, behind it */
        HIPCHK(c, hipGetLastError());
        it = c->g8k.emplace(k, t).first;
    }
    *out = (const uint2 *)it->second;
    return NTL_OK;
}

/* The window stage: the plan's 32-bit pass, the exact pass over what it flagged (redo) and over the multi-run strips; or the exact pass alone.
   The 32-bit pass's first kernel runs on the window stream; what follows it (W.ss: the side stream, where there is one) reads and writes
   only this sketch's blocks and the slot, and is needed by nothing but this sketch's emit stage, which waits for W.last. */
static int sketch_window_stage(ntl_ctx *c, const ntl_batch *b, int k, const WindowPlan &P, ntl_sketch *s, SketchWork &W)
{
    const uint64_t ub_strips = P.strips;
    int rc;
    W.last = W.ws;
    if ((rc = SketchWork::order(c, W.ps, W.ws))) return rc; /* preparation -> window kernels */
    if (!ub_strips) return NTL_OK;
    const int wsid = W.wsid, nt = P.nt;
    SketchArgs A = {}; /* (redo_list, redo_count, redo_out: null) */
    A.T = W.T;
    A.run_n = W.run_n.as<uint32_t>(); A.run_ord = W.run_ord.as<uint32_t>(); A.seq_M = W.seq_M.as<uint32_t>();
    A.strip_lite = W.strip_lite.as<StripLite>(); A.strip_tab = W.strip_tab.as<StripInfo>(); A.nstrips = (uint32_t)ub_strips; A.mask = (uint32_t *)W.mask.p; A.G = P.G;
    make_tables(k, A.roll_tab, A.seed_tab);
    A.g4 = (const uint64_t (*)[2])c->g4; A.g8 = (const uint64_t (*)[2])c->g8;
    A.Ls = W.Ls;
    if (!P.fast()) {
        ProfSpan sp(c, "sketch_mask", wsid);
        if (P.pass == WP_SMALL) launch_small(c, A, (unsigned)ub_strips, b->any_multi);
        else if (P.C == 16) launch_mask<16>(W.ws, A, (unsigned)ub_strips, true, b->any_multi, nt);
        else if (P.C == 4) launch_mask<4>(W.ws, A, (unsigned)ub_strips, true, b->any_multi, nt);
        else launch_mask<1>(W.ws, A, (unsigned)ub_strips, true, b->any_multi, nt);
        HIPCHK(c, hipGetLastError());
        return NTL_OK;
    }
    uint32_t *const redo = W.redo.as<uint32_t>();
    Sketch2Args B = {};
    B.A = A;
    B.thresh = P.thresh; B.dbg = P.dbg; B.force_redo = P.force_redo;
    B.redo_count = redo; B.fb_count = redo + 1; B.chunk_next = redo + 16;
    B.redo_list = redo + REDO_HEAD; B.fb_list = B.redo_list + ub_strips + 2;
    B.max_word = b->nwords_packed - 1;
    B.q16 = k / 16; B.r16 = k % 16; B.rev_a = (uint32_t)(k - 1) % 33u; B.rev_b = (uint32_t)(k - 1) % 31u;
    if ((rc = g8k_for(c, k, W.ws, B.rev_a, B.rev_b, &B.g8k))) return rc;
    B.g4k = B.g8k + 2 * 65536;
    bool gave_up;
    {
        ProfSpan sp(c, "sketch_mask", wsid);
        gave_up = launch_window_pass(c, P, B);
        HIPCHK(c, hipGetLastError());
    }
    if ((rc = SketchWork::order(c, W.ws, W.ss))) return rc; /* first window kernel -> the passes over what it left */
    W.last = W.ss;
    if (gave_up) {
        ProfSpan sp(c, "sketch_mask", W.ssid);
        launch_give_up_pass(W.ss, P, B);
        HIPCHK(c, hipGetLastError());
    }
    ProfSpan sp(c, "sketch_redo", W.ssid);
    SketchArgs R = A;
    R.redo_count = B.redo_count; R.redo_list = B.redo_list;
    /* the redo pass writes the two counts into the slot (`redo` never leaves the window stage's streams); s->lz.done, on MAIN behind
       the emit kernel, is behind it too (window stage's last kernel -> emit) */
    R.redo_out = &((SketchSums *)c->pq.slot_dev(s->lz.slot))->redo_n;
    launch_mask<16>(W.ss, R, (unsigned)ub_strips, true, false, nt);
    if (b->any_multi) launch_mask<16>(W.ss, A, (unsigned)ub_strips, false, true, nt);
    HIPCHK(c, hipGetLastError());
    return NTL_OK;
}

/* Beside the window stage (two streams) the emit kernel may keep to a bounded number of resident workgroups that take their tiles from
   counters; alone: one workgroup per tile, as many resident as fit. */
struct EmitGrid { unsigned grid; bool from_counters; /* the workgroups take their tiles from tile_next */ };
static EmitGrid emit_grid(bool pipelined, int probe, bool lists, bool dense_windows, int n_cu, uint64_t tiles)
{
    /* the direct-slot form (most lookups hit: one random 64-byte line from HBM per minimizer) is bound by the rate of those
       transactions and gains nothing beyond 12 wavefronts per CU, while the slots it holds are missed by the map kernels
       and the window stage: C5 296-300 -> 269-271 ms per step at 3 workgroups per CU, 275 at 5, 280 at 4 with other window
       grids (profiles/r04_share_sweep_C5.jsonl); the tag form (C3) is as fast uncapped (74.4-75.0 against 74.9-75.9) */
    /* emit_list_kernel (44 registers, 13 KB of LDS) would fill all 32 wavefront slots of a CU, and the window stage's resident
       workgroups of the next sub-batch then wait for them to drain (C3: 91 ms per step uncapped, 75.9 at two per CU) */
    /* beside the DENSE window shapes (w < 137: twelve window wavefronts per CU, window_plan) the tag form takes four: C2
       0.890 -> 0.800 ms per step (0.806 at three, 0.815 uncapped; profiles/r07b_C2_share_sweep.txt) */
    int per_cu = !pipelined ? 0 : (probe == 2 ? 3 : (lists ? (dense_windows ? 4 : 2) : 0));
    if (const char *e = getenv("NTL_EMIT_WGS_PER_CU")) per_cu = atoi(e); /* read per call: the tests switch it inside one process */
    const uint64_t cap = (uint64_t)per_cu * (uint64_t)n_cu;
    if (per_cu > 0 && cap >= 8 && cap < tiles) return {(unsigned)cap, true};
    if (per_cu < 0) return {(unsigned)(-per_cu < 8 ? 8 : -per_cu), true}; /* tests: that many workgroups whatever the size */
    return {(unsigned)tiles, false};
}

/* the emit kernel of (lists, probe, NTL_EMIT_U, small windows): U -- minimizers in flight per thread -- comes down to a value the form has */
static void emit_launch(hipStream_t ms, unsigned grid, bool lists, int probe, bool small, const EmitArgs &E, const EmitListArgs &Q)
{
    const char *eu = getenv("NTL_EMIT_U"); /* read per call: the tests switch it inside one process */
    const int emit_u = eu ? atoi(eu) : 1;
    const dim3 g(grid);
    if (lists && probe == 0) hipLaunchKernelGGL((emit_list_kernel<0, 1>), g, dim3(EL_NT), 0, ms, E, Q);
    else if (lists) with_constant<1, 3>(probe, [&](auto p) {
        constexpr int PROBE = decltype(p)::value;
        if (emit_u >= 4) hipLaunchKernelGGL((emit_list_kernel<PROBE, 4>), g, dim3(EL_NT), 0, ms, E, Q);
        else if (emit_u >= 2) hipLaunchKernelGGL((emit_list_kernel<PROBE, 2>), g, dim3(EL_NT), 0, ms, E, Q);
        else hipLaunchKernelGGL((emit_list_kernel<PROBE, 1>), g, dim3(EL_NT), 0, ms, E, Q);
    });
    else if (probe == 0 && (eu ? emit_u >= 4 : small)) hipLaunchKernelGGL((emit_kernel<0, 4, NTL_EMIT_DENSE_CAP>), g, dim3(EMIT_NT), 0, ms, E); /* dense sketches: rounds of 8192, four k-mers' loads in flight per thread */
    else if (probe == 0 && emit_u >= 2) hipLaunchKernelGGL((emit_kernel<0, 2>), g, dim3(EMIT_NT), 0, ms, E);
    else if (probe == 0) hipLaunchKernelGGL((emit_kernel<0, 1>), g, dim3(EMIT_NT), 0, ms, E);
    else with_constant<1, 3>(probe, [&](auto p) {
        constexpr int PROBE = decltype(p)::value;
        if (emit_u >= 2) hipLaunchKernelGGL((emit_kernel<PROBE, 2>), g, dim3(EMIT_NT), 0, ms, E);
        else hipLaunchKernelGGL((emit_kernel<PROBE, 1>), g, dim3(EMIT_NT), 0, ms, E);
    });
}

/* The emit stage, on MAIN: the minimizers' ranks (a scan over the strips' list counts or the bitmask's tiles), the records (and the index lookup), the totals */
static int sketch_emit_stage(ntl_ctx *c, const ntl_batch *b, int k, const WindowPlan &P, const ntl_index *ix, ntl_sketch *s, uint64_t cap, SketchWork &W)
{
    const bool lists = P.lists;
    const uint64_t nseq = b->nseq, ub_strips = P.strips, nmask = W.nmask;
    hipStream_t ms = W.ms;
    const StripLists &Ls = W.Ls;
    SketchSums *dsums = s->sums.as<SketchSums>();
    int rc;
    ProfSpan sp(c, "sketch_emit");
    const uint64_t tiles = lists ? (ub_strips + EL_STRIPS - 1) / EL_STRIPS : (nmask + EMIT_TILE - 1) / EMIT_TILE;
    DevBuf tile_seq, tile_next;
    if ((rc = tile_next.alloc(c, 8 * 16 * 4))) return rc;
    if (lists) {
        /* ranks: a scan over one count per strip; the total (or, if the lists ran out of pool, a total no array holds: the map
           kernels leave such a sketch alone and sketch_finalize makes it again through the bitmask) */
        W.strip_first.touch(SID_MAIN); W.strip_tab.touch(SID_MAIN);
        if ((rc = device_scan(c, Ls.cnt, W.loff.as<uint32_t>(), ub_strips, nullptr, 1, &dsums->total_mx))) return rc;
        SketchSums *hd = (SketchSums *)c->pq.slot_dev(s->lz.slot); /* the true total and whether the lists ran out, for the host */
        hipLaunchKernelGGL(list_fail_kernel, dim3(1), dim3(64), 0, ms, (const uint32_t *)Ls.ctl, &dsums->total_mx, &dsums->list_fail, tile_next.as<uint32_t>(),
                           &hd->total_mx, &hd->list_fail);
        hipLaunchKernelGGL(mx_off_from_strips_kernel, dim3((unsigned)((nseq + 256) / 256)), dim3(256), 0, ms, (const uint32_t *)W.strip_first.as<uint32_t>(),
                           (const uint32_t *)W.loff.as<uint32_t>(), (uint32_t)nseq, s->mx_off.as<uint32_t>());
    } else {
        if ((rc = W.tile.alloc(c, tiles * 4)) || (rc = tile_seq.alloc(c, (tiles + 2) * 4))) return rc;
        if (nseq)
            hipLaunchKernelGGL(tile_seq_kernel, dim3((unsigned)((nseq + 255) / 256)), dim3(256), 0, ms, (const uint64_t *)W.T.seq_base, (uint32_t)nseq, tiles, tile_seq.as<uint32_t>());
        hipLaunchKernelGGL(mask_count_kernel, dim3((unsigned)tiles), dim3(EMIT_NT), 0, ms, (const uint32_t *)W.mask.p, nmask, W.tile.as<uint32_t>(), tile_next.as<uint32_t>());
        hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(SCAN_NT), 0, ms, W.tile.as<uint32_t>(), tiles, &dsums->total_mx, (uint64_t)0, (uint32_t *)nullptr);
    }
    HIPCHK(c, hipGetLastError());
    if (!s->no_records && (rc = s->records.alloc(c, cap * sizeof(MxRecord)))) return rc;
    s->cap = cap;
    const int probe = !ix ? 0 : (ix->hit_fraction->load(std::memory_order_relaxed) <= 0.5f ? 1 : 2); /* tags first unless the last batch on this index mostly hit */
    if (ix) {
        if ((rc = s->rpos.alloc(c, cap * 4)) || (rc = s->cand.alloc(c, cap * sizeof(Cand)))) return rc;
        s->cand_gen = ix->gen;
        if (ix->c != c && ix->built) HIPCHK(c, hipStreamWaitEvent(ms, ix->built, 0));
    }
    EmitArgs E = {};
    E.packed = W.T.packed; E.seq_base = W.T.seq_base; E.nseq = (uint32_t)nseq; E.mask = (uint32_t *)W.mask.p;
    E.nwords = nmask; E.tile_off = W.tile.as<uint32_t>(); E.tile_seq = tile_seq.as<uint32_t>(); E.mx_off = s->mx_off.as<uint32_t>();
    E.out = s->no_records ? nullptr : s->records.as<MxRecord>(); E.out_cap = (uint32_t)cap;
    E.k = k; E.mult = 1ull ^ ((uint64_t)k * 0x90b45d39fb6da1faull);
    uint64_t roll[16][2];
    make_tables(k, roll, E.seed_tab);
    E.g4 = (const uint64_t (*)[2])c->g4; E.g8 = (const uint64_t (*)[2])c->g8;
    if (ix) { /* (else no lookup: those pointers stay null) */
        E.rpos = s->rpos.as<uint32_t>();
        E.slots = ix->slots.as<IndexSlot>(); E.tags = ix->tags.as<uint8_t>(); E.special = ix->special.as<IndexSpecial>();
        E.ix_bits = ix->bits; E.cand = s->cand.as<Cand>(); E.nfound = &dsums->nfound;
    }
    const EmitGrid eg = emit_grid(c->pipelined, probe, lists, P.dense_windows, c->n_cu, tiles);
    E.ntiles = (uint32_t)tiles; E.tile_next = eg.from_counters ? tile_next.as<uint32_t>() : nullptr;
    EmitListArgs Q = {};
    if (lists) { Q.Ls = Ls; Q.strip_tab = W.strip_tab.as<StripInfo>(); Q.strip_off = W.loff.as<uint32_t>(); Q.nstrips = (uint32_t)ub_strips; }
    emit_launch(ms, eg.grid, lists, probe, P.pass == WP_SMALL, E, Q);
    HIPCHK(c, hipGetLastError());
    /* the emit kernel is the last reader of the bitmask and clears the words it read: the mask goes back clean */
    if (W.mask.p) {
        CleanMask m = W.mask;
        m.clean = c->pq.event_get();
        if (m.clean) HIPCHK(c, hipEventRecord(m.clean, ms));
        else HIPCHK(c, hipStreamSynchronize(ms));
        c->masks.push_back(m);
        W.mask.p = nullptr; /* handed over */
    }
    /* (the map kernels read the lengths of the sketched sequences from the batch itself: ntl_map_run holds it) */
    s->nfound_owed = false;
    if (!lists) { /* the bitmask path (off the hot path): the totals come back by copies */
        SketchSums *hs = (SketchSums *)s->lz.slot;
        HIPCHK(c, hipMemcpyAsync(&hs->total_mx, &dsums->total_mx, 4, hipMemcpyDeviceToHost, ms));
        if (ix) HIPCHK(c, hipMemcpyAsync(&hs->nfound, &dsums->nfound, 8, hipMemcpyDeviceToHost, ms));
    } else s->nfound_owed = ix != nullptr; /* (list_fail_kernel wrote the total and the flag) */
    return NTL_OK;
}

/* Queues one sketch: the window stage on the window stream, count + emit (+ index lookup) on MAIN behind it.  Nothing
 * waits; the minimizer total lands in the sketch's page-locked slot and s->lz.done is recorded behind it.  `cap` = records the
 * arrays hold: a guess from the expected density (sketch_finalize makes the sketch again if the batch was denser), or the
 * exact total on that second round. */
static int sketch_enqueue(ntl_ctx *c, const ntl_batch *b, int k, int w, const ntl_index *ix, ntl_sketch *s, uint64_t cap)
{
    /* the host runs at most 8 sketches ahead of the device */
    hipEvent_t &throttle = c->throttle[c->n_enqueued & 7u];
    if (throttle) (void)hipEventSynchronize(throttle);
    c->pq.reap(false);
    WindowPlan P;
    int rc;
    if ((rc = window_plan(c, b, k, w, s->no_lists, P))) return rc;
    SketchWork W;
    W.wsid = c->sid(SID_W); W.ws = c->s(W.wsid); W.ms = c->stream;
    W.ssid = c->sid(SID_S); W.ss = c->s(W.ssid);
    W.psid = c->side_prep ? W.ssid : W.wsid; W.ps = c->s(W.psid);
    if ((rc = sketch_prepare(c, b, k, w, P, s, W))) return rc;
    if ((rc = sketch_window_stage(c, b, k, P, s, W))) return rc;
    if ((rc = SketchWork::order(c, W.last, W.ms))) return rc; /* window stage -> emit */
    if ((rc = sketch_emit_stage(c, b, k, P, ix, s, cap, W))) return rc;
    /* "lists complete" reaches the handle and the throttle through MAIN: both events are recorded behind the emit kernel, which waited for
       the side stream's last pass -- the host never runs further ahead of the give-up passes than of the emit kernels */
    HIPCHK(c, hipEventRecord(s->lz.done, W.ms));
    if (!throttle) throttle = c->pq.event_get();
    if (throttle) HIPCHK(c, hipEventRecord(throttle, W.ms));
    c->n_enqueued++;
    s->strips = P.strips; s->from_lists = P.lists;
    ntl_plan_info &I = s->plan; /* the plan that was carried out, as plain integers (ntl_sketch_plan) */
    memset(&I, 0, sizeof I);
    I.pass = (int32_t)P.pass; I.nt = P.nt; I.C = P.C; I.NWO = P.G.NWO;
    I.big = P.big; I.direct = P.direct; I.lists = P.lists; I.thresh = P.thresh;
    if (P.pass == WP_WAVE) wave_shape_numbers(P.shape, &I.wave_wavefronts);
    s->lz.pending = true;
    return NTL_OK; /* (W's temporaries return to the context's cache here) */
}

static int sketch_run_impl(ntl_ctx *c, const ntl_batch *b, int k, int w, const ntl_index *ix, ntl_sketch **out, bool no_records = false)
{
    if (!c || !b || !out) return NTL_EINVAL;
    *out = nullptr;
    (void)hipSetDevice(c->device);
    SketchGeom G;
    int C, nt, rc; bool small;
    if ((rc = sketch_geometry(c, k, w, G, C, nt, small))) return rc; /* (a window this build cannot sketch: refused before anything is made) */
    ntl_sketch *s = new ntl_sketch();
    s->c = c; s->nseq = b->nseq; s->k = k; s->w = w;
    s->no_records = no_records && ix;
    if (ix) { ix->refs++; s->lz.holds[0] = {ix, hold_index}; }
    if (!s->lz.arm(c->pq)) { sketch_unref(s); return fail(c, NTL_EDEVICE, "out of events / page-locked slots"); }
    /* The record array is sized from the expected density before the count is known (the device goes straight on to the
       emit kernel); a batch denser than the guess (low-complexity sequence) is sketched a second time into exact-size
       arrays when its count is asked for (sketch_finalize). */
    uint64_t cap_guess = (uint64_t)(2.5 * (double)b->bases / (double)(w + 1)) + 65536;
    if (cap_guess > b->bases + 1) cap_guess = b->bases + 1;
    if (cap_guess > 0xFFFFFFF0ull) cap_guess = 0xFFFFFFF0ull;
    if (const char *e = getenv("NTL_SKETCH_CAP_GUESS")) cap_guess = (uint64_t)atoll(e); /* tests: force the second round */
    const_cast<ntl_batch *>(b)->refs++;
    s->src = b;
    if ((rc = sketch_enqueue(c, b, k, w, ix, s, cap_guess))) {
        pending_abort(c, s->lz, rc);
        sketch_unref(s);
        return rc;
    }
    *out = s;
    return NTL_OK;
}

/* Completes a sketch: waits for its event, reads the totals, and -- when the batch held more minimizers than the arrays
 * that were sized from the expected density -- makes the sketch again with exact-size arrays (same minimizers). */
static int sketch_finalize(const ntl_sketch *cs)
{
    ntl_sketch *s = const_cast<ntl_sketch *>(cs);
    Pending &lz = s->lz;
    if (!lz.pending) return lz.failed;
    ntl_ctx *c = s->c;
    (void)hipSetDevice(c->device);
    for (int round = 0;; round++) {
        if (s->nfound_owed) { /* no map kernel took the hit count: a kernel of its own, behind the lookup, and the event behind that */
            s->nfound_owed = false;
            hipLaunchKernelGGL(sketch_nfound_kernel, dim3(1), dim3(64), 0, c->stream, (const unsigned long long *)&s->sums.as<SketchSums>()->nfound,
                               &((SketchSums *)c->pq.slot_dev(lz.slot))->nfound);
            hipError_t le = hipGetLastError();
            if (le == hipSuccess) le = hipEventRecord(lz.done, c->stream);
            if (le != hipSuccess) { pending_abort(c, lz, fail(c, NTL_EDEVICE, std::string("sketch: ") + hipGetErrorString(le))); break; }
        }
        const hipError_t e = lz.wait();
        lz.pending = false;
        if (e != hipSuccess) { lz.failed = fail(c, NTL_EDEVICE, std::string("sketch: ") + hipGetErrorString(e)); break; }
        const SketchSums hs = *(const SketchSums *)lz.slot;
        s->count = hs.total_mx; s->redo_strips = hs.redo_n; s->fallback_strips = hs.fb_n; s->nfound = hs.nfound;
        if (s->count <= s->cap && !hs.list_fail) break;
        if (round || !s->src) { lz.failed = fail(c, NTL_EINTERNAL, "sketch: the exact-size round overflowed again"); break; }
        if (hs.list_fail) s->no_lists = true; /* the strips' lists ran out of pool (the counts are right): once more, through the bitmask */
        s->gen++;
        memset(lz.slot, 0, sizeof(PinSlot));
        const int rc = sketch_enqueue(c, s->src, s->k, s->w, (const ntl_index *)lz.holds[0].p, s, s->count);
        if (rc) { pending_abort(c, lz, rc); break; }
    }
    if (s->src) { batch_unref(s->src); s->src = nullptr; }
    /* complete: what only a pending sketch needs goes back now, not when the handle is destroyed -- a context has NTL_NSLOTS
       page-locked slots, and callers keep thousands of completed sketches alive */
    lz.settle(c->pq);
    return lz.failed;
}

extern "C" int ntl_sketch_run(ntl_ctx *c, const ntl_batch *b, int k, int w, ntl_sketch **out)
{
    return sketch_run_impl(c, b, k, w, nullptr, out);
}

/* The same sketch made FOR one contig index: every minimizer is looked up in `ix` while it is emitted, and ntl_map_run on
 * (ix, this sketch) skips its own lookup pass over the records.  The minimizers are those of ntl_sketch_run. */
extern "C" int ntl_sketch_run_indexed(ntl_ctx *c, const ntl_batch *b, int k, int w, const ntl_index *ix, ntl_sketch **out)
{
    if (!ix) return NTL_EINVAL;
    if (ix->c->device != c->device) return fail(c, NTL_EINVAL, "the index lives on another device");
    return sketch_run_impl(c, b, k, w, ix, out);
}

/* ... and made ONLY for ntl_map_run(ix, this sketch): the 16-byte records are never written (a minimizer leaves its position in
 * the read and its candidate: 12 bytes instead of 24 written here and read by the map kernels).  Everything that needs the records
 * (download, index build, overlap filter, a map against another index) answers NTL_EINVAL. */
extern "C" int ntl_sketch_run_for_map(ntl_ctx *c, const ntl_batch *b, int k, int w, const ntl_index *ix, ntl_sketch **out)
{
    if (!ix) return NTL_EINVAL;
    if (ix->c->device != c->device) return fail(c, NTL_EINVAL, "the index lives on another device");
    return sketch_run_impl(c, b, k, w, ix, out, true);
}

extern "C" int ntl_sketch_has_records(const ntl_sketch *s) { return s && !s->no_records; }

extern "C" void ntl_sketch_destroy(ntl_sketch *s) { sketch_unref(s); }
extern "C" int ntl_sketch_wait(const ntl_sketch *s) { return s ? sketch_finalize(s) : NTL_EINVAL; }
extern "C" uint64_t ntl_sketch_nseq(const ntl_sketch *s) { return s ? s->nseq : 0; }
extern "C" uint64_t ntl_sketch_count(const ntl_sketch *s) { return s && sketch_finalize(s) == NTL_OK ? s->count : 0; }
extern "C" uint64_t ntl_sketch_strips(const ntl_sketch *s) { return s ? s->strips : 0; }
extern "C" uint64_t ntl_sketch_redo_strips(const ntl_sketch *s) { return s && sketch_finalize(s) == NTL_OK ? s->redo_strips : 0; }
extern "C" int ntl_sketch_from_lists(const ntl_sketch *s) { return s && sketch_finalize(s) == NTL_OK && s->from_lists ? 1 : 0; }
extern "C" uint64_t ntl_sketch_fallback_strips(const ntl_sketch *s) { return s && sketch_finalize(s) == NTL_OK ? s->fallback_strips : 0; }
static_assert(WP_SMALL == NTL_PASS_SMALL && WP_EXACT_ONLY == NTL_PASS_EXACT_ONLY && WP_BLOCK_MINIMA == NTL_PASS_BLOCK_MINIMA &&
              WP_THRESH == NTL_PASS_THRESH && WP_WAVE == NTL_PASS_WAVE, "WindowPass is ntl_plan_info's `pass`");
extern "C" int ntl_sketch_plan(const ntl_sketch *s, ntl_plan_info *out)
{
    if (!s || !out) return NTL_EINVAL;
    const int rc = sketch_finalize(s); /* (a sketch that overflowed is made again there: the plan is the last round's) */
    if (rc == NTL_OK) *out = s->plan;
    return rc;
}

extern "C" int ntl_sketch_download(const ntl_sketch *s, uint64_t *mx_off, uint64_t *hash, uint32_t *pos, uint8_t *strand)
{
    if (!s) return NTL_EINVAL;
    ntl_ctx *c = s->c;
    (void)hipSetDevice(c->device);
    int rc = sketch_finalize(s);
    if (rc) return rc;
    if (s->no_records && (hash || pos || strand)) return fail(c, NTL_EINVAL, "a sketch made by ntl_sketch_run_for_map holds no records");
    const size_t off_bytes = ((s->nseq + 1) * 4 + 63) & ~(size_t)63;
    void *tmp = nullptr;
    if ((rc = host_tmp(c, off_bytes + (s->no_records ? 0 : s->count * sizeof(MxRecord)), &tmp))) return rc;
    const uint32_t *off = (const uint32_t *)tmp;
    const MxRecord *rec = (const MxRecord *)((const char *)tmp + off_bytes);
    HIPCHK(c, hipMemcpyAsync(tmp, s->mx_off.p, (s->nseq + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    if (s->count && !s->no_records) HIPCHK(c, hipMemcpyAsync((void *)rec, s->records.p, s->count * sizeof(MxRecord), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (mx_off) for (uint64_t i = 0; i <= s->nseq; i++) mx_off[i] = off[i];
    if (s->no_records) return NTL_OK;
    /* records -> the caller's column arrays, split over threads */
    unsigned nthr = std::thread::hardware_concurrency();
    nthr = nthr == 0 ? 1 : std::min(nthr, 16u);
    if (s->count < (1u << 18)) nthr = 1;
    auto work = [&](uint64_t a, uint64_t b) {
        for (uint64_t i = a; i < b; i++) {
            if (hash) hash[i] = rec[i].hash;
            if (pos) pos[i] = rec[i].pos;
            if (strand) strand[i] = (uint8_t)(rec[i].meta & 1u);
        }
    };
    if (nthr == 1) work(0, s->count);
    else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nthr; t++) th.emplace_back(work, s->count * t / nthr, s->count * (t + 1) / nthr);
        for (auto &x : th) x.join();
    }
    return NTL_OK;
}

extern "C" int ntl_sketch_from_host(ntl_ctx *c, uint64_t nseq, const uint64_t *mx_off, const uint64_t *hash,
                                    const uint32_t *pos, const uint8_t *strand, ntl_sketch **out)
{
    if (!c || !out || !mx_off) return NTL_EINVAL;
    *out = nullptr;
    const uint64_t n = mx_off[nseq];
    if (n >= 0xFFFFFFF0ull || nseq >= ((uint64_t)1 << 31)) return fail(c, NTL_EINVAL, "sketch too large for one batch");
    if (n && (!hash || !pos || !strand)) return NTL_EINVAL;
    (void)hipSetDevice(c->device);
    if (mx_off[0] != 0) return fail(c, NTL_EINVAL, "mx_off[0] must be 0");
    for (uint64_t i = 1; i <= nseq; i++)
        if (mx_off[i] < mx_off[i - 1]) return fail(c, NTL_EINVAL, "mx_off must be non-decreasing");
    /* columns -> 16-byte records in the page-locked bounce buffer, sequences split over threads */
    const size_t off_bytes = ((nseq + 1) * 4 + 63) & ~(size_t)63;
    void *tmp = nullptr;
    int rc = host_tmp(c, off_bytes + n * sizeof(MxRecord), &tmp);
    if (rc) return rc;
    uint32_t *off = (uint32_t *)tmp;
    MxRecord *rec = (MxRecord *)((char *)tmp + off_bytes);
    unsigned nthr = std::thread::hardware_concurrency();
    nthr = nthr == 0 ? 1 : std::min(nthr, 16u);
    if (n < (1u << 18)) nthr = 1;
    auto work = [&](uint64_t s0, uint64_t s1) {
        for (uint64_t s = s0; s < s1; s++) {
            off[s] = (uint32_t)mx_off[s];
            for (uint64_t i = mx_off[s]; i < mx_off[s + 1]; i++) {
                rec[i].hash = hash[i]; rec[i].pos = pos[i];
                rec[i].meta = ((uint32_t)s << 1) | (strand[i] ? 1u : 0u);
            }
        }
    };
    if (nthr == 1) work(0, nseq);
    else {
        std::vector<std::thread> th;
        std::vector<uint64_t> cut(nthr + 1, nseq); /* about equal numbers of minimizers per thread */
        cut[0] = 0;
        for (unsigned t = 1; t < nthr; t++)
            cut[t] = std::max<uint64_t>(cut[t - 1], (uint64_t)(std::lower_bound(mx_off, mx_off + nseq, n * t / nthr) - mx_off));
        for (unsigned t = 0; t < nthr; t++) th.emplace_back(work, cut[t], cut[t + 1]);
        for (auto &x : th) x.join();
    }
    off[nseq] = (uint32_t)mx_off[nseq];
    std::unique_ptr<ntl_sketch> sk(new ntl_sketch());
    sk->c = c; sk->nseq = nseq; sk->count = n; sk->cap = n;
    if ((rc = sk->records.alloc(c, n * sizeof(MxRecord))) || (rc = sk->mx_off.alloc(c, (nseq + 1) * 4))) return rc;
    hipError_t e = hipSuccess;
    if (n) e = hipMemcpyAsync(sk->records.p, rec, n * sizeof(MxRecord), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sk->mx_off.p, off, (nseq + 1) * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, NTL_EDEVICE, hipGetErrorString(e));
    *out = sk.release();
    return NTL_OK;
}


/* ------------------------------------------------------------------ overlap-stage consumer -- */

/* read_minimizer_line of bin/ntlink_overlap_sequences.py:170-190 over a device-resident sketch (overlap_kernels.h):
 * valid-region filter, per-sequence removal of every hash that occurs more than once, dense result in input order. */
extern "C" int ntl_overlap_filter(ntl_ctx *c, const ntl_sketch *s, const uint64_t *region_off, const uint32_t *region_start,
                                  const uint32_t *region_end, ntl_sketch **out)
{
    if (!c || !s || !region_off || !out) return NTL_EINVAL;
    *out = nullptr;
    (void)hipSetDevice(c->device);
    if (s->no_records) return fail(c, NTL_EINVAL, "a sketch made by ntl_sketch_run_for_map holds no records");
    if (int frc = sketch_finalize(s)) return frc;
    const uint64_t nseq = s->nseq, n = s->count;
    const uint64_t nreg = region_off[nseq];
    if (region_off[0] != 0) return fail(c, NTL_EINVAL, "region_off[0] must be 0");
    for (uint64_t i = 0; i < nseq; i++)
        if (region_off[i + 1] < region_off[i]) return fail(c, NTL_EINVAL, "region_off must be non-decreasing");
    if (nreg >= 0xFFFFFFF0ull) return fail(c, NTL_EINVAL, "too many regions");
    if (nreg && (!region_start || !region_end)) return NTL_EINVAL;
    (void)hipSetDevice(c->device);
    std::unique_ptr<ntl_sketch> o(new ntl_sketch());
    o->c = c; o->nseq = nseq;
    int rc;
    DevBuf roff, rs, re, slots, dup, side, keep, dst;
    std::vector<uint32_t> roff32(nseq + 1);
    for (uint64_t i = 0; i <= nseq; i++) roff32[i] = (uint32_t)region_off[i];
    if ((rc = roff.alloc(c, (nseq + 1) * 4)) || (rc = rs.alloc(c, (nreg + 1) * 4)) || (rc = re.alloc(c, (nreg + 1) * 4)) ||
        (rc = slots.alloc(c, (2 * n + 1) * 8)) || (rc = dup.alloc(c, (2 * n / 32 + 2) * 4)) || (rc = side.alloc(c, (nseq + 1) * 4)) ||
        (rc = keep.alloc(c, (n + 1) * 4)) || (rc = dst.alloc(c, (n + 2) * 4)) || (rc = o->mx_off.alloc(c, (nseq + 1) * 4)))
        return rc;
    uint32_t total = 0;
    {
        ProfSpan sp(c, "overlap_filter");
        HIPCHK(c, hipMemcpyAsync(roff.p, roff32.data(), (nseq + 1) * 4, hipMemcpyHostToDevice, c->stream));
        if (nreg) {
            HIPCHK(c, hipMemcpyAsync(rs.p, region_start, nreg * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(re.p, region_end, nreg * 4, hipMemcpyHostToDevice, c->stream));
        }
        HIPCHK(c, hipMemsetAsync(slots.p, 0xFF, (2 * n + 1) * 8, c->stream)); /* NTL_INF = empty */
        HIPCHK(c, hipMemsetAsync(dup.p, 0, (2 * n / 32 + 2) * 4, c->stream));
        HIPCHK(c, hipMemsetAsync(side.p, 0, (nseq + 1) * 4, c->stream));
        HIPCHK(c, hipMemsetAsync(keep.p, 0, (n + 1) * 4, c->stream));
        OvlArgs A;
        A.rec = s->records.as<MxRecord>(); A.n = n; A.mx_off = s->mx_off.as<uint32_t>();
        A.reg_off = roff.as<uint32_t>(); A.reg_start = rs.as<uint32_t>(); A.reg_end = re.as<uint32_t>();
        A.slots = slots.as<unsigned long long>(); A.dupbits = dup.as<uint32_t>(); A.side = side.as<uint32_t>();
        A.keep = keep.as<uint32_t>();
        const unsigned grid = (unsigned)((n + 255) / 256);
        if (n) {
            hipLaunchKernelGGL(ovl_insert_kernel, dim3(grid), dim3(256), 0, c->stream, A);
            hipLaunchKernelGGL(ovl_resolve_kernel, dim3(grid), dim3(256), 0, c->stream, A);
            HIPCHK(c, hipGetLastError());
        }
        /* the one wait of the call: the number of kept records sizes the result */
        if ((rc = device_scan(c, keep.as<uint32_t>(), dst.as<uint32_t>(), n, &total))) return rc;
        o->count = total; o->cap = total;
        if ((rc = o->records.alloc(c, (uint64_t)total * sizeof(MxRecord)))) return rc;
        const uint64_t work = std::max<uint64_t>(n, nseq + 1);
        hipLaunchKernelGGL(ovl_gather_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, c->stream,
                           (const MxRecord *)s->records.as<MxRecord>(), n, (const uint32_t *)keep.as<uint32_t>(),
                           (const uint32_t *)dst.as<uint32_t>(), o->records.as<MxRecord>(), (const uint32_t *)s->mx_off.as<uint32_t>(),
                           (uint32_t)nseq, o->mx_off.as<uint32_t>());
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipStreamSynchronize(c->stream)); /* roff32 and the caller's region arrays are free again */
    *out = o.release();
    return NTL_OK;
}

static_assert(sizeof(ntl_overlap_pair) == sizeof(OvcPair) && sizeof(OvcPair) == 40 && sizeof(ntl_overlap_cut) == sizeof(OvcCut) && sizeof(OvcCut) == 32,
              "ABI records must match the device records");
static_assert(NTL_OVERLAP_CUT == OVC_CUT && NTL_OVERLAP_GLOBAL == OVC_GLOBAL && NTL_OVERLAP_LDS_SLICE == OVC_LDS_SLICE &&
              NTL_OVERLAP_SRC_MINUS == OVC_SRC_MINUS && NTL_OVERLAP_TGT_MINUS == OVC_TGT_MINUS, "constants of the ABI and of overlap_cut_kernels.h");

/* merge_overlapping of bin/ntlink_overlap_sequences.py:341-417 for every pair at once (overlap_cut_kernels.h).  One wait when every
   target slice fits the LDS table; a second one behind the overflow kernel, whose scratch is sized by the first. */
extern "C" int ntl_overlap_cuts(ntl_ctx *c, const ntl_sketch *s, const ntl_overlap_pair *pairs, uint64_t n_pairs, ntl_overlap_cut *out)
{
    if (!c || !s || (n_pairs && (!pairs || !out))) return NTL_EINVAL;
    (void)hipSetDevice(c->device);
    if (s->c->device != c->device) return fail(c, NTL_EINVAL, "ntl_overlap_cuts: the sketch lives on another device");
    if (s->no_records) return fail(c, NTL_EINVAL, "a sketch made by ntl_sketch_run_for_map holds no records");
    if (int frc = sketch_finalize(s)) return frc;
    if (n_pairs >= ((uint64_t)1 << 31)) return fail(c, NTL_EINVAL, "ntl_overlap_cuts: too many pairs for one call");
    for (uint64_t i = 0; i < n_pairs; i++) {
        const ntl_overlap_pair &P = pairs[i];
        if (P.src >= s->nseq || P.tgt >= s->nseq)
            return fail(c, NTL_EINVAL, "ntl_overlap_cuts: pair " + std::to_string(i) + " names a sequence the sketch does not hold");
        if (P.src_start > P.src_end || P.tgt_start > P.tgt_end)
            return fail(c, NTL_EINVAL, "ntl_overlap_cuts: pair " + std::to_string(i) + " has a region that starts behind its end");
    }
    if (!n_pairs) return NTL_OK;
    DevBuf dpairs, dout, list, info, scratch;
    int rc;
    if ((rc = dpairs.alloc(c, n_pairs * sizeof(OvcPair))) || (rc = dout.alloc(c, n_pairs * sizeof(OvcCut))) || (rc = list.alloc(c, n_pairs * 4)) ||
        (rc = info.alloc(c, 16)))
        return rc;
    OvcArgs A = {};
    A.rec = s->records.as<MxRecord>(); A.mx_off = s->mx_off.as<uint32_t>(); A.pairs = dpairs.as<OvcPair>(); A.n_pairs = (uint32_t)n_pairs;
    A.out = dout.as<OvcCut>(); A.over_list = list.as<uint32_t>(); A.info = info.as<uint32_t>();
    uint32_t hinfo[4] = {0, 0, 0, 0};
    {
        ProfSpan sp(c, "overlap_cut");
        HIPCHK(c, hipMemcpyAsync(dpairs.p, pairs, n_pairs * sizeof(OvcPair), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(info.p, 0, 16, c->stream));
        hipLaunchKernelGGL(overlap_cut_kernel, dim3((unsigned)n_pairs), dim3(OVC_NT), 0, c->stream, A);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(hinfo, info.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out, dout.p, n_pairs * sizeof(OvcCut), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, main_wait(c));
    if (hinfo[0]) { /* target slices above OVC_LDS_SLICE: the same body over global scratch, sized now that the longest is known */
        const unsigned blocks = std::min<uint32_t>(hinfo[0], OVC_OVER_BLOCKS);
        A.slab_cap = hinfo[1];
        A.slab_bytes = ((uint64_t)OVC_SLAB_BYTES_PER_MX * hinfo[1] + 255) & ~(uint64_t)255;
        if ((rc = scratch.alloc(c, A.slab_bytes * blocks))) return rc;
        A.scratch = scratch.as<uint8_t>();
        {
            ProfSpan sp(c, "overlap_cut_overflow");
            hipLaunchKernelGGL(overlap_cut_overflow_kernel, dim3(blocks), dim3(OVC_NT), 0, c->stream, A);
            HIPCHK(c, hipGetLastError());
        }
        HIPCHK(c, hipMemcpyAsync(hinfo, info.p, 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(out, dout.p, n_pairs * sizeof(OvcCut), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, main_wait(c));
    }
    if (hinfo[2]) return fail(c, NTL_EINTERNAL, "ntl_overlap_cuts: a pair's slices broke the sketch's contract (a hash twice in one sequence, or a probe sequence without an end)");
    return NTL_OK;
}

/* ------------------------------------------------------------------ path chains ---------- */

static_assert(sizeof(ntl_path_edge) == sizeof(PathEdge) && sizeof(PathEdge) == 20 && sizeof(ntl_path_link) == sizeof(PathLink) &&
              sizeof(ntl_path_counts) == sizeof(PathInfo) && sizeof(PathInfo) == 32, "ABI records must match the device records");
static_assert(NTL_PATH_EDGE_NEW == PATH_EDGE_NEW && NTL_PATH_CONSERVATIVE == PATH_MODE_CONSERVATIVE && NTL_PATH_STITCH == PATH_MODE_STITCH &&
              NTL_PATH_TRANSITIVE == PATH_MODE_TRANSITIVE, "constants of the ABI and of path_kernels.h");

/* the ranking of the linear graph as it stands -> the buffer that holds it */
static int path_rank(ntl_ctx *c, const PathArgs &A, unsigned grid, int rounds)
{
    hipLaunchKernelGGL(path_rank_init_kernel, dim3(grid), dim3(PATH_NT), 0, c->stream, A);
    int at = 0;
    for (int r = 0; r < rounds; r++, at ^= 1) hipLaunchKernelGGL(path_rank_round_kernel, dim3(grid), dim3(PATH_NT), 0, c->stream, A, at);
    return at;
}

/* linearize_graph .. remove_duplicate_paths of bin/ntlink_stitch_paths.py:221-365 (path_kernels.h): launches sized by the caller's
   counts alone -- the doubling rounds by n_vertices -- and ONE wait behind them, for the counts, the error word and the chains.
   In front of the first launch the host checks every edge's and link's vertex numbers, a serial pass over the caller's arrays. */
extern "C" int ntl_path_chains(ntl_ctx *c, uint32_t n_vertices, const ntl_path_edge *edges, uint64_t n_edges, const ntl_path_link *links,
                               uint64_t n_links, uint32_t mode, uint32_t *chain_off, uint32_t *chain_vertex, int32_t *chain_d,
                               ntl_path_counts *counts)
{
    if (!c || !counts || !chain_off || (n_edges && !edges) || (n_links && !links) || (n_vertices && (!chain_vertex || !chain_d))) return NTL_EINVAL;
    (void)hipSetDevice(c->device);
    memset(counts, 0, sizeof(*counts));
    chain_off[0] = 0;
    if (mode > PATH_MODE_TRANSITIVE) return fail(c, NTL_EINVAL, "ntl_path_chains: mode " + std::to_string(mode) + " is none of conservative, stitch, stitch + transitive");
    if (n_vertices & 1u) return fail(c, NTL_EINVAL, "ntl_path_chains: n_vertices is odd (a vertex and its twin are 2 * contig and 2 * contig + 1)");
    if (n_vertices >= (1u << 31) || n_edges >= ((uint64_t)1 << 30) || n_links >= ((uint64_t)1 << 31))
        return fail(c, NTL_EINVAL, "ntl_path_chains: too many vertices, edges or scaffold-graph edges for one call");
    for (uint64_t i = 0; i < n_edges; i++) {
        if (edges[i].src >= n_vertices || edges[i].tgt >= n_vertices)
            return fail(c, NTL_EINVAL, "ntl_path_chains: edge " + std::to_string(i) + " names a vertex beyond n_vertices");
        if (edges[i].flags & ~PATH_EDGE_NEW) return fail(c, NTL_EINVAL, "ntl_path_chains: edge " + std::to_string(i) + " has unknown flags");
    }
    if (mode != PATH_MODE_TRANSITIVE) n_links = 0; /* the scaffold graph counts for the transitive filter only */
    for (uint64_t i = 0; i < n_links; i++)
        if (links[i].a >= n_vertices || links[i].b >= n_vertices)
            return fail(c, NTL_EINVAL, "ntl_path_chains: scaffold-graph edge " + std::to_string(i) + " names a vertex beyond n_vertices");
    if (!n_vertices) return NTL_OK;
    const uint64_t V = n_vertices;
    int slot_bits = 4, rounds = 0;
    while (((uint64_t)1 << slot_bits) < 2 * n_edges + 2) slot_bits++;
    while (((uint64_t)1 << rounds) < V) rounds++;
    const uint64_t n_slots = (uint64_t)1 << slot_bits;
    DevBuf dedges, dlinks, slots, slot_edge, sides, graph, words, mins, scans, outs, info;
    int rc;
    /* sides: deg, notnew, maxn, cntmax, kept_deg [2V each]; graph: next, prev (0xFF) | vnew, sup, vd, head_of; outs: vertex, d [V], off */
    if ((rc = dedges.alloc(c, (n_edges + 1) * sizeof(PathEdge))) || (rc = dlinks.alloc(c, (n_links + 1) * sizeof(PathLink))) ||
        (rc = slots.alloc(c, n_slots * 8)) || (rc = slot_edge.alloc(c, n_slots * 4)) || (rc = sides.alloc(c, 10 * V * 4)) ||
        (rc = graph.alloc(c, 6 * V * 4)) || (rc = words.alloc(c, 2 * V * 8)) || (rc = mins.alloc(c, 2 * V * 4)) ||
        (rc = scans.alloc(c, 2 * (V + 1) * 4)) || (rc = outs.alloc(c, (2 * V + V / 2 + 1) * 4)) || (rc = info.alloc(c, sizeof(PathInfo))))
        return rc;
    PathArgs A = {};
    A.n_vertices = n_vertices; A.n_edges = (uint32_t)n_edges; A.n_links = (uint32_t)n_links; A.mode = mode;
    A.edges = dedges.as<PathEdge>(); A.links = dlinks.as<PathLink>();
    A.slots = slots.as<unsigned long long>(); A.slot_edge = slot_edge.as<uint32_t>(); A.slot_bits = (uint32_t)slot_bits;
    A.deg = sides.as<uint32_t>(); A.notnew = A.deg + 2 * V; A.maxn = A.notnew + 2 * V; A.cntmax = A.maxn + 2 * V; A.kept_deg = A.cntmax + 2 * V;
    A.next = graph.as<uint32_t>(); A.prev = A.next + V; A.vnew = A.prev + V; A.sup = A.vnew + V; A.vd = (int32_t *)(A.sup + V);
    A.head_of = A.sup + 2 * V;
    A.word[0] = words.as<unsigned long long>(); A.word[1] = A.word[0] + V;
    A.minv[0] = mins.as<uint32_t>(); A.minv[1] = A.minv[0] + V;
    A.lens = scans.as<uint32_t>(); A.cnts = A.lens + V + 1;
    A.chain_vertex = outs.as<uint32_t>(); A.chain_d = (int32_t *)(A.chain_vertex + V); A.chain_off = A.chain_vertex + 2 * V;
    A.info = info.as<PathInfo>();
    PathInfo hinfo = {};
    const unsigned vgrid = (unsigned)((V + PATH_NT - 1) / PATH_NT), egrid = (unsigned)((n_edges + PATH_NT - 1) / PATH_NT);
    {
        ProfSpan sp(c, "paths");
        if (n_edges) HIPCHK(c, hipMemcpyAsync(dedges.p, edges, n_edges * sizeof(PathEdge), hipMemcpyHostToDevice, c->stream));
        if (n_links) HIPCHK(c, hipMemcpyAsync(dlinks.p, links, n_links * sizeof(PathLink), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(info.p, 0, sizeof(PathInfo), c->stream));
        HIPCHK(c, hipMemsetAsync(slots.p, 0xFF, n_slots * 8, c->stream));
        HIPCHK(c, hipMemsetAsync(sides.p, 0, 10 * V * 4, c->stream));
        HIPCHK(c, hipMemsetAsync(A.next, 0xFF, 2 * V * 4, c->stream)); /* next, prev = PATH_NONE */
        HIPCHK(c, hipMemsetAsync(A.vnew, 0, 4 * V * 4, c->stream));
        if (n_edges) {
            hipLaunchKernelGGL(path_pass1_kernel, dim3(egrid), dim3(PATH_NT), 0, c->stream, A);
            hipLaunchKernelGGL(path_pass2_kernel, dim3(egrid), dim3(PATH_NT), 0, c->stream, A);
            hipLaunchKernelGGL(path_linearize_kernel, dim3(egrid), dim3(PATH_NT), 0, c->stream, A);
        }
        int at = path_rank(c, A, vgrid, rounds);
        if (mode == PATH_MODE_TRANSITIVE) { /* every new edge is judged on the same graph (:363-365), then the graph is ranked again */
            if (n_links) hipLaunchKernelGGL(path_support_kernel, dim3((unsigned)((n_links + PATH_NT - 1) / PATH_NT)), dim3(PATH_NT), 0, c->stream, A, at);
            hipLaunchKernelGGL(path_filter_kernel, dim3(vgrid), dim3(PATH_NT), 0, c->stream, A);
            at = path_rank(c, A, vgrid, rounds);
        }
        hipLaunchKernelGGL(path_heads_kernel, dim3(vgrid), dim3(PATH_NT), 0, c->stream, A, at);
        HIPCHK(c, hipGetLastError());
        if ((rc = device_scan(c, A.lens, A.lens, V, nullptr, 2, &A.info->n_chain_vertices))) return rc;
        hipLaunchKernelGGL(path_scatter_kernel, dim3(vgrid), dim3(PATH_NT), 0, c->stream, A, at);
        HIPCHK(c, hipGetLastError());
    }
    /* the result comes back through the context's page-locked block: two copies that do not block, ONE wait, and only what the
       counts say goes on to the caller's arrays */
    const size_t out_bytes = (2 * V + V / 2 + 1) * 4;
    void *stage = nullptr;
    if ((rc = host_tmp(c, out_bytes + sizeof(PathInfo), &stage))) return rc;
    uint32_t *h_vertex = (uint32_t *)stage, *h_d = h_vertex + V, *h_off = h_vertex + 2 * V;
    HIPCHK(c, hipMemcpyAsync(stage, outs.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync((char *)stage + out_bytes, info.p, sizeof(PathInfo), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, main_wait(c));
    memcpy(&hinfo, (char *)stage + out_bytes, sizeof(PathInfo));
    if (hinfo.err & PATH_ERR_DUP) return fail(c, NTL_EINVAL, "ntl_path_chains: an edge occurs twice in the edge list");
    if (hinfo.err & PATH_ERR_TWIN)
        return fail(c, NTL_EINVAL, "ntl_path_chains: an edge lacks its twin (tgt ^ 1, src ^ 1) with the same d, n and flags");
    if (hinfo.err & PATH_ERR_NONLINEAR) return fail(c, NTL_EINVAL, "ntl_path_chains: graph is not linear after linearize");
    if (hinfo.n_chain_vertices > V || hinfo.n_chains > V / 2) return fail(c, NTL_EINTERNAL, "ntl_path_chains: the chains do not fit the graph");
    memcpy(chain_vertex, h_vertex, (size_t)hinfo.n_chain_vertices * 4);
    memcpy(chain_d, h_d, (size_t)hinfo.n_chain_vertices * 4);
    memcpy(chain_off, h_off, ((size_t)hinfo.n_chains + 1) * 4);
    memcpy(counts, &hinfo, sizeof(*counts));
    counts->reserved[0] = counts->reserved[1] = counts->reserved[2] = 0;
    return NTL_OK;
}

/* ------------------------------------------------------------------ index ---------------- */


extern "C" int ntl_index_build(ntl_ctx *c, const ntl_sketch *ctg, const uint32_t *ctg_len, uint32_t n_ctg, ntl_index **out)
{
    if (!c || !ctg || !out || (!ctg_len && n_ctg)) return NTL_EINVAL;
    *out = nullptr;
    if ((uint64_t)n_ctg != ctg->nseq) return fail(c, NTL_EINVAL, "n_ctg must equal the number of sketched contigs");
    if (ctg->no_records) return fail(c, NTL_EINVAL, "a sketch made by ntl_sketch_run_for_map holds no records");
    if (n_ctg >= (1u << 29)) return fail(c, NTL_EINVAL, "too many contigs"); /* contig id << 3 | flags in one word (map_kernels.h) */
    (void)hipSetDevice(c->device);
    if (int frc = sketch_finalize(ctg)) return frc; /* the table is sized from the number of contig minimizers */
    if (ctg->c != c) HIPCHK(c, sync_both(ctg->c));
    std::unique_ptr<ntl_index> ix_guard(new ntl_index());
    ntl_index *ix = ix_guard.get();
    ix->c = c; ix->n_ctg = n_ctg; ix->gen = g_index_gen++;
    int bits = 10;
    while (((uint64_t)1 << bits) < 2 * ctg->count + 2) bits++;
    ix->bits = bits;
    ix->nslots = (uint64_t)1 << bits;
    int rc;
    DevBuf &cnt = ix->cnt;
    if ((rc = ix->slots.alloc(c, ix->nslots * sizeof(IndexSlot))) || (rc = ix->special.alloc(c, sizeof(IndexSpecial))) ||
        (rc = ix->ctg_len.alloc(c, ((uint64_t)n_ctg + 1) * 4)) || (rc = cnt.alloc(c, 8)) || (rc = ix->tags.alloc(c, ix->nslots + 16))) return rc;
    unsigned long long size = 0;
    {
        ProfSpan sp(c, "index");
        ix->h_ctg_len.assign(ctg_len, ctg_len + n_ctg);
        if (n_ctg) HIPCHK(c, hipMemcpyAsync(ix->ctg_len.p, ix->h_ctg_len.data(), (uint64_t)n_ctg * 4, hipMemcpyHostToDevice, c->stream));
        DevBuf dup; /* one bit per slot: the key arrived more than once */
        if ((rc = dup.alloc(c, ix->nslots / 8))) return rc;
        hipLaunchKernelGGL(index_clear_kernel, dim3((unsigned)((ix->nslots + 255) / 256)), dim3(256), 0, c->stream,
                           ix->slots.as<IndexSlot>(), ix->nslots, dup.as<uint32_t>(), ix->special.as<IndexSpecial>(),
                           cnt.as<unsigned long long>());
        if (ctg->count)
            hipLaunchKernelGGL(index_insert_kernel, dim3((unsigned)((ctg->count + 255) / 256)), dim3(256), 0, c->stream,
                               (const MxRecord *)ctg->records.as<MxRecord>(), ctg->count, ix->slots.as<IndexSlot>(), bits,
                               ix->special.as<IndexSpecial>(), dup.as<uint32_t>());
        hipLaunchKernelGGL(index_finish_kernel, dim3((unsigned)std::min<uint64_t>((ix->nslots / 4 + 255) / 256, 4096)), dim3(256), 0, c->stream,
                           ix->slots.as<IndexSlot>(), ix->nslots, (const IndexSpecial *)ix->special.as<IndexSpecial>(),
                           (const uint32_t *)dup.as<uint32_t>(), ix->tags.as<uint8_t>(), cnt.as<unsigned long long>());
        HIPCHK(c, hipGetLastError());
        /* the lookups read eight tags at a time from any slot: the first eight again behind the last (the probe sequence wraps) */
        HIPCHK(c, hipMemcpyAsync(ix->tags.as<uint8_t>() + ix->nslots, ix->tags.p, 8, hipMemcpyDeviceToDevice, c->stream));
    }
    (void)size;
    if ((ix->built = c->pq.event_get())) HIPCHK(c, hipEventRecord(ix->built, c->stream));
    *out = ix_guard.release();
    return NTL_OK;
}

extern "C" void ntl_index_destroy(ntl_index *ix)
{
    if (ix) index_unref(ix, ix->c); /* sketches and map results still pending against it keep it until their work has run */
}

extern "C" uint64_t ntl_index_size(const ntl_index *ix)
{
    if (!ix) return 0;
    if (!ix->size_known) {
        unsigned long long v = 0;
        (void)hipSetDevice(ix->c->device);
        if (hipMemcpyAsync(&v, ix->cnt.p, 8, hipMemcpyDeviceToHost, ix->c->stream) == hipSuccess &&
            hipStreamSynchronize(ix->c->stream) == hipSuccess) {
            ix->size = v;
            ix->size_known = true;
        }
    }
    return ix->size;
}

/* ------------------------------------------------------------------ map ------------------ */

static_assert(sizeof(MapSums) <= sizeof(PinSlot), "the sums must fit a page-locked slot (map_kernels.h)");
static_assert(sizeof(ntl_mapping) == sizeof(MapRec) && sizeof(ntl_hit) == sizeof(HitRec) && sizeof(ntl_paf) == sizeof(PafRec),
              "ABI records must match the device records"); /* uploads, downloads and the gap reader copy them as they are */

/* Made by mapres_new only: a result of ntl_mapres_from_host is these defaults (nothing armed, no lookup, not grouped) plus its records */
struct ntl_mapres {
    ntl_ctx *c;
    const ntl_map_params params;
    ntl_mapres(ntl_ctx *ctx, const ntl_map_params &p) : c(ctx), params(p) {}
    mutable uint64_t n_maps = 0, n_hits = 0, n_pafs = 0, n_index_hits = 0;
    mutable DevBuf maps, pafs;       /* dense, read order; sized from the sketch's capacity, filled to n_* */
    mutable DevBuf hits;             /* per-read regions (read r's hits from mx_off[r] on); maps[].hit_off points into them */
    mutable DevBuf maps_dense, hits_dense, hit_doff; /* made on demand: the dense copy ntl_mapres_download hands out; u32[n_maps + 1] dense offsets */
    mutable bool dense_made = false, doff_made = false;
    uint64_t n_reads = 0, rec_cap = 0;  /* reads of the sketch; records `maps`, `hits` and `pafs` hold */
    mutable Pending lz;                 /* lazy completion (pending.h); holds[0]: the lookup's source (`ix`, or a grouped result's contig sketch), holds[1]: the batch whose lengths the kernels read */
    /* what map_enqueue queues from, the first time and -- mapres_finalize -- the second */
    const ntl_index *ix = nullptr;      /* the index of the lookup (ntl_map_run only); alive while lz.holds[0] is */
    const ntl_sketch *reads = nullptr; uint64_t reads_gen = 0; /* held (refs) while pending; its generation when the kernels were queued */
    std::shared_ptr<std::atomic<float>> hitf; /* the index's hit fraction (the index itself may be gone when this completes) */
    DevBuf rlen_own;                    /* read lengths uploaded by this call (sketches that did not come from a batch) */
    const uint32_t *d_rlen = nullptr;   /* the read lengths the kernels read: rlen_own, or the batch's own (d_seq_len; lz holds the batch) */
    /* ntl_map_run_grouped only: no index -- the lookup reads the records of the contig sketch -- and contig lengths of the result's own */
    bool grouped = false, gap_shaped = false; /* gap_shaped: group g is "contigs 2g and 2g + 1, read g" (ntl_mapres_gap_cuts) */
    ntl_grouped_info ginfo = {};
    DevBuf ctg_len_own;
    mutable DevBuf map_off;             /* the gather's scans, kept for ntl_mapres_gap_cuts: the first third, u32[n_reads + 1], first mapping of every read */
};

/* what map_lookup_stage queues in place of the index lookup for a grouped result (group_kernels.h); it fills in cand, rpos, nfound and err */
struct GroupJob { GroupArgs A; unsigned grid; };

/* What one map_enqueue holds between its stages (SketchWork is the model).  Every temporary lives here and not in a stage: the blocks
 * return to the context's cache when map_enqueue ends, behind every kernel of this work on MAIN. */
struct MapWork {
    bool have_cand;            /* the sketch carries this index's candidates: no lookup */
    uint64_t nreads, nmx, cap; /* cap: records the arrays hold (nmx, at least 1) */
    DevBuf cand, rpos, smaps, spafs, n3, off3_own, scr, over;
    DevBuf *off3;              /* off3_own; a grouped result keeps its offsets: R->map_off (ntl_mapres_gap_cuts) */
    MapSums *dsums;            /* the result's entry of the per-slot device array (map_prepare) */
    MapArgs A;
};

/* The temporaries, the result's arrays and the kernels' arguments, from R->ix (a grouped result has none), R->reads, R->d_rlen, R->params */
static int map_prepare(ntl_ctx *c, ntl_mapres *R, MapWork &W)
{
    const ntl_sketch *reads = R->reads;
    int rc;
    W.have_cand = R->ix && reads->cand_gen == R->ix->gen && reads->cand.p != nullptr;
    if (reads->no_records && !W.have_cand) return fail(c, NTL_EINVAL, "a sketch made by ntl_sketch_run_for_map maps against the index it was made for only");
    if (!W.have_cand && (rc = sketch_finalize(reads))) return rc; /* the lookup pass runs over the records: their number sizes its grid */
    const uint64_t nreads = W.nreads = reads->nseq;
    W.nmx = reads->lz.pending ? reads->cap : reads->count;
    const uint64_t cap = W.cap = W.nmx ? W.nmx : 1;
    W.off3 = R->grouped ? &R->map_off : &W.off3_own;
    R->dense_made = R->doff_made = false; R->n_reads = nreads; R->rec_cap = cap;
    if ((!W.have_cand && ((rc = W.cand.alloc(c, cap * sizeof(Cand))) || (rc = W.rpos.alloc(c, cap * 4)))) || (rc = W.smaps.alloc(c, cap * sizeof(MapRec))) ||
        (rc = W.spafs.alloc(c, cap * sizeof(PafRec))) || (rc = W.n3.alloc(c, 3 * (nreads + 1) * 4)) || (rc = W.off3->alloc(c, 3 * (nreads + 1) * 4)) ||
        (rc = W.scr.alloc(c, (uint64_t)(MAP_NHA + MAP_NRA) * cap * 4)) || (rc = W.over.alloc(c, (nreads + 1) * 4)) ||
        (rc = R->maps.alloc(c, cap * sizeof(MapRec))) || (rc = R->hits.alloc(c, cap * sizeof(HitRec))) || (rc = R->pafs.alloc(c, cap * sizeof(PafRec)))) return rc;
    /* The sums: the result's entry of the per-slot device array.  It is zero whenever the slot is free -- map_gather_kernel, the last
       kernel of this work, hands the sums to the slot and leaves the entry zero; the slot is recycled only after R->lz.done, behind it
       (or, on the error paths, after pending_abort zeroed it) -- and every kernel that adds to it runs on MAIN behind the gather of the slot's
       previous holder.  The lookup's count of a sketch made for this index stays where the lookup left it (SketchSums::nfound). */
    MapSums *dsums = W.dsums = (MapSums *)c->pq.slot_dsums(R->lz.slot);
    MapArgs &A = W.A;
    A.mx_off = reads->mx_off.as<uint32_t>(); A.nreads = (uint32_t)nreads;
    A.rpos = W.have_cand ? reads->rpos.as<uint32_t>() : W.rpos.as<uint32_t>();
    A.cand = W.have_cand ? reads->cand.as<Cand>() : W.cand.as<Cand>();
    A.read_len = R->d_rlen; A.ctg_len = R->grouped ? R->ctg_len_own.as<uint32_t>() : R->ix->ctg_len.as<uint32_t>();
    A.P.k = R->params.k; A.P.z = R->params.z; A.P.x = R->params.x; A.P.sensitive = R->params.sensitive; A.P.repeat_filter = R->params.repeat_filter;
    A.maps = W.smaps.as<MapRec>(); A.hits = R->hits.as<HitRec>(); A.pafs = W.spafs.as<PafRec>();
    A.n_maps = W.n3.as<uint32_t>(); A.n_hits = A.n_maps + (nreads + 1); A.n_pafs = A.n_hits + (nreads + 1);
    A.scr = W.scr.as<uint32_t>(); A.scr_stride = cap; A.err = &dsums->err; A.over_list = W.over.as<uint32_t>(); A.over_count = &dsums->n_over;
    /* a sketch whose count is not known yet may have overflowed its arrays: the kernels look at its total and leave it alone */
    A.mx_total = reads->lz.pending ? &reads->sums.as<SketchSums>()->total_mx : nullptr;
    A.mx_cap = (uint32_t)std::min<uint64_t>(reads->cap, 0xFFFFFFFFull);
    A.lanes = MAP_GW; A.group_strict = 0; /* (map_kernels_stage reads the knobs) */
    return NTL_OK;
}

/* The lookup, unless the sketch carries its candidates: the index probe, or gj's probe of every read in its own group's contigs (one kernel builds, uses and drops the tables) */
static int map_lookup_stage(ntl_ctx *c, const ntl_mapres *R, const GroupJob *gj, MapWork &W)
{
    const ntl_index *ix = R->ix;
    hipStream_t ms = c->stream;
    if (ix && ix->c != c && ix->built) HIPCHK(c, hipStreamWaitEvent(ms, ix->built, 0));
    if (W.have_cand) return NTL_OK;
    ProfSpan sp(c, "probe");
    if (gj && W.nmx) {
        GroupArgs G = gj->A;
        G.cand = W.cand.as<Cand>(); G.rpos = W.rpos.as<uint32_t>(); G.nfound = &W.dsums->nfound; G.err = &W.dsums->err;
        hipLaunchKernelGGL(group_probe_kernel, dim3(gj->grid), dim3(GROUP_NT), 0, ms, G);
    } else if (W.nmx) {
        const dim3 grid((unsigned)std::min<uint64_t>((W.nmx + 256 * PROBE_U - 1) / (256 * PROBE_U), 4096));
        /* tags first unless the previous batch on this index found more than half of its minimizers (same result either way) */
        const auto probe = ix->hit_fraction->load(std::memory_order_relaxed) <= 0.5f ? probe_kernel<true> : probe_kernel<false>;
        hipLaunchKernelGGL(probe, grid, dim3(256), 0, ms, (const MxRecord *)R->reads->records.as<MxRecord>(), W.nmx,
                           (const IndexSlot *)ix->slots.as<IndexSlot>(), ix->bits, (const IndexSpecial *)ix->special.as<IndexSpecial>(),
                           W.cand.as<Cand>(), W.rpos.as<uint32_t>(), &W.dsums->nfound, (const uint8_t *)ix->tags.as<uint8_t>());
    }
    HIPCHK(c, hipGetLastError());
    return NTL_OK;
}

/* Reads by size class, each class with the LDS staging that fits it; resident-size grids (28 / 14 / 8 wavefronts per CU fit) looping
   over all reads, 64 at a time */
static int map_kernels_stage(ntl_ctx *c, const MapWork &W)
{
    hipStream_t ms = c->stream;
    ProfSpan sp(c, "map");
    const uint64_t groups = (W.nreads + MAP_GROUP - 1) / MAP_GROUP;
    uint64_t g0 = 4 * 7168, g1 = 4 * 3584, g2 = 4 * 2048;
    if (const char *e = getenv("NTL_MAP_WAVES_PER_CU")) { /* tuning: a bounded number of resident wavefronts beside the window stage */
        const uint64_t resident = (uint64_t)std::max(1, atoi(e)) * (uint64_t)std::max(1, c->n_cu);
        g0 = std::min(g0, resident); g1 = std::min(g1, resident); g2 = std::min(g2, resident);
    }
    MapArgs A = W.A;
    /* NTL_MAP_LANES=64: the first class never enters its group path (one read per wavefront throughout: A/B runs, tests).
       NTL_MAP_GROUP_STRICT=1: a first-class read that leaves the group path fails the result (MAP_ERR_LEFT_GROUP): which path ran */
    if (const char *e = getenv("NTL_MAP_LANES")) if (atoi(e) == MAP_NT) A.lanes = MAP_NT;
    if (const char *e = getenv("NTL_MAP_GROUP_STRICT")) A.group_strict = atoi(e) != 0;
    hipLaunchKernelGGL((map_kernel<256, 64, 0>), dim3((unsigned)std::min<uint64_t>(groups, g0)), dim3(MAP_NT), 0, ms, A);
    hipLaunchKernelGGL((map_kernel<512, 128, 1>), dim3((unsigned)std::min<uint64_t>(groups, g1)), dim3(MAP_NT), 0, ms, A);
    hipLaunchKernelGGL((map_kernel<1024, 128, 2>), dim3((unsigned)std::min<uint64_t>(groups, g2)), dim3(MAP_NT), 0, ms, A);
    /* reads with more hits / runs than the largest staging holds (rare): same code on global scratch */
    hipLaunchKernelGGL(map_overflow_kernel, dim3((unsigned)std::min<uint64_t>(W.nreads, 8192)), dim3(MAP_NT), 0, ms, A); /* no LDS: 32 wavefronts per CU resident */
    HIPCHK(c, hipGetLastError());
    return NTL_OK;
}

/* The three offset scans and the gather, whose first lane hands the sums to the result's slot */
static int map_gather_stage(ntl_ctx *c, ntl_mapres *R, MapWork &W)
{
    const ntl_sketch *reads = R->reads;
    const uint64_t nreads = W.nreads;
    ProfSpan sp(c, "compact");
    uint32_t *o = W.off3->as<uint32_t>();
    if (int rc = device_scan(c, W.n3.as<uint32_t>(), o, nreads, nullptr, 3, W.dsums->tot)) return rc;
    MapSumsOut O;
    O.sums = W.dsums; O.slot = (unsigned long long *)c->pq.slot_dev(R->lz.slot);
    O.nfound = W.have_cand ? &reads->sums.as<SketchSums>()->nfound : &W.dsums->nfound;
    /* the sketch's own hit count, if nothing has copied it yet: its event moves behind this kernel (sketch_finalize waits for it) */
    const bool owed = W.have_cand && reads->lz.pending && reads->nfound_owed;
    O.sk_nfound = owed ? &((SketchSums *)c->pq.slot_dev(reads->lz.slot))->nfound : nullptr;
    hipLaunchKernelGGL(map_gather_kernel, dim3((unsigned)((nreads + GATHER_NT - 1) / GATHER_NT)), dim3(GATHER_NT), 0, c->stream, W.A, (const uint32_t *)o,
                       (const uint32_t *)(o + 2 * (nreads + 1)), R->maps.as<MapRec>(), R->pafs.as<PafRec>(), O);
    HIPCHK(c, hipGetLastError());
    if (owed) { HIPCHK(c, hipEventRecord(reads->lz.done, c->stream)); reads->nfound_owed = false; }
    return NTL_OK;
}

/* Queues the lookup (when the sketch does not carry candidates), the map kernels, the offset scans and the gather on MAIN, from the result's
 * own fields (and gj for a grouped one).  Nothing waits: the three totals, the hit count and the invariant flag land in its page-locked slot. */
static int map_enqueue(ntl_ctx *c, ntl_mapres *R, const GroupJob *gj = nullptr)
{
    MapWork W;
    int rc;
    if ((rc = map_prepare(c, R, W)) || (rc = map_lookup_stage(c, R, gj, W))) return rc;
    /* (no reads: no kernel, and the slot keeps the zeros slot_get left in it) */
    if (W.nreads && ((rc = map_kernels_stage(c, W)) || (rc = map_gather_stage(c, R, W)))) return rc;
    HIPCHK(c, hipEventRecord(R->lz.done, c->stream));
    R->lz.pending = true;
    R->reads_gen = R->reads->gen;
    return NTL_OK; /* (W's temporaries return to the context's cache here) */
}

/* The check of a map result, completed or destroyed before anybody asked: the invariant flag, and the batch's hit fraction for the
   index's next batch */
static const char *map_check(const PinSlot &slot, uint64_t, std::atomic<float> *hitf)
{
    const MapSums &hs = (const MapSums &)slot;
    if (hitf && hs.nmx) hitf->store((float)((double)hs.nfound / (double)hs.nmx), std::memory_order_relaxed);
    if (hs.err & GROUP_ERR_PROBE) return "a probe sequence of a grouped lookup did not end within its table (group_kernels.h)";
    if (hs.err & MAP_ERR_TWICE) return "an accepted contig appeared twice in one read (bin/ntlink_utils.py:262-266)";
    if (hs.err & MAP_ERR_LEFT_GROUP) return "a read of the first class left the group path (NTL_MAP_GROUP_STRICT, map_kernels.h map_read_groups)";
    return hs.err ? "a map result's err word holds an unknown bit" : nullptr;
}

static void mapres_free(ntl_mapres *R)
{
    if (!R) return;
    (void)hipSetDevice(R->c->device);
    R->lz.orphan(R->c->pq, map_check, 0, R->hitf); /* index and batch stay until the kernels have run: they read d_seq_len */
    if (R->reads) sketch_unref(R->reads);
    delete R;
}

/* The one way to make a result: whatever path drops the handle gives back event, slot, holds and the sketch (mapres_free) */
struct MapResFree { void operator()(ntl_mapres *R) const { mapres_free(R); } };
typedef std::unique_ptr<ntl_mapres, MapResFree> MapResPtr;
static MapResPtr mapres_new(ntl_ctx *c, const ntl_map_params &params) { return MapResPtr(new ntl_mapres(c, params)); }

/* The one error exit of the calls that make a result.  `queued`: from the call's first launch or async copy on, every exit drains the
   device and scrubs the slot's device sums (pending_abort) before an armed result lets go of what the queued work reads; before that none does. */
static int mapres_fail(MapResPtr &R, int rc, bool queued)
{
    if (queued && R->lz.slot) pending_abort(R->c, R->lz, rc, true);
    R.reset();
    return rc;
}

/* The lengths a call brings along, into the result's own arrays: rlen_own, which the kernels then read, and a grouped result's
   ctg_len_own.  wait: the source is pageable and the caller's array must be free again (a caller that waits on MAIN later passes false). */
static hipError_t mapres_upload_lengths(ntl_mapres *R, const uint32_t *read_len, uint64_t nreads, bool wait, const uint32_t *ctg_len = nullptr, uint64_t n_ctg = 0)
{
    hipError_t e = n_ctg ? hipMemcpyAsync(R->ctg_len_own.p, ctg_len, n_ctg * 4, hipMemcpyHostToDevice, R->c->stream) : hipSuccess;
    if (e == hipSuccess && nreads) e = hipMemcpyAsync(R->rlen_own.p, read_len, nreads * 4, hipMemcpyHostToDevice, R->c->stream);
    if (e == hipSuccess && nreads && wait) e = hipStreamSynchronize(R->c->stream);
    R->d_rlen = R->rlen_own.as<uint32_t>();
    return e;
}

/* Completes a map result: the sketch first (it may have to be made again with larger arrays -- then the map kernels ran on
 * nothing and are queued again), then this call's totals. */
static int mapres_finalize(const ntl_mapres *cR)
{
    ntl_mapres *R = const_cast<ntl_mapres *>(cR);
    Pending &lz = R->lz;
    if (!lz.pending) return lz.failed;
    ntl_ctx *c = R->c;
    (void)hipSetDevice(c->device);
    for (int round = 0;; round++) {
        if (R->reads && (lz.failed = sketch_finalize(R->reads))) { (void)hipEventSynchronize(lz.done); lz.pending = false; break; }
        const hipError_t e = lz.wait();
        lz.pending = false;
        if (e != hipSuccess) { lz.failed = fail(c, NTL_EDEVICE, std::string("map: ") + hipGetErrorString(e)); break; }
        if (R->reads && R->reads->gen != R->reads_gen && round == 0) {
            /* unreachable for a grouped result: ntl_map_run_grouped completes both sketches (its two sketch_finalize calls) before it
               queues anything, so reads->gen cannot move; its group tables were temporaries of that call and are gone */
            if (R->grouped) { lz.failed = fail(c, NTL_EINTERNAL, "map: the read sketch of a grouped result was made again"); break; }
            memset(lz.slot, 0, sizeof(PinSlot));
            if (const int rc = map_enqueue(c, R)) { pending_abort(c, lz, rc, true); break; }
            continue;
        }
        const MapSums hs = *(const MapSums *)lz.slot;
        R->n_maps = hs.tot[0]; R->n_hits = hs.tot[1]; R->n_pafs = hs.tot[2]; R->n_index_hits = hs.nfound;
        if (const char *m = map_check(*lz.slot, 0, R->hitf.get())) lz.failed = fail(c, NTL_EINTERNAL, m);
        break;
    }
    if (R->reads) { sketch_unref(R->reads); R->reads = nullptr; }
    lz.settle(c->pq);
    return lz.failed;
}

extern "C" int ntl_map_run(ntl_ctx *c, const ntl_index *ix, const ntl_sketch *reads, const uint32_t *read_len,
                           const ntl_map_params *params, ntl_mapres **out)
{
    if (!c || !ix || !reads || !params || !out || (!read_len && reads->nseq)) return NTL_EINVAL;
    *out = nullptr;
    (void)hipSetDevice(c->device);
    if (reads->c != c) { /* a sketch of another context: complete it there first */
        if (int frc = sketch_finalize(reads)) return frc;
        HIPCHK(c, sync_both(reads->c));
    }
    const uint64_t nreads = reads->nseq;
    MapResPtr R = mapres_new(c, *params);
    R->ix = ix; R->hitf = ix->hit_fraction;
    ix->refs++; R->lz.holds[0] = {ix, hold_index};
    if (!R->lz.arm(c->pq)) return mapres_fail(R, fail(c, NTL_EDEVICE, "out of events / page-locked slots"), false);
    /* read lengths: a sketch made from a batch that it still holds (pending) reads them from the batch (the `--len` column IS the
       sequence length); the result holds the batch too, until its kernels have run (mapres_finalize, or reap for a result destroyed
       before that).  Anything else -- or lengths that differ from the batch's -- is uploaded here. */
    if (reads->src && reads->src->d_seq_len && nreads && memcmp(read_len, reads->src->seq_len.data(), nreads * 4) == 0) {
        R->d_rlen = reads->src->d_seq_len;
        const_cast<ntl_batch *>(reads->src)->refs++; R->lz.holds[1] = {reads->src, hold_batch};
    } else {
        if (int rc = R->rlen_own.alloc(c, (nreads + 1) * 4)) return mapres_fail(R, rc, false);
        if (mapres_upload_lengths(R.get(), read_len, nreads, true)) return mapres_fail(R, fail(c, NTL_EDEVICE, "upload of the read lengths failed"), true);
    }
    const_cast<ntl_sketch *>(reads)->refs++; R->reads = reads;
    if (int rc = map_enqueue(c, R.get())) return mapres_fail(R, rc, true);
    *out = R.release();
    return NTL_OK;
}

/* A completed result from the caller's records (the map side's ntl_sketch_from_host): no kernel, three uploads.  The hits keep the
   layout map_gather_kernel leaves -- regions that ascend with the mapping number, unused slots wherever the caller put them -- so that
   densify and the text kernels see what they see behind the mapper.  Nothing is armed: everything but the records is as mapres_new made it. */
extern "C" int ntl_mapres_from_host(ntl_ctx *c, const ntl_mapping *maps, uint64_t n_maps, const ntl_hit *hit_slots, uint64_t n_hit_slots,
                                    const ntl_paf *pafs, uint64_t n_pafs, ntl_mapres **out)
{
    if (!c || !out) return NTL_EINVAL;
    *out = nullptr;
    (void)hipSetDevice(c->device);
    if ((n_maps && !maps) || (n_hit_slots && !hit_slots) || (n_pafs && !pafs))
        return fail(c, NTL_EINVAL, "ntl_mapres_from_host: a null array with a non-zero count");
    if (n_maps >= 0xFFFFFF00ull || n_hit_slots >= 0xFFFFFF00ull || n_pafs >= 0xFFFFFF00ull)
        return fail(c, NTL_EINVAL, "ntl_mapres_from_host: too many records for one result");
    uint64_t n_hits = 0, at = 0; /* at: the first slot behind the regions so far */
    for (uint64_t m = 0; m < n_maps; m++) {
        const ntl_mapping &M = maps[m];
        if (!M.n_hits) return fail(c, NTL_EINVAL, "ntl_mapres_from_host: mapping " + std::to_string(m) + " has no hits");
        if (M.hit_off > n_hit_slots || M.n_hits > n_hit_slots - M.hit_off)
            return fail(c, NTL_EINVAL, "ntl_mapres_from_host: the hit region of mapping " + std::to_string(m) + " leaves hit_slots");
        if (M.hit_off < at)
            return fail(c, NTL_EINVAL, "ntl_mapres_from_host: the hit region of mapping " + std::to_string(m) + " overlaps or lies in front of the one before it");
        at = M.hit_off + M.n_hits;
        n_hits += M.n_hits;
    }
    MapResPtr R = mapres_new(c, ntl_map_params());
    R->n_maps = n_maps; R->n_hits = n_hits; R->n_pafs = n_pafs;
    R->rec_cap = std::max<uint64_t>(n_hit_slots, 1);
    int rc;
    if ((rc = R->maps.alloc(c, (n_maps + 1) * sizeof(MapRec))) || (rc = R->hits.alloc(c, (n_hit_slots + 1) * sizeof(HitRec))) ||
        (rc = R->pafs.alloc(c, (n_pafs + 1) * sizeof(PafRec)))) return mapres_fail(R, rc, false);
    hipError_t e = hipSuccess;
    if (n_maps) e = hipMemcpyAsync(R->maps.p, maps, n_maps * sizeof(MapRec), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && n_hit_slots) e = hipMemcpyAsync(R->hits.p, hit_slots, n_hit_slots * sizeof(HitRec), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && n_pafs) e = hipMemcpyAsync(R->pafs.p, pafs, n_pafs * sizeof(PafRec), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream); /* pageable sources: the caller's arrays are free again */
    if (e != hipSuccess) return mapres_fail(R, fail(c, NTL_EDEVICE, hipGetErrorString(e)), true); /* (nothing armed: no slot to scrub) */
    *out = R.release();
    return NTL_OK;
}

extern "C" void ntl_mapres_destroy(ntl_mapres *r) { mapres_free(r); }
extern "C" int ntl_mapres_wait(const ntl_mapres *r) { return r ? mapres_finalize(r) : NTL_EINVAL; }
extern "C" uint64_t ntl_mapres_n_mappings(const ntl_mapres *r) { return r && mapres_finalize(r) == NTL_OK ? r->n_maps : 0; }
extern "C" uint64_t ntl_mapres_n_hits(const ntl_mapres *r) { return r && mapres_finalize(r) == NTL_OK ? r->n_hits : 0; }
extern "C" uint64_t ntl_mapres_n_pafs(const ntl_mapres *r) { return r && mapres_finalize(r) == NTL_OK ? r->n_pafs : 0; }
extern "C" uint64_t ntl_mapres_n_index_hits(const ntl_mapres *r) { return r && mapres_finalize(r) == NTL_OK ? r->n_index_hits : 0; }

/* ------------------------------------------------------------------ grouped map ---------- */

static void hold_sketch(const void *s, void *) { sketch_unref((const ntl_sketch *)s); }

static const char *group_offsets_check(const uint32_t *off, uint32_t n_groups, uint64_t nseq, const char *what, std::string &msg)
{
    if (off[0] != 0) msg = std::string(what) + "[0] must be 0";
    else if (off[n_groups] != nseq) msg = std::string(what) + " must end at the sketch's number of sequences";
    else
        for (uint32_t g = 0; g < n_groups; g++)
            if (off[g + 1] < off[g]) { msg = std::string(what) + " must be non-decreasing"; break; }
    return msg.empty() ? nullptr : msg.c_str();
}

extern "C" int ntl_map_run_grouped(ntl_ctx *c, const ntl_sketch *ctg, const uint32_t *ctg_len, const uint32_t *ctg_group_off,
                                   const ntl_sketch *reads, const uint32_t *read_len, const uint32_t *read_group_off, uint32_t n_groups,
                                   const ntl_map_params *params, ntl_mapres **out)
{
    if (!c || !ctg || !reads || !params || !out || !ctg_group_off || !read_group_off || (!ctg_len && ctg->nseq) ||
        (!read_len && reads->nseq)) return NTL_EINVAL;
    *out = nullptr;
    (void)hipSetDevice(c->device);
    if (ctg->no_records || reads->no_records) return fail(c, NTL_EINVAL, "a sketch made by ntl_sketch_run_for_map holds no records");
    if (ctg->nseq >= (1u << 29)) return fail(c, NTL_EINVAL, "too many contigs"); /* contig id << 3 | flags in one word (map_kernels.h) */
    if (n_groups == 0xFFFFFFFFu) return fail(c, NTL_EINVAL, "too many groups");
    std::string msg;
    if (group_offsets_check(ctg_group_off, n_groups, ctg->nseq, "ctg_group_off", msg) ||
        group_offsets_check(read_group_off, n_groups, reads->nseq, "read_group_off", msg)) return fail(c, NTL_EINVAL, msg);
    /* the counts size the work: the tables from the contig minimizers, the lookup's arrays from the reads' */
    if (int frc = sketch_finalize(ctg)) return frc;
    if (int frc = sketch_finalize(reads)) return frc;
    if (ctg->c != c) HIPCHK(c, sync_both(ctg->c));
    if (reads->c != c) HIPCHK(c, sync_both(reads->c));
    /* a large group's table has fewer than 4 n + 4 slots (at least 1024): all regions together must fit the 32-bit scan */
    if (4ull * ctg->count + 1024ull * n_groups >= 0xFFFFFFF0ull) return fail(c, NTL_EINVAL, "too many contig minimizers for one grouped call");
    const uint64_t n_ctg = ctg->nseq, nreads = reads->nseq;
    MapResPtr R = mapres_new(c, *params);
    R->grouped = true;
    R->gap_shaped = ctg->nseq == 2ull * n_groups && reads->nseq == n_groups;
    for (uint32_t g = 0; R->gap_shaped && g <= n_groups; g++) R->gap_shaped = ctg_group_off[g] == 2u * g && read_group_off[g] == g;
    if (!R->lz.arm(c->pq)) return mapres_fail(R, fail(c, NTL_EDEVICE, "out of events / page-locked slots"), false);
    const_cast<ntl_sketch *>(ctg)->refs++; R->lz.holds[0] = {ctg, hold_sketch};
    const_cast<ntl_sketch *>(reads)->refs++; R->reads = reads;
    int rc = NTL_OK;
    DevBuf cg, rg, big, boff, next, scratch;
    const uint64_t ng1 = (uint64_t)n_groups + 1;
    if ((rc = R->ctg_len_own.alloc(c, (n_ctg + 1) * 4)) || (rc = R->rlen_own.alloc(c, (nreads + 1) * 4)) || (rc = cg.alloc(c, ng1 * 4)) ||
        (rc = rg.alloc(c, ng1 * 4)) || (rc = big.alloc(c, 2 * ng1 * 4)) || (rc = boff.alloc(c, 2 * ng1 * 4)) || (rc = next.alloc(c, 4)))
        return mapres_fail(R, rc, false);
    hipError_t e = mapres_upload_lengths(R.get(), read_len, nreads, false, ctg_len, n_ctg); /* (the scan below waits on MAIN); queued from here on */
    if (e == hipSuccess) e = hipMemcpyAsync(cg.p, ctg_group_off, ng1 * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(rg.p, read_group_off, ng1 * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(next.p, 0, 4, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(big.p, 0, 2 * ng1 * 4, c->stream);
    if (e != hipSuccess) return mapres_fail(R, fail(c, NTL_EDEVICE, "upload of the lengths and group offsets failed"), true);
    GroupJob J = {};
    J.A.cmx = ctg->records.as<MxRecord>(); J.A.c_off = ctg->mx_off.as<uint32_t>();
    J.A.rmx = reads->records.as<MxRecord>(); J.A.r_off = reads->mx_off.as<uint32_t>();
    J.A.cg_off = cg.as<uint32_t>(); J.A.rg_off = rg.as<uint32_t>(); J.A.n_groups = n_groups;
    J.A.big_off = boff.as<uint32_t>(); J.A.next = next.as<uint32_t>();
    /* regions of the large groups: one scan over their slot counts and one over a 1 per large group; the two totals are the call's
       one size that comes back (behind it the caller's arrays are free again, too) */
    uint32_t totals[2] = {0, 0};
    if (n_groups) {
        hipLaunchKernelGGL(group_size_kernel, dim3((n_groups + 255) / 256), dim3(256), 0, c->stream, J.A, big.as<uint32_t>());
        if (hipGetLastError() != hipSuccess) return mapres_fail(R, fail(c, NTL_EDEVICE, "group_size_kernel could not be launched"), true);
        if ((rc = device_scan(c, big.as<uint32_t>(), boff.as<uint32_t>(), n_groups, totals, 2))) return mapres_fail(R, rc, true);
    } else if (hipStreamSynchronize(c->stream) != hipSuccess)
        return mapres_fail(R, fail(c, NTL_EDEVICE, "upload of the lengths and group offsets failed"), true);
    R->ginfo.lds_slots = GROUP_LDS_SLOTS; R->ginfo.groups_in_global = totals[1]; R->ginfo.groups_in_lds = (uint64_t)n_groups - totals[1];
    if ((rc = scratch.alloc(c, ((uint64_t)totals[0] + 1) * sizeof(IndexSlot)))) return mapres_fail(R, rc, true);
    J.A.scratch = scratch.as<IndexSlot>();
    static const int per_cu = occupancy_blocks(group_probe_kernel, GROUP_NT);
    J.grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_groups, (uint64_t)per_cu * (uint64_t)std::max(1, c->n_cu)));
    if ((rc = map_enqueue(c, R.get(), &J))) return mapres_fail(R, rc, true);
    *out = R.release();
    return NTL_OK;
}

extern "C" int ntl_mapres_grouped_info(const ntl_mapres *r, ntl_grouped_info *out)
{
    if (!r || !out || !r->grouped) return NTL_EINVAL;
    *out = r->ginfo;
    return NTL_OK;
}

static_assert(sizeof(ntl_gap_cut) == sizeof(GapCut) && sizeof(GapCut) == 32, "ABI record must match the device record");
static_assert(NTL_GAP_NOT_TWO == GAP_NOT_TWO && NTL_GAP_SRC_MIXED_STRANDS == GAP_SRC_MIXED_STRANDS && NTL_GAP_TGT_MIXED_STRANDS == GAP_TGT_MIXED_STRANDS &&
              NTL_GAP_SRC_POSITIONS == GAP_SRC_POSITIONS && NTL_GAP_TGT_POSITIONS == GAP_TGT_POSITIONS, "status bits of the ABI and of gap_kernels.h");

/* The kernel goes on MAIN behind the result's own kernels, pending or not; one wait for the records, and the result's completion
   behind it costs no second one.  Neither the dense hit copy nor any download is involved: the hits are read where the map kernels
   left them. */
extern "C" int ntl_mapres_gap_cuts(const ntl_mapres *r, const uint8_t *src_minus, const uint8_t *tgt_minus, uint32_t n_gaps, int32_t k,
                                   ntl_gap_cut *out)
{
    if (!r || k < 0 || (n_gaps && (!src_minus || !tgt_minus || !out))) return NTL_EINVAL;
    ntl_ctx *c = r->c;
    (void)hipSetDevice(c->device);
    if (!r->grouped) return fail(c, NTL_EINVAL, "ntl_mapres_gap_cuts: not a result of ntl_map_run_grouped");
    if (!r->gap_shaped) return fail(c, NTL_EINVAL, "ntl_mapres_gap_cuts: the groups must be ctg_group_off[g] = 2g, read_group_off[g] = g");
    if (n_gaps != r->n_reads) return fail(c, NTL_EINVAL, "ntl_mapres_gap_cuts: n_gaps must be the read sketch's number of sequences");
    if (!r->lz.pending && r->lz.failed) return r->lz.failed;
    if (!n_gaps) return mapres_finalize(r);
    DevBuf signs, cuts;
    int rc;
    if ((rc = signs.alloc(c, 2ull * n_gaps)) || (rc = cuts.alloc(c, (uint64_t)n_gaps * sizeof(GapCut)))) return rc;
    HIPCHK(c, hipMemcpyAsync(signs.p, src_minus, n_gaps, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(signs.as<uint8_t>() + n_gaps, tgt_minus, n_gaps, hipMemcpyHostToDevice, c->stream));
    GapArgs A;
    A.maps = r->maps.as<MapRec>(); A.hits = r->hits.as<HitRec>(); A.maps_cap = A.hits_cap = r->rec_cap;
    A.map_off = r->map_off.as<uint32_t>();
    A.src_minus = signs.as<uint8_t>(); A.tgt_minus = A.src_minus + n_gaps;
    A.n_gaps = n_gaps; A.k = (uint32_t)k; A.out = cuts.as<GapCut>();
    {
        ProfSpan sp(c, "gap_cut");
        hipLaunchKernelGGL(gap_cut_kernel, dim3((n_gaps + GAP_NT / 64 - 1) / (GAP_NT / 64)), dim3(GAP_NT), 0, c->stream, A);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(out, cuts.p, (uint64_t)n_gaps * sizeof(GapCut), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, main_wait(c));
    return mapres_finalize(r); /* (its event has passed: no second wait) the error of a result whose completion failed */
}

/* ------------------------------------------------------------------ gap filling: the read of every gap ---- */

struct ntl_gap_cands { std::vector<GapCand> rec; };

static_assert(sizeof(ntl_gap_cand) == sizeof(GapCand) && sizeof(GapCand) == 32, "ABI record must match the device record");
static_assert(NTL_GAPSEL_VALID == GSEL_VALID && NTL_GAPSEL_NEGATIVE == GSEL_NEGATIVE && NTL_GAPSEL_VIA_REVCOMP == GSEL_VIA_REVCOMP,
              "flag bits of the ABI and of gap_select_kernels.h");

extern "C" int ntl_gap_pair_table(const uint64_t *keys, uint64_t n_pairs, uint64_t *slot_keys, uint32_t *slot_vals, uint64_t n_slots)
{
    if ((n_pairs && !keys) || !slot_keys || !slot_vals || n_pairs >= 0xFFFFFFFFull) return NTL_EINVAL;
    if (n_slots < 2 || (n_slots & (n_slots - 1)) || n_slots > (1ull << 32) || n_slots / 2 < n_pairs) return NTL_EINVAL;
    for (uint64_t s = 0; s < n_slots; s++) { slot_keys[s] = GSEL_EMPTY; slot_vals[s] = 0; }
    for (uint64_t i = 0; i < n_pairs; i++) {
        if (keys[i] == GSEL_EMPTY) return NTL_EINVAL;
        uint64_t s = gsel_slot(keys[i], n_slots);
        while (slot_keys[s] != GSEL_EMPTY) { /* at most half full: an empty slot is met */
            if (slot_keys[s] == keys[i]) return NTL_EINVAL;
            s = (s + 1) & (n_slots - 1);
        }
        slot_keys[s] = keys[i]; slot_vals[s] = (uint32_t)i;
    }
    return NTL_OK;
}

/* Three kernels and a scan on MAIN (gap_select_kernels.h): assess, count, device_scan -- the one wait that sizes the records --
   fill, and a second wait for the records and the error word. */
extern "C" int ntl_gap_select(ntl_ctx *c, const uint32_t *map_off, uint32_t n_reads, const ntl_mapping *maps, const uint32_t *anchors,
                              uint64_t n_maps, const ntl_hit *hits, uint64_t n_hits, const uint32_t *ctg_len, uint32_t n_ctg, int32_t large_k,
                              const uint64_t *slot_keys, const uint32_t *slot_vals, uint64_t n_slots, ntl_gap_cands **out)
{
    if (!c || !out || !map_off || !slot_keys || !slot_vals || large_k < 0 || (n_maps && (!maps || !anchors)) || (n_hits && !hits) ||
        (n_ctg && !ctg_len))
        return NTL_EINVAL;
    *out = nullptr;
    (void)hipSetDevice(c->device);
    if (n_ctg >= 0x7FFFFFFFu) return fail(c, NTL_EINVAL, "ntl_gap_select: fewer than 2^31 - 1 contigs");
    if (n_reads == 0xFFFFFFFFu || n_maps >= 0xFFFFFF00ull) return fail(c, NTL_EINVAL, "ntl_gap_select: too many reads or mappings in one block");
    if (map_off[0] != 0 || map_off[n_reads] != n_maps) return fail(c, NTL_EINVAL, "ntl_gap_select: map_off must start at 0 and end at n_maps");
    for (uint32_t r = 0; r < n_reads; r++)
        if (map_off[r + 1] < map_off[r]) return fail(c, NTL_EINVAL, "ntl_gap_select: map_off must be non-decreasing");
    if (n_slots < 2 || (n_slots & (n_slots - 1)) || n_slots > (1ull << 32)) return fail(c, NTL_EINVAL, "ntl_gap_select: the pair table's slot count must be a power of two");
    uint64_t filled = 0;
    for (uint64_t s = 0; s < n_slots; s++) filled += slot_keys[s] != GSEL_EMPTY;
    if (filled > n_slots / 2) return fail(c, NTL_EINVAL, "ntl_gap_select: the pair table is more than half full");
    std::unique_ptr<ntl_gap_cands> o(new ntl_gap_cands());
    if (!n_reads || !n_maps || !filled) { *out = o.release(); return NTL_OK; }
    DevBuf d_off, d_maps, d_anc, d_hits, d_len, d_keys, d_vals, d_state, d_length, d_cnt, d_err, d_out;
    int rc;
    if ((rc = d_off.alloc(c, ((uint64_t)n_reads + 1) * 4)) || (rc = d_maps.alloc(c, n_maps * sizeof(MapRec))) || (rc = d_anc.alloc(c, n_maps * 4)) ||
        (rc = d_hits.alloc(c, (n_hits + 1) * sizeof(HitRec))) || (rc = d_len.alloc(c, ((uint64_t)n_ctg + 1) * 4)) || (rc = d_keys.alloc(c, n_slots * 8)) ||
        (rc = d_vals.alloc(c, n_slots * 4)) || (rc = d_state.alloc(c, n_maps)) || (rc = d_length.alloc(c, (uint64_t)n_reads * 4)) ||
        (rc = d_cnt.alloc(c, ((uint64_t)n_reads + 1) * 4)) || (rc = d_err.alloc(c, 4)))
        return rc;
    GselArgs A;
    A.map_off = d_off.as<uint32_t>(); A.maps = d_maps.as<MapRec>(); A.anchors = d_anc.as<uint32_t>(); A.hits = d_hits.as<HitRec>();
    A.n_maps = n_maps; A.n_hits = n_hits; A.n_reads = n_reads; A.n_ctg = n_ctg; A.k = (uint32_t)large_k;
    A.ctg_len = d_len.as<uint32_t>(); A.pair_keys = d_keys.as<unsigned long long>(); A.pair_vals = d_vals.as<uint32_t>(); A.n_slots = n_slots;
    A.mstate = d_state.as<uint8_t>(); A.length = d_length.as<uint32_t>(); A.cnt = d_cnt.as<uint32_t>(); A.err = d_err.as<uint32_t>();
    A.out = nullptr; A.out_cap = 0;
    HIPCHK(c, hipMemcpyAsync(d_off.p, map_off, ((uint64_t)n_reads + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_maps.p, maps, n_maps * sizeof(MapRec), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_anc.p, anchors, n_maps * 4, hipMemcpyHostToDevice, c->stream));
    if (n_hits) HIPCHK(c, hipMemcpyAsync(d_hits.p, hits, n_hits * sizeof(HitRec), hipMemcpyHostToDevice, c->stream));
    if (n_ctg) HIPCHK(c, hipMemcpyAsync(d_len.p, ctg_len, (uint64_t)n_ctg * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_keys.p, slot_keys, n_slots * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_vals.p, slot_vals, n_slots * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_err.p, 0, 4, c->stream));
    const dim3 grid((n_reads + GSEL_NT / 64 - 1) / (GSEL_NT / 64)), block(GSEL_NT);
    uint32_t total = 0, err = 0;
    {
        ProfSpan sp(c, "gap_select");
        hipLaunchKernelGGL(gap_select_assess_kernel, grid, block, 0, c->stream, A);
        hipLaunchKernelGGL(gap_select_count_kernel, grid, block, 0, c->stream, A);
        HIPCHK(c, hipGetLastError());
        if ((rc = device_scan(c, A.cnt, A.cnt, n_reads, &total))) return rc; /* waits: the caller's arrays are free again */
        if (total) {
            if ((rc = d_out.alloc(c, (uint64_t)total * sizeof(GapCand)))) return rc;
            A.out = d_out.as<GapCand>(); A.out_cap = total;
            hipLaunchKernelGGL(gap_select_fill_kernel, grid, block, 0, c->stream, A);
            HIPCHK(c, hipGetLastError());
        }
    }
    o->rec.resize(total);
    if (total) HIPCHK(c, hipMemcpyAsync(o->rec.data(), d_out.p, (uint64_t)total * sizeof(GapCand), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&err, d_err.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, main_wait(c));
    if (err & GSEL_ERR_PROBE) return fail(c, NTL_EINTERNAL, "ntl_gap_select: a probe sequence did not end within the pair table (gap_select_kernels.h)");
    if (err & GSEL_ERR_SAME_CTG) return fail(c, NTL_EINVAL, "ntl_gap_select: two valid mappings of one read name the same contig");
    *out = o.release();
    return NTL_OK;
}

extern "C" uint64_t ntl_gap_cands_count(const ntl_gap_cands *s) { return s ? s->rec.size() : 0; }

extern "C" int ntl_gap_cands_copy(const ntl_gap_cands *s, ntl_gap_cand *out)
{
    if (!s || (!out && !s->rec.empty())) return NTL_EINVAL;
    if (!s->rec.empty()) memcpy(out, s->rec.data(), s->rec.size() * sizeof(GapCand));
    return NTL_OK;
}

extern "C" void ntl_gap_cands_destroy(ntl_gap_cands *s) { delete s; }

/* hit_doff[m] = hits of the mappings before m (the dense numbering of the hits); needs a completed result */
static int mapres_dense_offsets(const ntl_mapres *r)
{
    if (r->doff_made) return NTL_OK;
    ntl_ctx *c = r->c;
    int rc;
    if ((rc = r->hit_doff.alloc(c, (r->n_maps + 1) * 4))) return rc;
    if (r->n_maps) {
        hipLaunchKernelGGL(map_nhits_kernel, dim3((unsigned)((r->n_maps + 255) / 256)), dim3(256), 0, c->stream, (const MapRec *)r->maps.as<MapRec>(),
                           (uint32_t)r->n_maps, r->hit_doff.as<uint32_t>());
        if ((rc = device_scan(c, r->hit_doff.as<uint32_t>(), r->hit_doff.as<uint32_t>(), r->n_maps, nullptr))) return rc;
    } else HIPCHK(c, hipMemsetAsync(r->hit_doff.p, 0, 4, c->stream));
    HIPCHK(c, hipGetLastError());
    r->doff_made = true;
    return NTL_OK;
}

/* the dense copy of mappings and hits that the host receives (the device keeps the hits in their per-read regions) */
static int mapres_densify(const ntl_mapres *r)
{
    if (r->dense_made) return NTL_OK;
    ntl_ctx *c = r->c;
    int rc;
    if ((rc = mapres_dense_offsets(r)) || (rc = r->maps_dense.alloc(c, (r->n_maps + 1) * sizeof(MapRec))) ||
        (rc = r->hits_dense.alloc(c, (r->n_hits + 1) * sizeof(HitRec))))
        return rc;
    if (r->n_maps)
        hipLaunchKernelGGL(map_densify_kernel, dim3((unsigned)r->n_maps), dim3(64), 0, c->stream, (const MapRec *)r->maps.as<MapRec>(), (uint32_t)r->n_maps,
                           (const HitRec *)r->hits.as<HitRec>(), (const uint32_t *)r->hit_doff.as<uint32_t>(), r->maps_dense.as<MapRec>(),
                           r->hits_dense.as<HitRec>());
    HIPCHK(c, hipGetLastError());
    r->dense_made = true;
    return NTL_OK;
}

extern "C" int ntl_mapres_download(const ntl_mapres *r, ntl_mapping *maps, ntl_hit *hits, ntl_paf *pafs)
{
    if (!r) return NTL_EINVAL;
    ntl_ctx *c = r->c;
    (void)hipSetDevice(c->device);
    if (int frc = mapres_finalize(r)) return frc;
    if ((maps || hits) && r->n_maps) {
        if (int drc = mapres_densify(r)) return drc;
        if (maps) HIPCHK(c, hipMemcpyAsync(maps, r->maps_dense.p, r->n_maps * sizeof(MapRec), hipMemcpyDeviceToHost, c->stream));
        if (hits && r->n_hits) HIPCHK(c, hipMemcpyAsync(hits, r->hits_dense.p, r->n_hits * sizeof(HitRec), hipMemcpyDeviceToHost, c->stream));
    }
    if (pafs && r->n_pafs) HIPCHK(c, hipMemcpyAsync(pafs, r->pafs.p, r->n_pafs * sizeof(PafRec), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, main_wait(c));
    return NTL_OK;
}

/* ------------------------------------------------------------------ liftover of a resident result ---- */

static_assert(sizeof(ntl_lift_entry) == sizeof(LiftEntry) && sizeof(LiftEntry) == 20 && sizeof(LiftLine) == 16 && sizeof(LiftInfo) == 16,
              "ABI record must match the device record");
static_assert(NTL_LIFT_LANE_LINES == LIFT_LANE_LINES, "constant of the ABI and of liftover_kernels.h");

/* Five launches and a scan on MAIN (liftover_kernels.h), all sized by the input's counts, and ONE wait behind them: the error word,
   the hits and the mappings of the output come back together.  Every temporary is a block of the context's cache. */
extern "C" int ntl_mapres_liftover(ntl_ctx *c, const ntl_mapres *in, const ntl_lift_entry *table, uint32_t n_ctg, int32_t k, ntl_mapres **out)
{
    if (!c || !in || !out) return NTL_EINVAL;
    *out = nullptr;
    (void)hipSetDevice(c->device);
    if (n_ctg && !table) return fail(c, NTL_EINVAL, "ntl_mapres_liftover: a null table with a non-zero count");
    if (k < 1) return fail(c, NTL_EINVAL, "ntl_mapres_liftover: k must be at least 1");
    if (in->c->device != c->device) return fail(c, NTL_EINVAL, "ntl_mapres_liftover: the result lives on another device");
    for (uint32_t i = 0; i < n_ctg; i++) {
        const ntl_lift_entry &E = table[i];
        if (E.mode > 3u) return fail(c, NTL_EINVAL, "ntl_mapres_liftover: table entry " + std::to_string(i) + " has mode " + std::to_string(E.mode));
        if (E.mode && (!E.scaf_start || !E.ctg_start))
            return fail(c, NTL_EINVAL, "ntl_mapres_liftover: table entry " + std::to_string(i) + " has a start of 0 (AGP coordinates count from 1)");
        if (E.mode && E.ctg_end < E.ctg_start)
            return fail(c, NTL_EINVAL, "ntl_mapres_liftover: table entry " + std::to_string(i) + " ends in front of its start");
    }
    if (int frc = mapres_finalize(in)) return fail(c, frc, "ntl_mapres_liftover: the input result failed: " + in->c->err);
    if (in->c != c) HIPCHK(c, sync_both(in->c)); /* its records were made on another context's streams */
    const uint64_t n_maps = in->n_maps, cap = in->rec_cap;
    MapResPtr R = mapres_new(c, ntl_map_params());
    R->rec_cap = std::max<uint64_t>(cap, 1);
    int rc;
    if ((rc = R->maps.alloc(c, (n_maps + 1) * sizeof(MapRec))) || (rc = R->hits.alloc(c, (cap + 1) * sizeof(HitRec))) ||
        (rc = R->pafs.alloc(c, sizeof(PafRec)))) return mapres_fail(R, rc, false);
    if (!n_maps) { *out = R.release(); return NTL_OK; }
    DevBuf tab, kept, line, bytes, words, info;
    if ((rc = tab.alloc(c, ((uint64_t)n_ctg + 1) * sizeof(LiftEntry))) || (rc = kept.alloc(c, (cap + 1) * sizeof(HitRec))) ||
        (rc = line.alloc(c, n_maps * sizeof(LiftLine))) || (rc = bytes.alloc(c, 3 * n_maps)) || (rc = words.alloc(c, (5 * n_maps + 1) * 4)) ||
        (rc = info.alloc(c, sizeof(LiftInfo))))
        return mapres_fail(R, rc, false);
    LiftArgs A = {};
    A.maps = in->maps.as<MapRec>(); A.hits = in->hits.as<HitRec>(); A.hits_cap = cap;
    A.n_maps = (uint32_t)n_maps; A.n_ctg = n_ctg; A.k = k; A.table = tab.as<LiftEntry>();
    A.kept_hits = kept.as<HitRec>(); A.line = line.as<LiftLine>();
    A.mono = bytes.as<uint8_t>(); A.cov = A.mono + n_maps; A.drop = A.cov + n_maps;
    A.gfirst = words.as<uint32_t>(); A.goff = A.gfirst + n_maps; A.gcnt = A.goff + n_maps; A.over_list = A.gcnt + n_maps; A.emit = A.over_list + n_maps;
    A.info = info.as<LiftInfo>();
    A.out_maps = R->maps.as<MapRec>(); A.out_hits = R->hits.as<HitRec>();
    LiftInfo hinfo = {};
    uint32_t n_out = 0;
    hipError_t e = hipSuccess;
    {
        ProfSpan sp(c, "liftover");
        if (n_ctg) e = hipMemcpyAsync(tab.p, table, (uint64_t)n_ctg * sizeof(LiftEntry), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(info.p, 0, sizeof(LiftInfo), c->stream);
        if (e == hipSuccess) {
            const unsigned per_wave = (unsigned)((n_maps + LIFT_NT / 64 - 1) / (LIFT_NT / 64)), per_lane = (unsigned)((n_maps + LIFT_NT - 1) / LIFT_NT);
            hipLaunchKernelGGL(lift_line_kernel, dim3(per_wave), dim3(LIFT_NT), 0, c->stream, A);
            hipLaunchKernelGGL(lift_read_kernel, dim3(per_lane), dim3(LIFT_NT), 0, c->stream, A);
            hipLaunchKernelGGL(lift_read_overflow_kernel, dim3((unsigned)std::min<uint64_t>(n_maps / (LIFT_LANE_LINES + 1) + 1, LIFT_OVER_BLOCKS)), dim3(64), 0,
                               c->stream, A);
            e = hipGetLastError();
            if (e == hipSuccess && (rc = device_scan(c, A.emit, A.emit, n_maps, nullptr))) return mapres_fail(R, rc, true);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(lift_gather_kernel, dim3(per_wave), dim3(LIFT_NT), 0, c->stream, A);
                e = hipGetLastError();
            }
        }
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&hinfo, info.p, sizeof(LiftInfo), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&n_out, A.emit + n_maps, 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = main_wait(c); /* the one wait; the caller's table is free again */
    if (e != hipSuccess) return mapres_fail(R, fail(c, NTL_EDEVICE, std::string("ntl_mapres_liftover: ") + hipGetErrorString(e)), true);
    if (hinfo.err & LIFT_ERR_CTG) return mapres_fail(R, fail(c, NTL_EINVAL, "ntl_mapres_liftover: a mapping names a contig that the table does not hold (ctg >= n_ctg)"), true);
    if (hinfo.err & LIFT_ERR_REGION) return mapres_fail(R, fail(c, NTL_EINTERNAL, "ntl_mapres_liftover: a mapping's hit region leaves the hit array"), true);
    if (hinfo.err & LIFT_ERR_RANGE) return mapres_fail(R, fail(c, NTL_ERANGE, "ntl_mapres_liftover: a lifted position does not fit 32 bits"), true);
    R->n_maps = n_out; R->n_hits = hinfo.n_hits;
    *out = R.release();
    return NTL_OK;
}

/* ------------------------------------------------------------------ pair records of a resident result ---- */

static_assert(sizeof(ntl_pair_rec) == sizeof(PairRec) && sizeof(PairRec) == 24 && sizeof(PairLine) == 32 && sizeof(PairInfo) == 16 && sizeof(PairCtg) == 8,
              "ABI record must match the device record");
static_assert(NTL_PAIR_LANE_MAPS == PAIR_LANE_MAPS, "constant of the ABI and of pair_kernels.h");

struct ntl_pairtab {
    ntl_ctx *c;
    uint64_t n_ctg = 0;
    int32_t k = 0, f = 0;
    DevBuf tab; /* PairCtg[n_ctg] */
};

struct ntl_pairs {
    ntl_ctx *c;
    uint64_t n = 0;
    DevBuf recs; /* PairRec[n] (sized for the most the mappings could make) */
};

extern "C" int ntl_pairtab_create(ntl_ctx *c, const ntl_tally *t, ntl_pairtab **out)
{
    if (!c || !t || !out) return NTL_EINVAL;
    *out = nullptr;
    (void)hipSetDevice(c->device);
    const TallyView V = ntl_tally_view(t);
    std::unique_ptr<ntl_pairtab> pt(new ntl_pairtab());
    pt->c = c; pt->n_ctg = V.n_ctg; pt->k = V.k; pt->f = V.f;
    std::vector<PairCtg> host(V.n_ctg);
    for (uint64_t i = 0; i < V.n_ctg; i++) host[i] = {V.rank[i], V.ctg_len[i]};
    if (int rc = pt->tab.alloc(c, (V.n_ctg + 1) * sizeof(PairCtg))) return rc;
    if (V.n_ctg) HIPCHK(c, hipMemcpyAsync(pt->tab.p, host.data(), V.n_ctg * sizeof(PairCtg), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, main_wait(c)); /* complete for every context of the device */
    *out = pt.release();
    return NTL_OK;
}

extern "C" void ntl_pairtab_destroy(ntl_pairtab *pt) { delete pt; }

/* Three launches, the scan and two more launches on MAIN (pair_kernels.h), all sized by the result's counts, and ONE wait behind them:
   the error word and the number of records come back together.  The records' array cannot wait for that number: it is sized from
   what n_maps mappings could make at most -- per read of m lines m (m - 1) / 2 <= m * (f / 2) in the first branch (m <= f) and fewer
   than 2 m in the second; never more than n_maps (n_maps - 1) / 2 in all.  Every temporary is a block of the context's cache. */
extern "C" int ntl_mapres_pairs(const ntl_mapres *r, const ntl_pairtab *pt, const uint32_t *read_len, uint64_t n_reads, ntl_pairs **out)
{
    if (!r || !pt || !out) return NTL_EINVAL;
    *out = nullptr;
    ntl_ctx *c = r->c;
    (void)hipSetDevice(c->device);
    if (r->grouped) return fail(c, NTL_EINVAL, "ntl_mapres_pairs: a grouped result has no pair tally");
    if (pt->c->device != c->device) return fail(c, NTL_EINVAL, "ntl_mapres_pairs: the table lives on another device");
    if (n_reads > 0xFFFFFFFFull) return fail(c, NTL_EINVAL, "ntl_mapres_pairs: read numbers are 32 bits");
    if (int frc = mapres_finalize(r)) return fail(c, frc, "ntl_mapres_pairs: the result failed: " + c->err);
    const uint64_t n_maps = r->n_maps;
    std::unique_ptr<ntl_pairs> P(new ntl_pairs());
    P->c = c;
    if (!n_maps) { *out = P.release(); return NTL_OK; }
    const uint64_t per = pt->f < 0 ? n_maps : std::max<uint64_t>(2, (uint64_t)pt->f / 2);
    const uint64_t cap = std::min<uint64_t>(std::min<uint64_t>(n_maps * std::min<uint64_t>(per, n_maps), n_maps * (n_maps - 1) / 2), PAIR_MAX_RECS);
    DevBuf line, key1, words, info, rlen;
    int rc;
    if ((rc = P->recs.alloc(c, (cap + 1) * sizeof(PairRec))) || (rc = line.alloc(c, n_maps * sizeof(PairLine))) || (rc = key1.alloc(c, n_maps * 8)) ||
        (rc = words.alloc(c, (2 * n_maps + 1) * 4)) || (rc = info.alloc(c, sizeof(PairInfo))) || (read_len && (rc = rlen.alloc(c, (n_reads + 1) * 4))))
        return rc;
    PairArgs A = {};
    A.maps = r->maps.as<MapRec>(); A.hits = r->hits.as<HitRec>(); A.hits_cap = r->rec_cap;
    A.n_maps = (uint32_t)n_maps; A.n_ctg = (uint32_t)pt->n_ctg; A.k = pt->k; A.f = pt->f;
    A.table = pt->tab.as<PairCtg>(); A.read_len = read_len ? rlen.as<uint32_t>() : nullptr; A.n_reads = n_reads;
    A.line = line.as<PairLine>(); A.key1 = key1.as<uint64_t>();
    A.over_list = words.as<uint32_t>(); A.cnt = A.over_list + n_maps;
    A.info = info.as<PairInfo>();
    A.out = P->recs.as<PairRec>(); A.out_cap = cap;
    PairInfo hinfo = {};
    hipError_t e = hipSuccess;
    {
        ProfSpan sp(c, "pairs");
        if (read_len && n_reads) e = hipMemcpyAsync(rlen.p, read_len, n_reads * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(info.p, 0, sizeof(PairInfo), c->stream);
        if (e == hipSuccess) {
            const unsigned per_lane = (unsigned)((n_maps + PAIR_NT - 1) / PAIR_NT);
            const unsigned over = (unsigned)std::min<uint64_t>(n_maps / (PAIR_LANE_MAPS + 1) + 1, PAIR_OVER_BLOCKS);
            hipLaunchKernelGGL(pair_line_kernel, dim3(per_lane), dim3(PAIR_NT), 0, c->stream, A);
            hipLaunchKernelGGL((pair_read_kernel<false>), dim3(per_lane), dim3(PAIR_NT), 0, c->stream, A);
            hipLaunchKernelGGL((pair_read_overflow_kernel<false>), dim3(over), dim3(64), 0, c->stream, A);
            e = hipGetLastError();
            if (e == hipSuccess && (rc = device_scan(c, A.cnt, A.cnt, n_maps, nullptr))) return rc;
            if (e == hipSuccess) {
                hipLaunchKernelGGL((pair_read_kernel<true>), dim3(per_lane), dim3(PAIR_NT), 0, c->stream, A);
                hipLaunchKernelGGL((pair_read_overflow_kernel<true>), dim3(over), dim3(64), 0, c->stream, A);
                e = hipGetLastError();
            }
        }
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&hinfo, info.p, sizeof(PairInfo), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = main_wait(c); /* the one wait; the caller's lengths are free again */
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream); /* the blocks return to the cache behind whatever still runs */
        return fail(c, NTL_EDEVICE, std::string("ntl_mapres_pairs: ") + hipGetErrorString(e));
    }
    if (hinfo.err & PAIR_ERR_CTG) return fail(c, NTL_EINVAL, "ntl_mapres_pairs: a mapping names a contig that the table does not hold (ctg >= the tally's contigs)");
    if (hinfo.err & PAIR_ERR_READ) return fail(c, NTL_EINVAL, "ntl_mapres_pairs: a mapping names a read that read_len does not hold (read >= n_reads)");
    if (hinfo.err & PAIR_ERR_REGION) return fail(c, NTL_EINTERNAL, "ntl_mapres_pairs: a mapping without a hit, or one whose hit region leaves the hit array");
    if (hinfo.err & PAIR_ERR_NEGATIVE) return fail(c, NTL_ERANGE, "ntl_mapres_pairs: Gap distance estimation less than 0");
    if (hinfo.total >= PAIR_MAX_RECS) return fail(c, NTL_ERANGE, "ntl_mapres_pairs: the result makes 2^32 - 256 pair records or more");
    P->n = hinfo.total;
    *out = P.release();
    return NTL_OK;
}

extern "C" uint64_t ntl_pairs_count(const ntl_pairs *p) { return p ? p->n : 0; }

extern "C" int ntl_pairs_download(const ntl_pairs *p, ntl_pair_rec *out)
{
    if (!p || (p->n && !out)) return NTL_EINVAL;
    ntl_ctx *c = p->c;
    (void)hipSetDevice(c->device);
    if (!p->n) return NTL_OK;
    HIPCHK(c, hipMemcpyAsync(out, p->recs.p, p->n * sizeof(PairRec), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, main_wait(c));
    return NTL_OK;
}

extern "C" void ntl_pairs_destroy(ntl_pairs *p) { delete p; }

/* ------------------------------------------------------------------ text on the device ---- */

struct ntl_names {
    ntl_ctx *c;
    uint64_t n = 0;
    uint64_t max_len = 0; /* the longest name: bounds the bytes of a header / PAF line (ntl_mapres_format) */
    DevBuf blob, off, len; /* bytes, u64[n + 1], u32[n] (or none) */
};

extern "C" int ntl_names_create(ntl_ctx *c, const char *blob, const uint64_t *off, const uint32_t *len, uint64_t n, ntl_names **out)
{
    if (!c || !out || (n && (!blob || !off))) return NTL_EINVAL;
    *out = nullptr;
    (void)hipSetDevice(c->device);
    std::unique_ptr<ntl_names> t(new ntl_names());
    t->c = c; t->n = n;
    const uint64_t zero = 0;
    const uint64_t bytes = n ? off[n] : 0;
    for (uint64_t i = 0; i < n; i++) t->max_len = std::max<uint64_t>(t->max_len, off[i + 1] - off[i]);
    int rc;
    if ((rc = t->blob.alloc(c, bytes + 16)) || (rc = t->off.alloc(c, (n + 1) * 8)) || (len && (rc = t->len.alloc(c, (n + 1) * 4)))) return rc;
    if (bytes) HIPCHK(c, hipMemcpyAsync(t->blob.p, blob, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(t->off.p, n ? (const void *)off : (const void *)&zero, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (len && n) HIPCHK(c, hipMemcpyAsync(t->len.p, len, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, main_wait(c)); /* the caller's arrays are free again */
    *out = t.release();
    return NTL_OK;
}

extern "C" void ntl_names_destroy(ntl_names *t)
{
    if (!t) return;
    (void)hipSetDevice(t->c->device);
    delete t;
}

struct ntl_text {
    ntl_ctx *c;
    uint64_t verbose_bytes = 0, paf_bytes = 0, n_maps = 0;
    DevBuf verbose, paf, ends, maps;
};

/* Makes the text of a map result on the device.  One host wait: the three byte totals decide the size of the text arrays. */
extern "C" int ntl_mapres_format(const ntl_mapres *r, const ntl_names *reads, const ntl_names *contigs, int want_verbose, int want_paf,
                                 ntl_text **out)
{
    if (!r || !reads || !contigs || !out) return NTL_EINVAL;
    *out = nullptr;
    ntl_ctx *c = r->c;
    (void)hipSetDevice(c->device);
    if (int frc = mapres_finalize(r)) return frc;
    if (!reads->len.p || !contigs->len.p) return fail(c, NTL_EINVAL, "ntl_mapres_format: both name tables need their lengths");
    if (r->n_hits >= 0xFFFFFF00ull || r->n_maps >= 0xFFFFFF00ull) return fail(c, NTL_ERANGE, "ntl_mapres_format: too many records for one text");
    /* 32-bit offsets, every one of the three scans (tokens, headers, PAF lines) bounded on its own: a token is at most 27 bytes, a header
       two names + a count + three separators, a PAF line two names + ten numbers + strand and tabs (the header and PAF
       sums could wrap unseen and the fill kernel then wrote at wrapped offsets) */
    {
        const uint64_t names2 = reads->max_len + contigs->max_len;
        const uint64_t tok_b = r->n_hits * 27, hdr_b = r->n_maps * (names2 + 16), paf_b = r->n_pafs * (names2 + 10 * 11 + 16);
        uint64_t most = 0xFFFFFF00ull;
        if (const char *e = getenv("NTL_FORMAT_MAX_TEXT")) most = (uint64_t)atoll(e); /* tests: the caller's fallback without 4 GB of text */
        if (tok_b + hdr_b >= most || paf_b >= most)
            return fail(c, NTL_ERANGE, "ntl_mapres_format: the text of this batch may exceed 4 GB (32-bit offsets): format it on the host, or map smaller batches");
    }
    std::unique_ptr<ntl_text> t(new ntl_text());
    t->c = c; t->n_maps = r->n_maps;
    const uint32_t nm = (uint32_t)r->n_maps, nh = want_verbose ? (uint32_t)r->n_hits : 0u, np = want_paf ? (uint32_t)r->n_pafs : 0u;
    DevBuf tok, hdr, pl;
    int rc;
    if ((rc = tok.alloc(c, ((uint64_t)nh + 1) * 4)) || (rc = hdr.alloc(c, ((uint64_t)nm + 1) * 4)) || (rc = pl.alloc(c, ((uint64_t)np + 1) * 4)) ||
        (rc = t->ends.alloc(c, ((uint64_t)r->n_maps * 2 + 1) * sizeof(HitRec))) || (rc = t->maps.alloc(c, ((uint64_t)r->n_maps + 1) * sizeof(MapRec))))
        return rc;
    if ((rc = mapres_dense_offsets(r))) return rc;
    FmtArgs A;
    A.hit_doff = r->hit_doff.as<uint32_t>();
    A.maps = r->maps.as<MapRec>(); A.hits = r->hits.as<HitRec>(); A.pafs = r->pafs.as<PafRec>();
    A.n_maps = nm; A.n_hits = nh; A.n_pafs = np; A.do_verbose = want_verbose ? 1 : 0;
    A.read_name_off = reads->off.as<uint64_t>(); A.read_names = reads->blob.as<char>();
    A.ctg_name_off = contigs->off.as<uint64_t>(); A.ctg_names = contigs->blob.as<char>();
    A.read_len = reads->len.as<uint32_t>(); A.ctg_len = contigs->len.as<uint32_t>();
    A.tok_len = tok.as<uint32_t>(); A.hdr_len = hdr.as<uint32_t>(); A.paf_len = pl.as<uint32_t>();
    A.verbose = nullptr; A.paf = nullptr; A.ends = t->ends.as<HitRec>(); A.maps_out = t->maps.as<MapRec>();
    const uint64_t most = std::max<uint64_t>(std::max<uint64_t>(nh, nm), np);
    uint32_t tot[3] = {0, 0, 0};
    if (most) {
        ProfSpan sp(c, "format");
        const unsigned grid = (unsigned)((most + 255) / 256);
        hipLaunchKernelGGL(fmt_len_kernel, dim3(grid), dim3(256), 0, c->stream, A);
        if (!want_verbose) HIPCHK(c, hipMemsetAsync(A.hdr_len, 0, ((uint64_t)nm + 1) * 4, c->stream));
        if ((rc = device_scan(c, A.tok_len, A.tok_len, nh, nullptr)) || (rc = device_scan(c, A.hdr_len, A.hdr_len, nm, nullptr)) ||
            (rc = device_scan(c, A.paf_len, A.paf_len, np, nullptr)))
            return rc;
        HIPCHK(c, hipMemcpyAsync(&tot[0], A.tok_len + nh, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&tot[1], A.hdr_len + nm, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&tot[2], A.paf_len + np, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, main_wait(c));
        t->verbose_bytes = (uint64_t)tot[0] + tot[1];
        t->paf_bytes = tot[2];
        if (t->verbose_bytes >= 0xFFFFFFFFull) return fail(c, NTL_ERANGE, "ntl_mapres_format: more than 4 GB of text in one batch");
        if ((rc = t->verbose.alloc(c, t->verbose_bytes + 16)) || (rc = t->paf.alloc(c, t->paf_bytes + 16))) return rc;
        A.verbose = t->verbose.as<char>(); A.paf = t->paf.as<char>();
        hipLaunchKernelGGL(fmt_fill_kernel, dim3(grid), dim3(256), 0, c->stream, A);
        HIPCHK(c, hipGetLastError());
    }
    *out = t.release();
    return NTL_OK;
}

extern "C" void ntl_text_sizes(const ntl_text *t, uint64_t *verbose_bytes, uint64_t *paf_bytes, uint64_t *n_maps)
{
    if (verbose_bytes) *verbose_bytes = t ? t->verbose_bytes : 0;
    if (paf_bytes) *paf_bytes = t ? t->paf_bytes : 0;
    if (n_maps) *n_maps = t ? t->n_maps : 0;
}

extern "C" int ntl_text_download(const ntl_text *t, char *verbose, char *paf, ntl_mapping *maps, ntl_hit *ends)
{
    if (!t) return NTL_EINVAL;
    ntl_ctx *c = t->c;
    (void)hipSetDevice(c->device);
    if (verbose && t->verbose_bytes) HIPCHK(c, hipMemcpyAsync(verbose, t->verbose.p, t->verbose_bytes, hipMemcpyDeviceToHost, c->stream));
    if (paf && t->paf_bytes) HIPCHK(c, hipMemcpyAsync(paf, t->paf.p, t->paf_bytes, hipMemcpyDeviceToHost, c->stream));
    if (maps && t->n_maps) HIPCHK(c, hipMemcpyAsync(maps, t->maps.p, t->n_maps * sizeof(MapRec), hipMemcpyDeviceToHost, c->stream));
    if (ends && t->n_maps) HIPCHK(c, hipMemcpyAsync(ends, t->ends.p, t->n_maps * 2 * sizeof(HitRec), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, main_wait(c));
    return NTL_OK;
}

extern "C" void ntl_text_destroy(ntl_text *t)
{
    if (!t) return;
    (void)hipSetDevice(t->c->device);
    delete t;
}

/* ------------------------------------------------------------------ a sketch's text on the device ---- */

/* One text, one size: a sibling of ntl_text, whose sizes and download speak of a map result's two files, mappings and hit ends. */
struct ntl_sktext {
    ntl_ctx *c;
    uint64_t bytes = 0;
    DevBuf text;
};

extern "C" uint64_t ntl_sketch_text_limit(void)
{
    uint64_t most = 0xFFFFFF00ull; /* 32-bit offsets */
    if (const char *e = getenv("NTL_SKETCH_TEXT_MAX_BYTES")) most = std::min<uint64_t>(most, strtoull(e, nullptr, 10)); /* tests: pieces without 4 GB of text */
    return most;
}

extern "C" uint64_t ntl_sketch_text_bound(const ntl_names *names, uint64_t n_seq, uint64_t n_mx)
{
    return n_mx * SKTEXT_TOKEN_MAX + n_seq * ((names ? names->max_len : 0) + SKTEXT_HEADER_EXTRA);
}

/* The length pass, two scans and the fill pass on MAIN (sketch_text_kernels.h), every temporary a block of the context's cache.  ONE wait
   between the scans and the fill: the two totals land in a page-locked slot (pending.h) and size the text.  The first call on a sketch
   also fetches its nseq + 1 offsets, once: the minimizers of a range size the launches and bound its bytes. */
extern "C" int ntl_sketch_format(const ntl_sketch *s, const ntl_names *names, int flags, uint64_t seq_lo, uint64_t seq_hi, ntl_sktext **out)
{
    if (!s || !names || !out) return NTL_EINVAL;
    *out = nullptr;
    ntl_ctx *c = s->c;
    (void)hipSetDevice(c->device);
    if (flags & ~(NTL_SKETCH_TEXT_LEN | NTL_SKETCH_TEXT_STRAND)) return fail(c, NTL_EINVAL, "ntl_sketch_format: unknown flag bits");
    if (s->no_records) return fail(c, NTL_EINVAL, "ntl_sketch_format: a sketch made by ntl_sketch_run_for_map holds no records");
    if (names->c->device != c->device) return fail(c, NTL_EINVAL, "ntl_sketch_format: the name table lives on another device");
    if (names->n < s->nseq) return fail(c, NTL_EINVAL, "ntl_sketch_format: the name table holds fewer names than the sketch has sequences");
    if (seq_lo > seq_hi || seq_hi > s->nseq)
        return fail(c, NTL_EINVAL, "ntl_sketch_format: the range [" + std::to_string(seq_lo) + ", " + std::to_string(seq_hi) + ") is not one of the sketch's " +
                                       std::to_string(s->nseq) + " sequences");
    if ((flags & NTL_SKETCH_TEXT_LEN) && names->n && !names->len.p) return fail(c, NTL_EINVAL, "ntl_sketch_format: the length column needs a name table with lengths");
    if (int frc = sketch_finalize(s)) return fail(c, frc, "ntl_sketch_format: the sketch failed: " + c->err);
    if (s->h_off.empty()) {
        s->h_off.resize(s->nseq + 1);
        hipError_t e = hipMemcpyAsync(s->h_off.data(), s->mx_off.p, (s->nseq + 1) * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = main_wait(c);
        if (e != hipSuccess) { s->h_off.clear(); return fail(c, NTL_EDEVICE, std::string("ntl_sketch_format: ") + hipGetErrorString(e)); }
    }
    const uint64_t n_seq = seq_hi - seq_lo, n_mx = s->h_off[seq_hi] - s->h_off[seq_lo];
    const uint64_t bound = ntl_sketch_text_bound(names, n_seq, n_mx), most = ntl_sketch_text_limit();
    if (bound >= most)
        return fail(c, NTL_ERANGE, "ntl_sketch_format: the text of sequences [" + std::to_string(seq_lo) + ", " + std::to_string(seq_hi) + ") may take " +
                                       std::to_string(bound) + " bytes, one call makes fewer than " + std::to_string(most) +
                                       " (32-bit offsets; NTL_SKETCH_TEXT_MAX_BYTES): format fewer sequences per call");
    std::unique_ptr<ntl_sktext> t(new ntl_sktext());
    t->c = c;
    if (!n_seq) { *out = t.release(); return NTL_OK; }
    DevBuf tok, hdr;
    int rc;
    if ((rc = tok.alloc(c, (n_mx + 1) * 4)) || (rc = hdr.alloc(c, (n_seq + 1) * 4))) return rc;
    SkTextArgs A = {};
    A.recs = s->records.as<MxRecord>(); A.mx_off = s->mx_off.as<uint32_t>();
    A.name_off = names->off.as<uint64_t>(); A.names = names->blob.as<char>(); A.seq_len = names->len.as<uint32_t>();
    A.seq_lo = (uint32_t)seq_lo; A.n_seq = (uint32_t)n_seq; A.mx_lo = s->h_off[seq_lo]; A.n_mx = (uint32_t)n_mx;
    A.with_len = flags & NTL_SKETCH_TEXT_LEN ? 1 : 0; A.with_strand = flags & NTL_SKETCH_TEXT_STRAND ? 1 : 0;
    A.tok_len = tok.as<uint32_t>(); A.hdr_len = hdr.as<uint32_t>(); A.text = nullptr;
    const unsigned grid = (unsigned)((std::max(n_mx, n_seq) + SKTEXT_NT - 1) / SKTEXT_NT);
    Pending p;
    if (!p.arm(c->pq)) return fail(c, NTL_EDEVICE, "ntl_sketch_format: no free result slot (too many pending results)");
    uint32_t *totals = (uint32_t *)c->pq.slot_dev(p.slot); /* [0] the tokens' bytes, [1] the headers' */
    ProfSpan sp(c, "sketch_text");
    hipLaunchKernelGGL((sktext_kernel<false>), dim3(grid), dim3(SKTEXT_NT), 0, c->stream, A);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && ((rc = device_scan(c, A.tok_len, A.tok_len, n_mx, nullptr, 1, totals)) || (rc = device_scan(c, A.hdr_len, A.hdr_len, n_seq, nullptr, 1, totals + 1))))
        return pending_abort(c, p, rc);
    if (e == hipSuccess) e = hipEventRecord(p.done, c->stream);
    if (e == hipSuccess) e = p.wait(); /* the one wait */
    if (e != hipSuccess) return pending_abort(c, p, fail(c, NTL_EDEVICE, std::string("ntl_sketch_format: ") + hipGetErrorString(e)));
    const uint32_t *got = (const uint32_t *)p.slot;
    t->bytes = (uint64_t)got[0] + got[1];
    p.settle(c->pq);
    if (t->bytes > bound) return fail(c, NTL_EINTERNAL, "ntl_sketch_format: the lengths exceed their bound");
    if ((rc = t->text.alloc(c, t->bytes + 16))) return rc;
    A.text = t->text.as<char>();
    hipLaunchKernelGGL((sktext_kernel<true>), dim3(grid), dim3(SKTEXT_NT), 0, c->stream, A);
    HIPCHK(c, hipGetLastError());
    *out = t.release();
    return NTL_OK;
}

extern "C" uint64_t ntl_sktext_bytes(const ntl_sktext *t) { return t ? t->bytes : 0; }

extern "C" int ntl_sktext_download(const ntl_sktext *t, char *out)
{
    if (!t || (t->bytes && !out)) return NTL_EINVAL;
    ntl_ctx *c = t->c;
    (void)hipSetDevice(c->device);
    if (!t->bytes) return NTL_OK;
    HIPCHK(c, hipMemcpyAsync(out, t->text.p, t->bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, main_wait(c));
    return NTL_OK;
}

extern "C" void ntl_sktext_destroy(ntl_sktext *t)
{
    if (!t) return;
    (void)hipSetDevice(t->c->device);
    delete t;
}
