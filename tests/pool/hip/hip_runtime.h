/*
 * A scripted stand-in for the HIP runtime: only what ntlink_amd/csrc/dev_pool.h and pending.h call.  TEST TOOL ONLY (tests/pool/pool_check.cpp,
 * pending_check.cpp).
 *
 * Streams belong to the test: each has a count of queued and of completed work.  An event records its stream's queued count and has
 * passed once the completed count reaches it; the test advances completion by hand (a host-side wait advances it too, and is counted).
 * Memory is address space only (nothing is ever dereferenced): hipMalloc hands out ranges that are never reused, refuses what would
 * take the live bytes over `limit`, and records every live range.
 */
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <atomic>
#include <map>
#include <mutex>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1, hipErrorNotReady = 600 };
enum { hipEventDisableTiming = 2, hipEventBlockingSync = 1 };

struct fake_stream {
    std::atomic<uint64_t> queued{0}, completed{0};
    void work(uint64_t n = 1) { queued += n; }
    void finish() { finish_to(queued); }
    void finish_to(uint64_t n) { uint64_t c = completed; while (c < n && !completed.compare_exchange_weak(c, n)) {} }
};
typedef fake_stream *hipStream_t;
struct fake_event { fake_stream *s = nullptr; uint64_t at = 0; };
typedef fake_event *hipEvent_t;

struct fake_runtime {
    std::mutex mu;
    std::map<uintptr_t, size_t> live; /* driver allocations: base -> bytes */
    size_t live_bytes = 0, limit = ~(size_t)0;
    uintptr_t next = (uintptr_t)1 << 44;
    uint64_t mallocs = 0, refused = 0, frees = 0, bad_frees = 0;
    std::atomic<uint64_t> stream_waits{0}, host_waits{0};
    std::atomic<int64_t> events{0};               /* created and not destroyed */
    fake_stream *waited_on = nullptr; fake_event waited_for; /* the last hipStreamWaitEvent */
};
inline fake_runtime fake;

inline hipError_t hipMalloc(void **out, size_t bytes)
{
    std::lock_guard<std::mutex> g(fake.mu);
    if (bytes > fake.limit || fake.live_bytes > fake.limit - bytes) { fake.refused++; *out = nullptr; return hipErrorOutOfMemory; }
    *out = (void *)fake.next;
    fake.live[fake.next] = bytes;
    fake.live_bytes += bytes;
    fake.next += (bytes + 4095) & ~(size_t)4095;
    fake.mallocs++;
    return hipSuccess;
}
inline hipError_t hipFree(void *p)
{
    std::lock_guard<std::mutex> g(fake.mu);
    auto it = fake.live.find((uintptr_t)p);
    if (it == fake.live.end()) { fake.bad_frees++; return hipErrorInvalidValue; }
    fake.live_bytes -= it->second;
    fake.live.erase(it);
    fake.frees++;
    return hipSuccess;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = new fake_event(); fake.events++; return hipSuccess; }
inline hipError_t hipEventDestroy(hipEvent_t e) { delete e; fake.events--; return hipSuccess; }
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { e->s = s; e->at = s->queued; return hipSuccess; }
inline hipError_t hipEventQuery(hipEvent_t e) { return !e->s || e->s->completed >= e->at ? hipSuccess : hipErrorNotReady; }
inline hipError_t hipEventSynchronize(hipEvent_t e) { fake.host_waits++; if (e->s) e->s->finish_to(e->at); return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t s) { fake.host_waits++; s->finish(); return hipSuccess; }
inline hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned)
{
    fake.stream_waits++; fake.waited_on = s; fake.waited_for = *e;
    return hipSuccess;
}
inline hipError_t hipGetLastError() { return hipSuccess; }
inline const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "scripted error"; }
