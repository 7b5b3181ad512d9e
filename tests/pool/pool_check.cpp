/*
 * Host test of the device block allocator (ntlink_amd/csrc/dev_pool.h) over the scripted runtime beside this file (hip/hip_runtime.h):
 * slabs on, streams advanced by hand, a driver that refuses on command.  One line per failed check, exit status 1 on any.
 * Built and run by tests/test_dev_pool.py (g++ -std=c++17 -I tests/pool, once with -fsanitize=address,undefined, once with =thread).
 */
#include "../../ntlink_amd/csrc/dev_pool.h"

#include <condition_variable>
#include <math.h>
#include <random>
#include <thread>

static int g_failed = 0;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            g_failed++;                                                                    \
            printf("FAILED %s:%d %s: ", __func__, __LINE__, #cond);                        \
            printf(__VA_ARGS__);                                                           \
            printf("\n");                                                                  \
        }                                                                                  \
    } while (0)

static const size_t MiB = (size_t)1 << 20, GiB = (size_t)1 << 30;
enum { MAIN = DevPool::MAIN, WINDOW = DevPool::WINDOW, BOTH = 3 };

/* a fresh runtime, two streams and a pool with slabs on; the pool is destroyed with it, and must then have freed all it allocated */
struct World {
    fake_stream A, B; /* MAIN, WINDOW */
    DevPool pool;
    explicit World(size_t bound = ~(size_t)0)
    {
        std::lock_guard<std::mutex> g(fake.mu);
        fake.live.clear();
        fake.live_bytes = 0; fake.limit = ~(size_t)0;
        fake.mallocs = fake.refused = fake.frees = fake.bad_frees = 0;
        fake.stream_waits = 0; fake.host_waits = 0; fake.events = 0;
        fake.waited_on = nullptr; fake.waited_for = fake_event();
        pool.setup(&A, &B, bound, true);
    }
    void finish() { A.finish(); B.finish(); }
    ~World()
    {
        pool.destroy();
        CHECK(fake.live.empty() && fake.frees == fake.mallocs && !fake.bad_frees && fake.events == 0,
              "after destroy: %zu live ranges, %llu hipMalloc, %llu hipFree, %llu bad, %lld events", fake.live.size(),
              (unsigned long long)fake.mallocs, (unsigned long long)fake.frees, (unsigned long long)fake.bad_frees, (long long)fake.events);
    }
};

/* the blocks the test holds: none may overlap another, each lies inside one driver allocation */
struct Live {
    std::mutex mu;
    std::map<uintptr_t, size_t> m;
    void add(void *p, size_t n, const char *what)
    {
        const uintptr_t a = (uintptr_t)p;
        {
            std::lock_guard<std::mutex> g(fake.mu);
            auto d = fake.live.upper_bound(a);
            const bool inside = d != fake.live.begin() && (--d, a >= d->first && a + n <= d->first + d->second);
            CHECK(inside, "%s: %zu bytes at %#zx lie in no driver allocation", what, n, (size_t)a);
        }
        std::lock_guard<std::mutex> g(mu);
        auto nx = m.lower_bound(a);
        CHECK(nx == m.end() || a + n <= nx->first, "%s: %#zx+%zu overlaps the live block at %#zx", what, (size_t)a, n, (size_t)nx->first);
        if (nx != m.begin()) { auto pv = std::prev(nx); CHECK(pv->first + pv->second <= a, "%s: %#zx overlaps the live block %#zx+%zu", what, (size_t)a, (size_t)pv->first, pv->second); }
        m[a] = n;
    }
    void remove(void *p) { std::lock_guard<std::mutex> g(mu); m.erase((uintptr_t)p); }
};

/* blocks on their way to the thread that does not own the pool */
struct Queue {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::pair<void *, size_t>> q;
    bool closed = false;
    void push(void *p, size_t n) { { std::lock_guard<std::mutex> g(mu); q.push_back({p, n}); } cv.notify_one(); }
    void close() { { std::lock_guard<std::mutex> g(mu); closed = true; } cv.notify_one(); }
    bool pop(std::pair<void *, size_t> *out)
    {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return closed || !q.empty(); });
        if (q.empty()) return false;
        *out = q.front(); q.pop_front();
        return true;
    }
};

/* Cases 1 and 7: a few thousand random calls, sizes from 1 B to 300 MB (both sides of the 1-MB size-class threshold and of the 192-MB
   slab limit), streams that run ahead and catch up at random.  With `foreign`, a share of the uncached blocks is freed by that thread. */
static void random_calls(unsigned seed, Queue *foreign)
{
    World w(4 * GiB);
    Live live;
    std::mt19937_64 rng(seed);
    auto uni = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); };
    struct Held { void *p; size_t bytes; unsigned used; bool cached; };
    std::vector<Held> held;
    std::map<void *, std::pair<uint64_t, uint64_t>> freed; /* an uncached block given back: what was queued on either stream then */
    std::thread other;
    if (foreign)
        other = std::thread([&] {
            std::pair<void *, size_t> b;
            while (foreign->pop(&b)) { live.remove(b.first); w.pool.free_uncached(b.first, b.second); }
        });
    for (int i = 0; i < 4000; i++) {
        const double r = uni(0, 1);
        const size_t n = (size_t)exp(uni(0, log(300e6)));
        if (held.size() < 48 && r < 0.35) {
            const int sid = uni(0, 1) < 0.5 ? MAIN : WINDOW;
            Held h = {nullptr, 0, 1u << sid, true};
            CHECK(w.pool.take(n, sid, &h.p, &h.bytes) == DevPool::OK && h.p && h.bytes >= n, "take(%zu)", n);
            if (uni(0, 1) < 0.4) h.used = BOTH;
            live.add(h.p, h.bytes, "take");
            held.push_back(h);
        } else if (held.size() < 48 && r < 0.6) {
            Held h = {nullptr, n, 0, false};
            CHECK(w.pool.alloc_uncached(n, &h.p) == DevPool::OK && h.p, "alloc_uncached(%zu)", n);
            auto f = freed.find(h.p);
            if (f != freed.end()) { /* out of limbo: both streams must have passed what was queued when it went in */
                CHECK(w.A.completed >= f->second.first && w.B.completed >= f->second.second, "block %p left limbo early", h.p);
                freed.erase(f);
            }
            live.add(h.p, n, "alloc_uncached");
            held.push_back(h);
        } else if (!held.empty()) {
            const size_t k = (size_t)uni(0, (double)held.size()) % held.size();
            const Held h = held[k];
            held.erase(held.begin() + (long)k);
            if (h.cached) { live.remove(h.p); w.pool.give(h.p, h.bytes, h.used); }
            else if (foreign && uni(0, 1) < 0.7) foreign->push(h.p, h.bytes);
            else {
                live.remove(h.p);
                if (!foreign) freed[h.p] = {w.A.queued.load(), w.B.queued.load()};
                w.pool.free_uncached(h.p, h.bytes);
            }
        }
        if (uni(0, 1) < 0.6) w.A.work();
        if (uni(0, 1) < 0.6) w.B.work();
        if (uni(0, 1) < 0.3) w.A.finish_to(std::min<uint64_t>(w.A.queued, w.A.completed + (uint64_t)uni(0, 4)));
        if (uni(0, 1) < 0.3) w.B.finish_to(std::min<uint64_t>(w.B.queued, w.B.completed + (uint64_t)uni(0, 4)));
    }
    if (foreign) { foreign->close(); other.join(); }
    for (auto &h : held) { if (h.cached) w.pool.give(h.p, h.bytes, h.used); else w.pool.free_uncached(h.p, h.bytes); }
    CHECK(fake.bad_frees == 0, "%llu hipFree of what is no driver allocation", (unsigned long long)fake.bad_frees);
}

static void case1_no_overlap() { for (unsigned seed = 1; seed <= 3; seed++) random_calls(seed, nullptr); }
static void case7_foreign_thread() { Queue q; random_calls(7, &q); }

/* Case 2: a slab block given back is not handed out while either stream has work in front of the events recorded at the free */
static void case2_limbo()
{
    World w;
    void *p = nullptr, *q = nullptr;
    CHECK(w.pool.alloc_uncached(1000, &p) == DevPool::OK, "first block");
    CHECK(fake.mallocs == 1 && fake.live.begin()->second == GiB, "the first block opens a slab: %llu hipMalloc", (unsigned long long)fake.mallocs);
    w.A.work(); w.B.work();
    w.pool.free_uncached(p, 1000);
    CHECK(w.pool.alloc_uncached(1000, &q) == DevPool::OK && q != p, "both streams busy: the block came back");
    w.pool.free_uncached(q, 1000); /* (behind the same work: in limbo as well) */
    w.A.finish();
    CHECK(w.pool.alloc_uncached(1000, &q) == DevPool::OK && q != p, "the window stream still busy: the block came back");
    w.B.finish();
    void *r = nullptr;
    CHECK(w.pool.alloc_uncached(1000, &r) == DevPool::OK && r == p, "both streams done: an equal request gets %p, not the block %p", r, p);
    CHECK(fake.mallocs == 1 && fake.host_waits == 0 && fake.stream_waits == 0, "no driver call, no wait: %llu hipMalloc, %llu host waits",
          (unsigned long long)fake.mallocs, (unsigned long long)fake.host_waits.load());
    w.pool.free_uncached(q, 1000); w.pool.free_uncached(r, 1000);
}

/* Case 3: a cached block that was used on both streams */
static void case3_cross_stream()
{
    for (int variant = 0; variant < 3; variant++) { /* 0: other stream busy; 1: other stream done; 2: busy, and the driver refuses */
        World w;
        const size_t n = variant == 2 ? 200 * MiB : 5000; /* (2: above the slab limit, so that the request reaches the driver) */
        void *p = nullptr, *q = nullptr;
        size_t np = 0, nq = 0;
        CHECK(w.pool.take(n, MAIN, &p, &np) == DevPool::OK, "first take");
        w.A.work(); w.B.work();
        const uint64_t b_at = w.B.queued;
        w.pool.give(p, np, BOTH);
        w.A.work(); w.B.work();
        if (variant == 1) w.B.finish_to(b_at);
        if (variant == 2) fake.limit = fake.live_bytes;
        const uint64_t frees = fake.frees;
        CHECK(w.pool.take(n, MAIN, &q, &nq) == DevPool::OK, "variant %d: second take", variant);
        if (variant == 0) CHECK(q != p && fake.stream_waits == 0, "busy on WINDOW: the same block (%d) or a wait (%llu)", q == p, (unsigned long long)fake.stream_waits.load());
        /* (as the code stands since the cache was written: the taker's stream is still told to wait for the event that has passed) */
        if (variant == 1) CHECK(q == p && nq == np && fake.stream_waits == 1 && fake.waited_for.at == b_at, "done on WINDOW: another block, or not the one stream-side wait (%llu)", (unsigned long long)fake.stream_waits.load());
        if (variant == 2)
            CHECK(q == p && nq == np && fake.stream_waits == 1 && fake.waited_on == &w.A && fake.waited_for.s == &w.B && fake.waited_for.at == b_at && fake.frees == frees,
                  "driver refuses: same block %d, %llu waits, %llu blocks freed", q == p, (unsigned long long)fake.stream_waits.load(), (unsigned long long)(fake.frees - frees));
        CHECK(fake.host_waits == 0, "variant %d: the host waited", variant);
        w.pool.give(q, nq, 1u << MAIN);
    }
    {   /* one stream and back: WINDOW's cached blocks become MAIN's, and WINDOW's requests are MAIN's */
        World w;
        void *p = nullptr, *q = nullptr;
        size_t np = 0, nq = 0;
        CHECK(w.pool.take(1000, WINDOW, &p, &np) == DevPool::OK, "take");
        w.pool.give(p, np, 1u << WINDOW);
        w.pool.set_window_stream(&w.A);
        CHECK(w.pool.sid(WINDOW) == MAIN && w.pool.take(1000, WINDOW, &q, &nq) == DevPool::OK && q == p, "one stream: WINDOW's block was stranded");
        w.pool.give(q, nq, 1u << MAIN);
    }
}

/* Case 4: a cache bound of 0 -- every give evicts, and the slabs' free list hands the blocks out again */
static void case4_bound()
{
    World w(0);
    std::mt19937_64 rng(3);
    std::vector<uint64_t> counts;
    for (int round = 0; round < 60; round++) {
        const size_t n = 8 * (20000 + rng() % 380000);
        for (int part = 0; part < 3; part++) { /* a sketch: tables on WINDOW, arrays used on both streams, results on MAIN */
            void *p[4]; size_t b[4];
            const size_t want[4] = {n / 8, n * 4, n * 16 / (part + 1), n / 3 + 1};
            const int sid[4] = {WINDOW, WINDOW, MAIN, MAIN};
            const unsigned used[4] = {1u << WINDOW, BOTH, BOTH, 1u << MAIN};
            for (int i = 0; i < 4; i++) CHECK(w.pool.take(want[i], sid[i], &p[i], &b[i]) == DevPool::OK, "take");
            w.A.work(); w.B.work();
            for (int i = 0; i < 4; i++) w.pool.give(p[i], b[i], used[i]);
            if (part == 1) w.B.finish();
        }
        w.finish(); /* (the caller asked for the sketch's records) */
        counts.push_back(fake.mallocs);
    }
    if (getenv("POOL_CHECK_VERBOSE")) for (int r = 0; r < 60; r++) printf("case 4: round %d, %llu driver allocations\n", r, (unsigned long long)counts[r]);
    CHECK(counts[59] <= counts[9] + 1, "%llu driver allocations after ten rounds, %llu after sixty", (unsigned long long)counts[9], (unsigned long long)counts[59]);
    CHECK(fake.host_waits == 0 && fake.frees == 0, "an eviction waited (%llu) or went to the driver (%llu)", (unsigned long long)fake.host_waits.load(), (unsigned long long)fake.frees);
}

/* Case 5: the driver refuses -- the cache is dropped, slabs without a live block go back, the request is made once more */
static void case5_out_of_memory()
{
    World w;
    void *x[8], *tail = nullptr, *big = nullptr, *c = nullptr;
    size_t nc = 0;
    for (int i = 0; i < 6; i++) CHECK(w.pool.alloc_uncached(150 * MiB, &x[i]) == DevPool::OK, "slab 1, block %d", i);
    const uintptr_t slab1 = fake.live.begin()->first;
    CHECK(fake.mallocs == 1 && (uintptr_t)x[5] == slab1 + 750 * MiB, "six blocks of 150 MiB in one slab");
    CHECK(w.pool.alloc_uncached(150 * MiB, &x[6]) == DevPool::OK && fake.mallocs == 2, "the seventh opens slab 2");
    const uintptr_t slab2 = std::prev(fake.live.end())->first;
    /* the 124 MiB behind block six are not lost with the bump pointer: the next request that fits gets them */
    CHECK(w.pool.alloc_uncached(100 * MiB, &tail) == DevPool::OK && (uintptr_t)tail == slab1 + 900 * MiB && fake.mallocs == 2, "the tail of slab 1: %#zx", (size_t)tail);
    CHECK(w.pool.take(300 * MiB, MAIN, &c, &nc) == DevPool::OK && nc == 304 * MiB && fake.mallocs == 3, "a cached single block: %zu bytes", nc);
    w.pool.give(c, nc, 1u << MAIN);
    w.B.work();
    w.pool.free_uncached(x[6], 150 * MiB); /* slab 2 holds no live block now; the block is in limbo behind WINDOW's work */
    fake.limit = 2 * GiB + 700 * MiB;
    CHECK(w.pool.alloc_uncached(600 * MiB, &big) == DevPool::OK, "600 MiB after the cache (304 MiB) and slab 2 (1 GiB) went back");
    CHECK(fake.refused == 1 && fake.frees == 2 && fake.live.count(slab1) && !fake.live.count(slab2) && !fake.live.count((uintptr_t)c),
          "%llu refusals, %llu hipFree, slab 1 live %zu, slab 2 live %zu", (unsigned long long)fake.refused, (unsigned long long)fake.frees, fake.live.count(slab1), fake.live.count(slab2));
    CHECK(w.B.completed == w.B.queued, "the limbo of a slab that may go is waited for when memory has run out");
    void *none = (void *)1;
    CHECK(w.pool.alloc_uncached(2 * GiB, &none) == DevPool::NOMEM && fake.refused == 3 && fake.frees == 2, "2 GiB more: nothing left to drop, %llu refusals", (unsigned long long)fake.refused);
    void *y = nullptr; /* slab 1 still serves: the blocks it gets back, and no driver call */
    w.pool.free_uncached(x[0], 150 * MiB);
    CHECK(w.pool.alloc_uncached(150 * MiB, &y) == DevPool::OK && y == x[0] && fake.mallocs == 4, "slab 1 after the trim");
    x[0] = y;
    for (int i = 0; i < 6; i++) w.pool.free_uncached(x[i], 150 * MiB);
    w.pool.free_uncached(tail, 100 * MiB);
    w.pool.free_uncached(big, 600 * MiB);
}

/* Case 6: destroy() with blocks in limbo and in both caches -- every driver allocation is freed exactly once (World's destructor checks) */
static void case6_destroy()
{
    World w;
    void *p[4]; size_t b[4];
    for (int i = 0; i < 4; i++) CHECK(w.pool.take(i < 2 ? 4096 : 250 * MiB, i & 1, &p[i], &b[i]) == DevPool::OK, "take %d", i);
    void *u[3];
    for (int i = 0; i < 3; i++) CHECK(w.pool.alloc_uncached(i < 2 ? 70000 : 200 * MiB, &u[i]) == DevPool::OK, "alloc_uncached %d", i);
    w.A.work(); w.B.work();
    w.pool.give(p[0], b[0], 1u << MAIN); w.pool.give(p[1], b[1], BOTH); w.pool.give(p[2], b[2], BOTH); w.pool.give(p[3], b[3], 1u << WINDOW);
    for (int i = 0; i < 3; i++) w.pool.free_uncached(u[i], i < 2 ? 70000 : 200 * MiB);
    CHECK(fake.mallocs == 4 && fake.frees == 1 && fake.events == 2 + 2 + 2 * 2, "%llu hipMalloc, %llu hipFree, %lld events before destroy",
          (unsigned long long)fake.mallocs, (unsigned long long)fake.frees, (long long)fake.events);
}

int main()
{
    case1_no_overlap();
    case2_limbo();
    case3_cross_stream();
    case4_bound();
    case5_out_of_memory();
    case6_destroy();
    case7_foreign_thread();
    if (g_failed) printf("%d checks failed\n", g_failed);
    else printf("pool_check: ok\n");
    return g_failed ? 1 : 0;
}
