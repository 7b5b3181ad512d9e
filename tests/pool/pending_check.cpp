/*
 * Host test of the lazy-completion types (ntlink_amd/csrc/pending.h) over the scripted runtime beside this file (hip/hip_runtime.h):
 * one stream advanced by hand, slots that are a plain array, holds that are counters.  One line per failed check, exit status 1 on any.
 * Built and run by tests/test_pending.py (g++ -std=c++17 -I tests/pool, once with -fsanitize=address,undefined, once with =thread).
 */
#include "../../ntlink_amd/csrc/pending.h"

#include <stdio.h>

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

/* what a hold keeps alive: taken once by the test, released through the hold */
struct Res { int refs = 0, released = 0; };
static std::vector<const Res *> g_release_order;
static void *g_released_by = nullptr;
static void let_go(const void *p, void *by)
{
    Res *r = (Res *)p;
    r->refs--; r->released++;
    g_release_order.push_back(r);
    g_released_by = by;
}

/* the check of the test: word 2 of the slot is the failure flag, words 0 / 1 the hit count and the minimizer count; arg picks the message */
static const char *const MSG[3] = {"orphan 0 failed", "orphan 1 failed", "orphan 2 failed"};
static std::vector<uint64_t> g_checked;
static const char *check(const PinSlot &s, uint64_t arg, std::atomic<float> *hitf)
{
    g_checked.push_back(arg);
    if (hitf && s.w[1]) hitf->store((float)((double)s.w[0] / (double)s.w[1]));
    return s.w[2] ? MSG[arg] : nullptr;
}

/* a fresh runtime, one stream and a queue of n slots; the queue is destroyed with it: no event and no hold may be left */
struct World {
    fake_stream A;
    PinSlot host[4], dev[4], dsums[4];
    Res res[6];
    PendingQueue q;
    explicit World(uint32_t n)
    {
        fake.events = 0; fake.host_waits = 0;
        g_release_order.clear(); g_checked.clear(); g_released_by = nullptr;
        memset(host, 0xAB, sizeof host);
        q.setup(host, dev, dsums, n, this);
    }
    /* an armed handle with two holds whose work is the stream's next */
    Pending queued(int i, bool pending = true)
    {
        Pending p;
        res[2 * i].refs++; res[2 * i + 1].refs++;
        p.holds[0] = {&res[2 * i], let_go};
        p.holds[1] = {&res[2 * i + 1], let_go};
        CHECK(p.arm(q), "arm %d", i);
        A.work();
        hipEventRecord(p.done, &A);
        p.pending = pending;
        return p;
    }
    int held() const { int n = 0; for (const Res &r : res) n += r.refs; return n; }
    ~World()
    {
        q.destroy();
        CHECK(fake.events == 0 && held() == 0, "after destroy: %lld events, %d holds", (long long)fake.events, held());
        for (const Res &r : res) CHECK(r.released <= 1, "a hold was released %d times", r.released);
    }
};

static bool zero(const PinSlot *p) { for (uint64_t w : p->w) if (w) return false; return true; }

/* arm, then settle: event and slot are back, every hold is released exactly once; a second settle does nothing */
static void case1_arm_settle()
{
    World w(4);
    Pending p = w.queued(0);
    PinSlot *const slot = p.slot;
    const hipEvent_t ev = p.done;
    CHECK(slot >= w.host && slot < w.host + 4 && zero(slot) && fake.events == 1, "a zeroed slot of the array and one new event");
    CHECK(w.q.slot_dev(slot) == w.dev + (slot - w.host) && w.q.slot_dsums(slot) == w.dsums + (slot - w.host), "the slot's other views");
    CHECK(p.wait() == hipSuccess && fake.host_waits == 1 && w.A.completed == 1, "wait: %llu host waits", (unsigned long long)fake.host_waits.load());
    CHECK(p.wait() == hipSuccess && fake.host_waits == 1, "the event has passed: wait does not block");
    p.pending = false;
    p.settle(w.q);
    CHECK(!p.done && !p.slot && !p.holds[0].p && !p.holds[1].p, "settle nulls what it hands back");
    CHECK(w.res[0].released == 1 && w.res[1].released == 1 && w.held() == 0 && g_released_by == &w, "each hold once, by the queue's owner");
    p.settle(w.q);
    CHECK(w.res[0].released == 1 && w.res[1].released == 1 && g_release_order.size() == 2, "a second settle released again");
    Pending r;
    CHECK(r.arm(w.q) && r.done == ev && r.slot == slot && fake.events == 1, "the next handle gets the event and the slot that went back");
    r.settle(w.q);
}

/* orphans: nothing is released before the event has passed; then in queue order, each checked once, the first failure kept */
static void case2_orphans()
{
    World w(4);
    auto hitf = std::make_shared<std::atomic<float>>(0.0f);
    Pending p[3] = {w.queued(0), w.queued(1), w.queued(2)};
    p[0].slot->w[0] = 3; p[0].slot->w[1] = 4;                     /* passes, three hits in four minimizers */
    p[1].slot->w[2] = 1;                                          /* fails */
    p[2].slot->w[0] = 1; p[2].slot->w[1] = 8; p[2].slot->w[2] = 1; /* fails too */
    for (int i = 0; i < 3; i++) {
        p[i].orphan(w.q, check, (uint64_t)i, i == 1 ? nullptr : hitf);
        CHECK(!p[i].done && !p[i].slot && !p[i].pending && !p[i].holds[0].p, "the handle keeps nothing of what the queue took over");
    }
    w.q.reap(false);
    CHECK(w.held() == 6 && g_checked.empty() && fake.host_waits == 0 && w.q.async_err.empty(), "the stream has not run: %d holds left, %zu checks", w.held(), g_checked.size());
    w.A.finish_to(2);
    w.q.reap(false);
    CHECK(g_release_order == (std::vector<const Res *>{&w.res[0], &w.res[1], &w.res[2], &w.res[3]}), "orphans 0 and 1, in that order: %zu releases", g_release_order.size());
    CHECK(g_checked == (std::vector<uint64_t>{0, 1}), "one check each: %zu", g_checked.size());
    CHECK(hitf->load() == 0.75f && w.q.async_err == MSG[1], "hit fraction %g, message '%s'", (double)hitf->load(), w.q.async_err.c_str());
    w.A.finish();
    w.q.reap(false);
    /* (as found: once a failure is kept, a later orphan is settled unchecked -- its message would be dropped anyway) */
    CHECK(w.held() == 0 && w.q.async_err == MSG[1] && hitf->load() == 0.75f && g_checked.size() == 2, "the first message stays: '%s'", w.q.async_err.c_str());
    CHECK(fake.host_waits == 0, "a non-blocking reap waited");
}

/* two slots, two orphans: the third slot_get waits for the oldest only; then nothing is free and nothing is owed */
static void case3_out_of_slots()
{
    World w(2);
    Pending a = w.queued(0), b = w.queued(1);
    PinSlot *const sa = a.slot, *const sb = b.slot;
    sa->w[0] = 7; sa->w[5] = ~0ull;
    a.orphan(w.q, check, 0);
    b.orphan(w.q, check, 1);
    PinSlot *s = w.q.slot_get();
    CHECK(s == sa && zero(s), "the oldest orphan's slot, zeroed");
    CHECK(fake.host_waits == 1 && w.A.completed == 1, "one host wait, for the oldest: %llu waits, stream at %llu", (unsigned long long)fake.host_waits.load(), (unsigned long long)w.A.completed.load());
    CHECK(w.res[0].released == 1 && w.res[1].released == 1 && !w.res[2].released && !w.res[3].released && g_checked.size() == 1, "the younger orphan is still queued");
    PinSlot *t = w.q.slot_get();
    CHECK(t == sb && fake.host_waits == 2 && w.held() == 0, "the second wait frees the younger one");
    /* nothing free, no orphan: no slot, and arm reports it without keeping the event it took */
    const long long events = fake.events;
    CHECK(!w.q.slot_get() && fake.host_waits == 2, "a slot out of nowhere, or a wait for nobody");
    Pending c;
    c.holds[0] = {&w.res[4], let_go}; w.res[4].refs++;
    CHECK(!c.arm(w.q) && !c.done && !c.slot, "arm without a slot");
    const hipEvent_t e = w.q.event_get();
    CHECK(e && fake.events == events, "the event arm took is back on the free list: %lld events, %lld before", (long long)fake.events, events);
    w.q.event_put(e);
    CHECK(w.res[4].refs == 1, "arm let go of a hold: that is the caller's orphan / settle");
    c.orphan(w.q, check, 2);
    w.q.slot_put(s); w.q.slot_put(t);
}

/* the error paths: a handle whose work never was pending (or was drained) is settled at once, nothing is queued */
static void case4_orphan_not_pending()
{
    World w(2);
    Pending p = w.queued(0, false);
    PinSlot *const slot = p.slot;
    slot->w[2] = 1;
    p.orphan(w.q, check, 0);
    CHECK(w.held() == 0 && w.res[0].released == 1 && w.res[1].released == 1 && !p.done && !p.slot, "released at once");
    w.A.finish();
    w.q.reap(true);
    CHECK(g_checked.empty() && w.q.async_err.empty() && fake.host_waits == 0 && g_release_order.size() == 2, "something was queued");
    PinSlot *s = w.q.slot_get();
    CHECK(s == slot && zero(s), "the slot is free again");
    w.q.slot_put(s);
}

/* destroy with orphans whose work has not run and events on the free list (World's destructor checks) */
static void case5_destroy()
{
    World w(4);
    Pending a = w.queued(0), b = w.queued(1), c = w.queued(2);
    a.orphan(w.q, check, 0);
    b.orphan(w.q, check, 1);
    c.pending = false;
    c.settle(w.q);
    w.q.event_put(w.q.event_get());
    CHECK(fake.events == 3 && w.held() == 4, "%lld events, %d holds before destroy", (long long)fake.events, w.held());
}

int main()
{
    case1_arm_settle();
    case2_orphans();
    case3_out_of_slots();
    case4_orphan_not_pending();
    case5_destroy();
    if (g_failed) printf("%d checks failed\n", g_failed);
    else printf("pending_check: ok\n");
    return g_failed ? 1 : 0;
}
