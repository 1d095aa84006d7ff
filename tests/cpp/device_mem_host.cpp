// The owners of csrc/device_mem.h against a counting stand-in for the runtime (tests/cpp/hip_stub): creates and releases balance through
// scopes, moves and regrows; the grow-only step; a create function's partial failures, every one; a seeded random walk.  Built with
// -fsanitize=address,undefined (leak detection on) and run directly: tests/test_device_mem_host.py.
//   device_mem_host [steps] [seed]  ->  one JSON line {"checks", "failed_checks", "steps", ...}, exit status 1 on a failed check
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "device_mem.h"

static std::string g_error;
void dabgpu_set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
}
int dabgpu_check_hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return 0;
    dabgpu_set_error("%s: error %d", what, (int)e);
    return 3;      // DABGPU_ERR_HIP
}

using namespace dabgpu;
using hip_stub::state;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond) do { g_checks++; if (!(cond)) { g_failed++; if (g_failed < 20) fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); } } while (0)

static long made_total() { long n = 0; for (long v : state().made) n += v; return n; }
static long released_total() { long n = 0; for (long v : state().released) n += v; return n; }
static bool balanced() { return state().live.empty() && made_total() == released_total(); }

// ---- scopes and moves, every owner kind ----
template <class Owner, class Make>
static void balance_of(hip_stub::Kind k, Make make) {
    const long made0 = state().made[k], rel0 = state().released[k];
    {
        Owner a;
        CHECK(!a && a.get() == nullptr);
        { Owner unused; }                                          // empty owners release nothing
        CHECK(state().released[k] == rel0);
        CHECK(make(a) == 0 && a && a.get() != nullptr);
        auto raw = a.get();
        Owner b(std::move(a));                                     // move construction: the source is empty
        CHECK(!a && a.get() == nullptr && b.get() == raw);
        Owner c;
        CHECK(make(c) == 0);
        c = std::move(b);                                          // move assignment releases what the target held
        CHECK(state().released[k] == rel0 + 1 && c.get() == raw && !b);
        Owner& self = c;
        c = std::move(self);                                       // self-move: nothing happens
        CHECK(c.get() == raw && state().released[k] == rel0 + 1);
        c.reset();
        CHECK(!c && state().released[k] == rel0 + 2);
        c.reset();                                                 // twice is once
        CHECK(state().released[k] == rel0 + 2);
        CHECK(make(c) == 0);
        CHECK(make(c) == 0);                                       // making again releases the first
        CHECK(state().released[k] == rel0 + 3);
    }
    CHECK(state().made[k] == made0 + 4 && state().released[k] == rel0 + 4);
    CHECK(balanced());
}

// ---- needs / regrow ----
template <class Buf>
static void grow_only(hip_stub::Kind k) {
    Buf b;
    CHECK(b.capacity() == 0 && !b.needs(0) && b.needs(1));
    long calls = state().calls;
    CHECK(b.regrow(0, "none") == 0 && state().calls == calls && !b);    // nothing asked, nothing done
    CHECK(b.regrow(100, "first") == 0 && b.capacity() == 100 && b.get());
    auto first = b.get();
    calls = state().calls;
    for (size_t n : {size_t(100), size_t(99), size_t(1), size_t(0)}) {  // at or below capacity: no runtime call, the same block, capacity never shrinks
        CHECK(!b.needs(n) && b.regrow(n, "same") == 0);
        CHECK(state().calls == calls && b.get() == first && b.capacity() == 100);
    }
    const long rel = state().released[k];
    CHECK(b.needs(101) && b.regrow(101, "second") == 0 && b.capacity() == 101 && state().released[k] == rel + 1);
    CHECK(state().release_log.back() == first);
    // a failed regrow: empty, capacity 0, exactly one release (the old block); a later one succeeds
    auto second = b.get();
    state().fail_at = 1; state().allocations = 0;
    g_error.clear();
    CHECK(b.regrow(500, "hipMalloc(the label)") == 3);
    state().fail_at = 0;
    CHECK(g_error.rfind("hipMalloc(the label): ", 0) == 0);
    CHECK(b.get() == nullptr && !b && b.capacity() == 0 && b.needs(1));
    CHECK(state().released[k] == rel + 2 && state().release_log.back() == second);
    CHECK(b.regrow(500, "third") == 0 && b.capacity() == 500 && b.get());
}

// ---- a create function: six owners in sequence, allocation k fails ----
struct Six {
    DeviceBuffer<float> d_a;
    DeviceBuffer<> d_b;
    PinnedBuffer<uint8_t> h_c;
    Event ev;
    Stream s;
    PinnedBuffer<float> h_d;
};
static const char* const SIX_LABELS[6] = {"hipMalloc(six a)", "hipMalloc(six b)", "hipHostMalloc(six c)", "hipEventCreate(six)", "hipStreamCreate(six)", "hipHostMalloc(six d)"};
static int six_create(Six** out) {
    *out = nullptr;
    Six* x = new (std::nothrow) Six();
    if (!x) return 3;
    int st = x->d_a.alloc(1000, SIX_LABELS[0]);
    if (!st) st = x->d_b.alloc(64, SIX_LABELS[1]);
    if (!st) st = x->h_c.alloc(4096, SIX_LABELS[2]);
    if (!st) st = x->ev.create(hipEventDisableTiming, SIX_LABELS[3]);
    if (!st) st = x->s.create(hipStreamNonBlocking, 0, SIX_LABELS[4]);
    if (!st) st = x->h_d.alloc(7, SIX_LABELS[5]);
    if (st) { delete x; return st; }
    *out = x;
    return 0;
}
static void partial_failures() {
    for (int k = 1; k <= 7; k++) {                                 // 7: nothing fails
        const long made0 = made_total(), rel0 = released_total();
        state().fail_at = k; state().allocations = 0;
        g_error.clear();
        Six* x = reinterpret_cast<Six*>(0x10);
        const int st = six_create(&x);
        state().fail_at = 0;
        if (k <= 6) {
            CHECK(st == 3 && x == nullptr);
            CHECK(g_error.rfind(std::string(SIX_LABELS[k - 1]) + ": ", 0) == 0);
            CHECK(made_total() - made0 == k - 1 && released_total() - rel0 == k - 1);
        } else {
            CHECK(st == 0 && x != nullptr && made_total() - made0 == 6 && released_total() == rel0);
            CHECK(x->d_a.capacity() == 1000 && x->d_b.capacity() == 64 && x->h_d.capacity() == 7);
            delete x;
            CHECK(released_total() - rel0 == 6);
        }
        CHECK(balanced());
    }
}

// ---- a seeded random walk over a few owners of every kind ----
static void random_walk(long steps, uint64_t seed) {
    std::mt19937_64 rng(seed);
    {
        std::vector<DeviceBuffer<int>> dev(5);
        std::vector<PinnedBuffer<>> pin(5);
        std::vector<Event> ev(3);
        std::vector<Stream> str(3);
        for (long i = 0; i < steps; i++) {
            const unsigned op = (unsigned)(rng() % 8), a = (unsigned)(rng() % 5), b = (unsigned)(rng() % 5);
            const size_t n = (size_t)(rng() % 300);
            const bool fail = rng() % 16 == 0;
            if (fail) { state().fail_at = 1; state().allocations = 0; }
            switch (op) {
            case 0: { const int st = dev[a].alloc(n, "walk"); CHECK(st ? !dev[a] && dev[a].capacity() == 0 : dev[a].capacity() == n && dev[a].get()); break; }
            case 1: { const size_t cap = dev[a].capacity(); const int st = dev[a].regrow(n, "walk");
                      CHECK(st ? !dev[a] && dev[a].capacity() == 0 : dev[a].capacity() == (n > cap ? n : cap)); break; }
            case 2: { const size_t cap = pin[a].capacity(); const int st = pin[a].regrow(n, "walk");
                      CHECK(st ? !pin[a] && pin[a].capacity() == 0 : pin[a].capacity() == (n > cap ? n : cap)); break; }
            case 3: dev[a] = std::move(dev[b]); if (a != b) CHECK(!dev[b] && dev[b].capacity() == 0); break;
            case 4: pin[a] = std::move(pin[b]); if (a != b) CHECK(!pin[b]); break;
            case 5: if (rng() & 1) dev[a].reset(); else pin[a].reset(); break;
            case 6: {
                Event& e = ev[a % 3];
                const int st = e.create(hipEventDisableTiming, "walk");
                CHECK(st ? !e : (bool)e);
                if (rng() & 1) ev[b % 3] = std::move(e);
                break;
            }
            case 7: {
                Stream& s = str[a % 3];
                const int st = (rng() & 1) ? s.create(hipStreamNonBlocking, "walk") : s.create(hipStreamNonBlocking, -1, "walk");
                CHECK(st ? !s : (bool)s);
                if (rng() & 1) { Stream t(std::move(s)); CHECK(!s); }
                break;
            }
            }
            state().fail_at = 0;
            // what the owners hold is exactly what is live
            size_t held = 0;
            for (auto& o : dev) held += o ? 1 : 0;
            for (auto& o : pin) held += o ? 1 : 0;
            for (auto& o : ev) held += o ? 1 : 0;
            for (auto& o : str) held += o ? 1 : 0;
            CHECK(held == state().live.size());
            if (i % 512 == 0) { dev.emplace_back(); dev.erase(dev.begin()); }      // the vector moves its owners about
        }
    }
    CHECK(balanced());
}

int main(int argc, char** argv) {
    const long steps = argc > 1 ? atol(argv[1]) : 4000;
    const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    balance_of<DeviceBuffer<float>>(hip_stub::DEVICE, [](DeviceBuffer<float>& o) { return o.alloc(10, "t"); });
    balance_of<DeviceBuffer<>>(hip_stub::DEVICE, [](DeviceBuffer<>& o) { return o.alloc(10, "t"); });
    balance_of<PinnedBuffer<uint8_t>>(hip_stub::PINNED, [](PinnedBuffer<uint8_t>& o) { return o.alloc(10, "t"); });
    balance_of<Event>(hip_stub::EVENT, [](Event& o) { return o.create(hipEventDisableTiming, "t"); });
    balance_of<Stream>(hip_stub::STREAM, [](Stream& o) { return o.create(hipStreamNonBlocking, "t"); });
    balance_of<Stream>(hip_stub::STREAM, [](Stream& o) { return o.create(hipStreamNonBlocking, -1, "t"); });
    grow_only<DeviceBuffer<>>(hip_stub::DEVICE);
    grow_only<PinnedBuffer<uint16_t>>(hip_stub::PINNED);
    CHECK(balanced());
    partial_failures();
    random_walk(steps, seed);
    printf("{\"checks\": %ld, \"failed_checks\": %ld, \"steps\": %ld, \"made\": %ld, \"released\": %ld}\n", g_checks, g_failed, steps,
           made_total(), released_total());
    return g_failed == 0 && balanced() ? 0 : 1;
}
