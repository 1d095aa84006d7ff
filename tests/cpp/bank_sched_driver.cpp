// bank_sched_driver.cpp -- the receiver bank's scheduler (dab-radio_amd/csrc/receiver_bank_sched.cpp) driven through the C entry points of
// include/dabgpu.h, without the classes, for sanitizer runs on a machine without a GPU: linked against tests/cpp/fake_dabgpu_oracle.cpp, whose
// banked receivers are members of a bank that the product's scheduler runs over the CPU oracle (tests/test_host_sanitizers.py).
//   bank_sched_driver backlog   a member posts as many frames as post_frame accepts with no synchroniser in between, and one more
//   bank_sched_driver churn     8 threads join, run two frames and leave, 20 times each
//   bank_sched_driver failed_round         a round with a frame of each of two members fails, then one with a synchroniser, then a wait for the device: only
//                                          those generations / that record answer the status, everything later is a private receiver's again, without a reset
//   bank_sched_driver late_destroy         two banked receivers are destroyed AFTER dabgpu_rx_bank_shutdown()
//   bank_sched_driver shutdown_with_queue  shutdown arrives while a round is held and two more jobs are queued behind it: every wait of the poster returns
// Expected bits are those of a private receiver of the same executable fed the same samples.  Prints one JSON line; exit status 0 only when all holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <thread>
#include <vector>

#include "dabgpu.h"
#include "receiver_bank_sched.h"

extern "C" void fake_dabgpu_bank_hold(int on);
extern "C" void fake_dabgpu_bank_fail_rounds(int n, int status);
extern "C" void fake_dabgpu_bank_fail_waits(int n, int status);
extern "C" int fake_dabgpu_bank_enqueues(void);

namespace {
const dabgpu_sync_cfg CFG = [] { dabgpu_sync_cfg c{}; c.fine_freq_update_beta = 0.9f; c.is_coarse_freq_correction = 1; c.max_coarse_freq_correction_norm = 0.5f;
                                 c.coarse_freq_slow_beta = 0.1f; c.impulse_peak_threshold_db = 20.0f; c.impulse_peak_distance_probability = 0.15f; return c; }();
constexpr size_t PRS_AT = 100, FRAME_AT = 40;            // where the synchroniser and the frame are cut in the staging buffer
#define CK(call) do { const int st_ = (call); if (st_) { std::fprintf(stderr, "%s -> %d (%s)\n", #call, st_, dabgpu_last_error()); std::exit(1); } } while (0)

// pseudo-noise samples, a different sequence per seed: the demodulator turns any samples into soft bits that depend on every one of them
void fill(dabgpu_receiver* rx, uint32_t seed) {
    float* h = nullptr; size_t cap = 0;
    CK(dabgpu_receiver_stage(rx, &h, &cap));
    uint32_t x = seed * 2654435761u + 12345u;
    for (size_t k = 0; k < 2 * cap; k++) { x = x * 1664525u + 1013904223u; h[k] = (float)(int32_t)x * (1.0f / 2147483648.0f); }
}
uint64_t fnv(const int8_t* b, size_t n) { uint64_t h = 0xCBF29CE484222325ull; for (size_t k = 0; k < n; k++) { h ^= (uint8_t)b[k]; h *= 0x100000001B3ull; } return h; }
uint64_t collect(dabgpu_receiver* rx, uint64_t gen) {
    dabgpu_receiver_frame f{};
    CK(dabgpu_receiver_wait_frame(rx, gen, &f));
    return f.generation == gen && f.n_bits == DABGPU_NB_FRAME_BITS ? fnv(f.bits, f.n_bits) : 0;
}
void sync(dabgpu_receiver* rx, uint32_t seed) {
    dabgpu_sync_state rec;
    fill(rx, seed);
    CK(dabgpu_receiver_submit_sync(rx, &CFG, PRS_AT));
    CK(dabgpu_receiver_wait_sync(rx, &rec, nullptr, nullptr));
}
// one synchroniser, then n frames posted back to back (seed + 1 ...); `hold`: no round completes before all are posted.  Returns the status of the post after them.
int run(dabgpu_receiver* rx, uint32_t seed, int n, bool hold, std::vector<uint64_t>& digests) {
    sync(rx, seed);
    if (hold) fake_dabgpu_bank_hold(1);
    std::vector<uint64_t> gens((size_t)n);
    for (int k = 0; k < n; k++) { fill(rx, seed + 1 + (uint32_t)k); CK(dabgpu_receiver_submit_frame(rx, FRAME_AT, CFG.fine_freq_update_beta, 0, 0, &gens[(size_t)k])); }
    int extra = DABGPU_OK;
    if (hold) { fill(rx, seed + 99); uint64_t g = 0; extra = dabgpu_receiver_submit_frame(rx, FRAME_AT, CFG.fine_freq_update_beta, 0, 0, &g); fake_dabgpu_bank_hold(0); }
    for (int k = 0; k < n; k++) digests.push_back(gens[(size_t)k] == (uint64_t)k ? collect(rx, gens[(size_t)k]) : 0);
    return extra;
}

int backlog() {
    const int n = RX_BANK_SLOTS - 1;                     // what post_frame accepts with nothing collected: next_gen < done_gen + R - 1
    dabgpu_receiver *priv = nullptr, *banked = nullptr;
    CK(dabgpu_receiver_create(&priv, 0, 1, nullptr, nullptr));
    CK(dabgpu_receiver_create_banked(&banked, 0));
    std::vector<uint64_t> want, got;
    run(priv, 7, n, false, want);
    const int extra = run(banked, 7, n, true, got);
    dabgpu_receiver_destroy(banked);
    dabgpu_receiver_destroy(priv);
    bool distinct = true;
    for (int a = 0; a < n; a++) for (int b = a + 1; b < n; b++) distinct = distinct && want[(size_t)a] != want[(size_t)b];
    const bool ok = extra == DABGPU_ERR_NOT_READY && got == want && distinct && want[0] != 0;
    std::printf("{\"accepted\": %d, \"one_more\": %d, \"in_order_with_own_bits\": %s, \"frames_distinct\": %s, \"ok\": %s}\n", n, extra, got == want ? "true" : "false",
                distinct ? "true" : "false", ok ? "true" : "false");
    return ok ? 0 : 1;
}

int churn() {
    constexpr int THREADS = 8, ROUNDS = 20;
    auto two_frames = [](dabgpu_receiver* rx, uint32_t seed, std::vector<uint64_t>& d) {
        run(rx, seed, 1, false, d);
        sync(rx, seed + 50);
        run(rx, seed + 60, 0, false, d);                 // (a second synchroniser with nothing behind it: its record is dropped by the next one's)
        fill(rx, seed + 51);
        uint64_t g = 0;
        CK(dabgpu_receiver_submit_frame(rx, FRAME_AT, CFG.fine_freq_update_beta, 0, 0, &g));
        d.push_back(collect(rx, g));
    };
    // what every thread's frames must come to, from private receivers, before the threads start (the oracle builds its tables at first use, on one thread)
    std::vector<uint64_t> want[THREADS];
    for (int t = 0; t < THREADS; t++) {
        dabgpu_receiver* priv = nullptr;
        CK(dabgpu_receiver_create(&priv, 0, 1, nullptr, nullptr));
        two_frames(priv, 1000u * (uint32_t)(t + 1), want[t]);
        dabgpu_receiver_destroy(priv);
    }
    int bad[THREADS] = {0};
    std::vector<std::thread> th;
    for (int t = 0; t < THREADS; t++) th.emplace_back([t, &bad, &want, &two_frames] {
        for (int k = 0; k < ROUNDS; k++) {
            dabgpu_receiver* rx = nullptr;
            CK(dabgpu_receiver_create_banked(&rx, 0));
            std::vector<uint64_t> got;
            two_frames(rx, 1000u * (uint32_t)(t + 1), got);
            if (got != want[t] || got.size() != 2 || got[0] == 0) bad[t]++;
            dabgpu_receiver_destroy(rx);
        }
    });
    for (auto& t : th) t.join();
    int wrong = 0, members = -2, refs = -2;
    for (int b : bad) wrong += b;
    dabgpu_rx_bank_census(0, &members, &refs);
    const bool ok = wrong == 0 && members == 0 && refs == 0;
    std::printf("{\"threads\": %d, \"joins\": %d, \"wrong_results\": %d, \"members_left\": %d, \"refs\": %d, \"ok\": %s}\n", THREADS, THREADS * ROUNDS, wrong, members, refs, ok ? "true" : "false");
    return ok ? 0 : 1;
}

// ---- failed_round ----
constexpr int INJECTED = DABGPU_ERR_HIP;
uint64_t post(dabgpu_receiver* rx, uint32_t seed) {
    fill(rx, seed);
    uint64_t g = ~0ull;
    CK(dabgpu_receiver_submit_frame(rx, FRAME_AT, CFG.fine_freq_update_beta, 0, 0, &g));
    return g;
}
// the status of wait_frame and, when it is DABGPU_OK, the digest
int collect_st(dabgpu_receiver* rx, uint64_t gen, uint64_t* digest) {
    dabgpu_receiver_frame f{};
    const int st = dabgpu_receiver_wait_frame(rx, gen, &f);
    *digest = !st && f.generation == gen && f.n_bits == DABGPU_NB_FRAME_BITS ? fnv(f.bits, f.n_bits) : 0;
    return st;
}
void until_enqueues(int n) { while (fake_dabgpu_bank_enqueues() < n) std::this_thread::sleep_for(std::chrono::milliseconds(1)); }

// The calls of one member of failed_round, in its own order: sync, frame 0 | sync, frames 1, 2 back to back | sync, frame 3 | sync (fails in the bank), sync,
// frame 4 | sync, frame 5 (its wait fails in the bank), sync, frame 6.  Here on a private receiver: the digests the bank's member must deliver.
void failed_round_private(uint32_t seed, uint64_t want[7]) {
    dabgpu_receiver* rx = nullptr;
    CK(dabgpu_receiver_create(&rx, 0, 1, nullptr, nullptr));
    sync(rx, seed); want[0] = collect(rx, post(rx, seed + 1));
    sync(rx, seed + 10);
    const uint64_t g1 = post(rx, seed + 11), g2 = post(rx, seed + 12);
    want[1] = collect(rx, g1); want[2] = collect(rx, g2);
    sync(rx, seed + 20); want[3] = collect(rx, post(rx, seed + 21));
    sync(rx, seed + 30); sync(rx, seed + 31); want[4] = collect(rx, post(rx, seed + 32));
    sync(rx, seed + 40); want[5] = collect(rx, post(rx, seed + 41));
    sync(rx, seed + 50); want[6] = collect(rx, post(rx, seed + 51));
    dabgpu_receiver_destroy(rx);
}

int failed_round() {
    const uint32_t seed[2] = {100, 200};
    uint64_t want[2][7], got[2][7] = {{0}};
    int st[2][7] = {{0}};
    for (int k = 0; k < 2; k++) failed_round_private(seed[k], want[k]);
    dabgpu_receiver* rx[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; k++) CK(dabgpu_receiver_create_banked(&rx[k], 0));
    for (int k = 0; k < 2; k++) { sync(rx[k], seed[k]); st[k][0] = collect_st(rx[k], post(rx[k], seed[k] + 1), &got[k][0]); }
    for (int k = 0; k < 2; k++) sync(rx[k], seed[k] + 10);
    // A round held with frame 1 of member 0 alone; behind it the queue [1.f1, 0.f2, 1.f2]: the next round takes one frame of each member (1.f1, 0.f2) and is
    // the one that fails -- ordered after the held round has entered enqueue --, the third carries 1.f2
    const int e0 = fake_dabgpu_bank_enqueues();
    fake_dabgpu_bank_hold(1);
    uint64_t g[2][3];
    g[0][1] = post(rx[0], seed[0] + 11);
    until_enqueues(e0 + 1);
    g[1][1] = post(rx[1], seed[1] + 11);
    g[0][2] = post(rx[0], seed[0] + 12);
    g[1][2] = post(rx[1], seed[1] + 12);
    fake_dabgpu_bank_fail_rounds(1, INJECTED);
    fake_dabgpu_bank_hold(0);
    // (collected newest first: the failed generations' status must not show under an earlier or a later one, whichever is asked for first)
    for (int k = 0; k < 2; k++) for (int f = 2; f >= 1; f--) st[k][f] = g[k][f] == (uint64_t)f ? collect_st(rx[k], g[k][f], &got[k][f]) : -1;
    const bool frames_ok = st[0][1] == DABGPU_OK && st[0][2] == INJECTED && st[1][1] == INJECTED && st[1][2] == DABGPU_OK;
    // later frames of both, no reset in between
    for (int k = 0; k < 2; k++) { sync(rx[k], seed[k] + 20); st[k][3] = collect_st(rx[k], post(rx[k], seed[k] + 21), &got[k][3]); }
    // a round with a synchroniser fails: that wait_sync answers the status, the next one a record again
    int sync_st[2] = {0, 0};
    for (int k = 0; k < 2; k++) {
        dabgpu_sync_state rec;
        fill(rx[k], seed[k] + 30);
        fake_dabgpu_bank_fail_rounds(1, INJECTED);
        CK(dabgpu_receiver_submit_sync(rx[k], &CFG, PRS_AT));
        sync_st[k] = dabgpu_receiver_wait_sync(rx[k], &rec, nullptr, nullptr);
        sync(rx[k], seed[k] + 31);
        st[k][4] = collect_st(rx[k], post(rx[k], seed[k] + 32), &got[k][4]);
    }
    // the device reports the failure when it is waited for (wait_frames): that frame's generation only
    for (int k = 0; k < 2; k++) {
        sync(rx[k], seed[k] + 40);
        fake_dabgpu_bank_fail_waits(1, INJECTED);
        st[k][5] = collect_st(rx[k], post(rx[k], seed[k] + 41), &got[k][5]);
        sync(rx[k], seed[k] + 50);
        st[k][6] = collect_st(rx[k], post(rx[k], seed[k] + 51), &got[k][6]);
    }
    for (int k = 0; k < 2; k++) dabgpu_receiver_destroy(rx[k]);
    bool later_ok = true, digests_ok = true;
    for (int k = 0; k < 2; k++) {
        later_ok = later_ok && st[k][0] == DABGPU_OK && st[k][3] == DABGPU_OK && st[k][4] == DABGPU_OK && st[k][5] == INJECTED && st[k][6] == DABGPU_OK;
        for (int f = 0; f < 7; f++) if (st[k][f] == DABGPU_OK) digests_ok = digests_ok && got[k][f] == want[k][f] && got[k][f] != 0;
    }
    const bool syncs_ok = sync_st[0] == INJECTED && sync_st[1] == INJECTED;
    const bool ok = frames_ok && later_ok && digests_ok && syncs_ok;
    std::printf("{\"status_member0\": [%d, %d, %d, %d, %d, %d, %d], \"status_member1\": [%d, %d, %d, %d, %d, %d, %d], \"failed_sync\": [%d, %d], \"injected\": %d, "
                "\"delivered_equal_private\": %s, \"ok\": %s}\n", st[0][0], st[0][1], st[0][2], st[0][3], st[0][4], st[0][5], st[0][6], st[1][0], st[1][1], st[1][2], st[1][3],
                st[1][4], st[1][5], st[1][6], sync_st[0], sync_st[1], INJECTED, digests_ok ? "true" : "false", ok ? "true" : "false");
    return ok ? 0 : 1;
}

// ---- late_destroy ----
int late_destroy() {
    dabgpu_receiver *priv = nullptr, *rx[2] = {nullptr, nullptr};
    CK(dabgpu_receiver_create(&priv, 0, 1, nullptr, nullptr));
    std::vector<uint64_t> want, got[2];
    run(priv, 7, 1, false, want);
    dabgpu_receiver_destroy(priv);
    for (int k = 0; k < 2; k++) { CK(dabgpu_receiver_create_banked(&rx[k], 0)); run(rx[k], 7, 1, false, got[k]); }
    dabgpu_rx_bank_shutdown();
    int members = -2, refs = -2;
    dabgpu_rx_bank_census(0, &members, &refs);                 // (-1, -1: the device has no bank any more; the members keep theirs)
    // what was delivered stays with the member; what it posts now is refused, with a status
    dabgpu_receiver_frame f{};
    const int again = dabgpu_receiver_wait_frame(rx[0], 0, &f);
    const bool kept = again == DABGPU_OK && f.generation == 0 && fnv(f.bits, f.n_bits) == want[0];
    fill(rx[1], 9);
    const int post_sync = dabgpu_receiver_submit_sync(rx[1], &CFG, PRS_AT);
    uint64_t g = 0;
    const int post_frame = dabgpu_receiver_submit_frame(rx[1], FRAME_AT, CFG.fine_freq_update_beta, 0, 0, &g);
    const int reset = dabgpu_receiver_reset(rx[1]);
    for (int k = 0; k < 2; k++) dabgpu_receiver_destroy(rx[k]);
    // a bank made afterwards is a new one and works
    dabgpu_receiver* next = nullptr;
    CK(dabgpu_receiver_create_banked(&next, 0));
    std::vector<uint64_t> got_next;
    run(next, 7, 1, false, got_next);
    dabgpu_receiver_destroy(next);
    const bool ok = got[0] == want && got[1] == want && want[0] != 0 && members == -1 && refs == -1 && kept && post_sync != DABGPU_OK && post_frame != DABGPU_OK &&
                    reset != DABGPU_OK && got_next == want;
    std::printf("{\"frames_equal_private\": %s, \"bank_after_shutdown\": [%d, %d], \"delivered_frame_kept\": %s, \"posts_after_shutdown\": [%d, %d, %d], "
                "\"new_bank_works\": %s, \"ok\": %s}\n", got[0] == want && got[1] == want ? "true" : "false", members, refs, kept ? "true" : "false", post_sync, post_frame, reset,
                got_next == want ? "true" : "false", ok ? "true" : "false");
    return ok ? 0 : 1;
}

// ---- shutdown_with_queue ----
int shutdown_with_queue() {
    // one round at a time: the worker forms the next round only when the one before is handed out -- the moment at which completers that looked at `stop`
    // alone had left, with the two jobs behind the held round still in the queue
    setenv("DABGPU_BANK_ROUNDS", "1", 1);
    dabgpu_receiver *priv = nullptr, *rx = nullptr;
    CK(dabgpu_receiver_create(&priv, 0, 1, nullptr, nullptr));
    std::vector<uint64_t> want;
    run(priv, 7, 2, false, want);
    dabgpu_receiver_destroy(priv);
    CK(dabgpu_receiver_create_banked(&rx, 0));
    sync(rx, 7);
    const int e0 = fake_dabgpu_bank_enqueues();
    fake_dabgpu_bank_hold(1);
    const uint64_t g0 = post(rx, 8);
    until_enqueues(e0 + 1);                                    // the worker sits in the round of frame 0
    const uint64_t g1 = post(rx, 9);
    fill(rx, 10);
    CK(dabgpu_receiver_submit_sync(rx, &CFG, PRS_AT));       // queue behind the held round: [frame 1, synchroniser]
    std::atomic<bool> down{false};
    std::thread closer([&down] { dabgpu_rx_bank_shutdown(); down = true; });
    std::this_thread::sleep_for(std::chrono::milliseconds(20));    // (the closer has set `stop` and waits for the worker -- or does so a moment later: both orders must end)
    fake_dabgpu_bank_hold(0);
    uint64_t d0 = 0, d1 = 0;
    dabgpu_sync_state rec;
    const int s0 = collect_st(rx, g0, &d0), s1 = collect_st(rx, g1, &d1);
    const int ss = dabgpu_receiver_wait_sync(rx, &rec, nullptr, nullptr);
    closer.join();
    dabgpu_receiver_destroy(rx);
    // every wait returned (we are here); a result where the status says so is the private receiver's
    const bool ok = down && g0 == 0 && g1 == 1 && (s0 != DABGPU_OK || d0 == want[0]) && (s1 != DABGPU_OK || d1 == want[1]) && want[0] != 0;
    std::printf("{\"wait_frame\": [%d, %d], \"wait_sync\": %d, \"results_equal_private\": %s, \"shutdown_returned\": %s, \"ok\": %s}\n", s0, s1, ss,
                (s0 != DABGPU_OK || d0 == want[0]) && (s1 != DABGPU_OK || d1 == want[1]) ? "true" : "false", down ? "true" : "false", ok ? "true" : "false");
    return ok ? 0 : 1;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "backlog")) return backlog();
    if (argc == 2 && !std::strcmp(argv[1], "churn")) return churn();
    if (argc == 2 && !std::strcmp(argv[1], "failed_round")) return failed_round();
    if (argc == 2 && !std::strcmp(argv[1], "late_destroy")) return late_destroy();
    if (argc == 2 && !std::strcmp(argv[1], "shutdown_with_queue")) return shutdown_with_queue();
    std::fprintf(stderr, "usage: %s backlog | churn | failed_round | late_destroy | shutdown_with_queue\n", argv[0]);
    return 2;
}
