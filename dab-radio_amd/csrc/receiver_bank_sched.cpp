// receiver_bank_sched.cpp -- the receiver bank's HOST SCHEDULING half (plain C++, no device runtime; receiver_bank.hip is the device half and says what a
// bank is).  What happens when: the members' posts enter one queue; a worker thread forms rounds out of it -- at most one job per receiver, in posting
// order -- and has the device enqueue them (rx_bank_device, receiver_bank_sched.h); two completer threads wait for the rounds in order and hand the
// results to the members, one the synchronisers' records, one the frames.  Part of the device-free code of the library: tests/test_host_sanitizers.py
// builds it under ThreadSanitizer and ASan + UBSan over a CPU implementation of rx_bank_device.
#include <pthread.h>
#include <stdio.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <thread>

#include "dabgpu_host_logic.h"
#include "receiver_bank_sched.h"

namespace {
constexpr int MAXM = DABGPU_RX_BANK_MAX, TICKS = RX_BANK_TICKS, R = RX_BANK_SLOTS;
constexpr size_t NFFT = DABGPU_NB_FFT;
}

struct dabgpu_rx_bank {
    int device = 0;
    rx_bank_device* dev = nullptr;
    int n_up = 0;                                // DABGPU_BANK_UPLOADS: how many upload streams are used; 0 = one up to 12 members, all of them beyond (measured: a round of
                                                 // 8 members waits on ONE event instead of three -- 12.0-13.9 k frames/s against 9.5-11.3 k -- and 32 members' uploads
                                                 // overlap on three DMA engines -- 17.2-18.5 k against 13.9-14.6 k on one)
    rx_bank_round ticks[TICKS];
    uint64_t n_ticks = 0;                       // ticks enqueued
    uint64_t n_handed = 0;                      // ticks whose frames were handed out (and that are free again)
    uint64_t n_sync_handed = 0;                 // ticks whose synchroniser records were handed out
    dabgpu_rx_member* members[MAXM] = {nullptr};
    // the decoders' subscription (process-wide in the classes above: dabgpu_frame_batcher)
    std::vector<dabgpu_subchannel> subs; std::vector<uint32_t> sub_off, sub_n; uint32_t cif_out = 0; bool fic = false;
    std::mutex mu;
    std::condition_variable cv_jobs, cv_done, cv_ticks;
    std::deque<rx_bank_job> jobs;
    bool stop = false;                           // shutdown: nothing more is posted; the worker forms rounds until the queue is empty, the completers hand all of them out
    bool worker_done = false;                    // the worker has returned: n_ticks is final
    std::thread worker, completer, sync_completer;
    int refs = 0;
    // shutdown with members left (receivers destroyed after it, e.g. by destructors that run behind the atexit handler): the bank is stopped and taken
    // out of g_banks but stays, with its device half, for the members' results and their leave; the last leave frees it.  Both under g_banks_mu.
    int attached = 0;                            // members between join and the end of their leave
    bool detached = false;
    // DABGPU_BANK_PROFILE=1: what the rounds looked like, printed at shutdown
    bool profile = false;
    int gather_us = 1000;                        // DABGPU_BANK_GATHER_US
    int max_rounds = 2;                          // DABGPU_BANK_ROUNDS: rounds enqueued and not yet handed out
    uint64_t p_sync_jobs = 0, p_frame_jobs = 0, p_ticks_with_frames = 0;
    double p_enqueue_us = 0, p_wait_sync_us = 0, p_wait_frames_us = 0, p_handout_us = 0, p_worker_idle_us = 0;
};

namespace {
double bank_now_us() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3; }
std::mutex g_banks_mu;
dabgpu_rx_bank* g_banks[16] = {nullptr};
// The worker's timed waits.  wait_for on the steady clock is pthread_cond_clockwait, which GCC 11's ThreadSanitizer runtime does not intercept: it misses the
// unlock inside and reports "double lock of a mutex" at the next thread's lock.  In a build under that sanitizer alone the wait goes through pthread_cond_timedwait.
template <class P> void wait_us(std::condition_variable& cv, std::unique_lock<std::mutex>& lock, int us, P pred) {
#if defined(__SANITIZE_THREAD__)
    cv.wait_until(lock, std::chrono::system_clock::now() + std::chrono::microseconds(us), pred);
#else
    cv.wait_for(lock, std::chrono::microseconds(us), pred);
#endif
}

void worker_main(dabgpu_rx_bank* b) {
    pthread_setname_np(pthread_self(), "dabgpu-bank");
    b->dev->bind_thread();
    for (;;) {
        std::unique_lock<std::mutex> lock(b->mu);
        const double ti0 = b->profile ? bank_now_us() : 0.0;
        b->cv_jobs.wait(lock, [b] { return b->stop || !b->jobs.empty(); });
        if (b->profile && b->n_ticks) b->p_worker_idle_us += bank_now_us() - ti0;       // (not the wait for the very first job: the members are still being constructed)
        if (b->stop && b->jobs.empty()) {                                  // (nothing is posted to a stopped bank: the queue stays empty)
            b->worker_done = true;
            lock.unlock();
            b->cv_done.notify_all();
            return;
        }
        if (b->gather_us > 0) {
            // (1) A frame was posted a moment ago and the synchroniser of the NEXT frame is not in the queue yet: the reader posts it as soon as it has read the
            // NULL symbol and the PRS that follow (tens of us, when the samples are there) -- a round formed in between carries the frame alone and the
            // synchroniser waits for the round after it (a third of the rounds of two members carried a synchroniser only).  At most 150 us after the post.
            auto follows = [b] {
                if (b->stop) return true;
                bool frame_q[MAXM] = {false}, sync_q[MAXM] = {false};
                for (const auto& j : b->jobs) { if (j.kind == rx_bank_job::SYNC) sync_q[j.m->slot] = true; else if (j.kind == rx_bank_job::FRAME) frame_q[j.m->slot] = true; }
                const double now = bank_now_us();
                for (int k = 0; k < MAXM; k++) {
                    const dabgpu_rx_member* m = b->members[k];
                    if (m && frame_q[k] && !sync_q[k] && m->sync_state == 0 && now - m->last_post_us < 150.0) return false;
                }
                return true;
            };
            for (int spin = 0; spin < 4 && !follows(); spin++) wait_us(b->cv_jobs, lock, 50, follows);
            // (2) several members: give the others a moment to post as well (a round costs ~25 runtime calls whatever it carries; the calls, not the
            // device, are what a process can issue only so many of per second) -- at most `gather_us`, and not at all for a lone member
            const double t_first = bank_now_us();
            auto all_in = [b, t_first] {                                   // every member that posted in the last few ms has a job in the queue again
                if (b->stop) return true;
                bool in_queue[MAXM] = {false};
                for (const auto& j : b->jobs) in_queue[j.m->slot] = true;
                for (int k = 0; k < MAXM; k++) {
                    const dabgpu_rx_member* m = b->members[k];
                    // a member with a job under way is waiting for THIS thread's rounds and will not post before they are handed out: only the ones
                    // that are buffering on their own (nothing in flight) and posted recently are worth waiting for
                    if (m && !in_queue[k] && m->jobs_in_flight == 0 && t_first - m->last_post_us < 4000.0) return false;
                    // ... and the ones that have just been handed a synchroniser's record: their frame follows within a few hundred us (what is left of
                    // it to buffer, the post), whatever of theirs is still being decoded -- a round formed before they arrive carries half the members
                    if (m && !in_queue[k] && !m->posted_since_record && t_first - m->last_record_us < 700.0) return false;
                }
                return true;
            };
            if (b->refs > 1 && !all_in()) wait_us(b->cv_jobs, lock, b->gather_us, all_in);
        }
        // Rounds are not enqueued ahead of the device: a round takes what is queued when it is formed, and with a deep queue of rounds under way every
        // job that arrives meanwhile becomes a small round of its own at the END of that queue -- many small rounds, each paying the fixed costs, each
        // member waiting for all of them (measured at 32 members: 4 frames per round, 8 rounds deep, 3 ms from posting a synchroniser to its record).
        // At most `max_rounds` are under way; what arrives while they run forms the next one, whose size so follows the load (group commit).
        b->cv_ticks.wait(lock, [b] { return b->n_ticks - b->n_handed < (uint64_t)b->max_rounds; });
        const uint64_t tick_no = b->n_ticks;
        rx_bank_round& t = b->ticks[tick_no % TICKS];
        b->cv_ticks.wait(lock, [&] { return !t.busy; });                  // (the completer hands ticks out in order: at most TICKS are under way)
        t.no = tick_no;
        t.sync_jobs.clear(); t.frame_jobs.clear(); t.resets.clear();
        int taken[MAXM] = {0};                                             // 0 nothing yet, 1 its frame is in (its next synchroniser may follow), 2 closed
        // Per member, in posting order: its oldest job, and -- when that is a frame -- the synchroniser of the NEXT frame as well: a round runs its
        // frames first (upload, demodulation, fine-frequency update) and its synchronisers behind them on the same stream, so the synchroniser still
        // reads the fine-frequency word the frame's update wrote.  Synchronisers / frames with another configuration wait a round.
        for (auto it = b->jobs.begin(); it != b->jobs.end();) {
            const int slot = it->m->slot;
            bool take = taken[slot] == 0 || (taken[slot] == 1 && it->kind == rx_bank_job::SYNC);
            if (take && it->kind == rx_bank_job::SYNC && !t.sync_jobs.empty() && memcmp(&t.sync_jobs[0].cfg, &it->cfg, sizeof(dabgpu_sync_cfg)) != 0) take = false;
            if (take && it->kind == rx_bank_job::FRAME && !t.frame_jobs.empty() && (t.frame_jobs[0].beta != it->beta || t.frame_jobs[0].tie != it->tie)) take = false;
            if (!take) { taken[slot] = 2; ++it; continue; }                // (a job left behind blocks the member's later ones: order)
            taken[slot] = (it->kind == rx_bank_job::FRAME && taken[slot] == 0) ? 1 : 2;
            if (it->kind == rx_bank_job::SYNC) t.sync_jobs.push_back(*it);
            else if (it->kind == rx_bank_job::FRAME) t.frame_jobs.push_back(*it);
            else t.resets.push_back(*it);                                  // (:277-289, behind everything enqueued for the member so far)
            it = b->jobs.erase(it);
        }
        t.subs = b->subs; t.sub_off = b->sub_off; t.sub_n = b->sub_n; t.cif_out = b->cif_out; t.fic = b->fic;
        t.busy = true;
        b->n_ticks = tick_no + 1;
        lock.unlock();
        const double te0 = b->profile ? bank_now_us() : 0.0;
        const int st = b->dev->enqueue(t);
        if (b->profile) { b->p_enqueue_us += bank_now_us() - te0; b->p_sync_jobs += t.sync_jobs.size(); b->p_frame_jobs += t.frame_jobs.size(); b->p_ticks_with_frames += t.frame_jobs.empty() ? 0 : 1; }
        lock.lock();
        t.status = st;
        for (const auto& j : t.sync_jobs) j.m->sync_state = 2;
        for (const auto& r : t.resets) { r.m->jobs_in_flight--; r.m->cv.notify_all(); }
        lock.unlock();
        b->cv_done.notify_all();                                           // (the two completers)
    }
}

// The synchronisers' records, round by round: the readers wait for them (they cannot finish buffering the frame before), so they do not queue
// behind the decode of the same or an earlier round
void sync_completer_main(dabgpu_rx_bank* b) {
    pthread_setname_np(pthread_self(), "dabgpu-bk-sync");
    b->dev->bind_thread();
    for (;;) {
        std::unique_lock<std::mutex> lock(b->mu);
        // (leaves when the worker has returned and its last round is handed out: `stop` alone is too early, the worker still forms rounds out of what is queued)
        b->cv_done.wait(lock, [b] { return (b->worker_done && b->n_sync_handed == b->n_ticks) || (b->n_sync_handed < b->n_ticks && b->ticks[b->n_sync_handed % TICKS].status != -1); });
        if (b->n_sync_handed == b->n_ticks) return;
        rx_bank_round& t = b->ticks[b->n_sync_handed % TICKS];
        lock.unlock();
        int st = t.status;
        const double tc0 = b->profile ? bank_now_us() : 0.0;
        if (!st && !t.sync_jobs.empty()) st = b->dev->wait_sync(t);
        if (b->profile) b->p_wait_sync_us += bank_now_us() - tc0;
        lock.lock();
        for (size_t k = 0; k < t.sync_jobs.size(); k++) {
            dabgpu_rx_member* m = t.sync_jobs[k].m;
            m->sync_status = st;
            if (!st) b->dev->hand_sync(t, k);
            m->sync_state = 3;
            m->jobs_in_flight--;
            if (!st && m->sync_rec.sync_valid) { m->last_record_us = bank_now_us(); m->posted_since_record = false; }
            m->cv.notify_all();
        }
        t.sync_handed = true;
        b->n_sync_handed++;
        lock.unlock();
        b->cv_done.notify_all();
    }
}

// The frames, round by round: waits for the device, has every frame's results delivered to its member's result store, wakes the members, frees the round
void completer_main(dabgpu_rx_bank* b) {
    pthread_setname_np(pthread_self(), "dabgpu-bk-frm");
    b->dev->bind_thread();
    for (;;) {
        std::unique_lock<std::mutex> lock(b->mu);
        b->cv_done.wait(lock, [b] { return (b->worker_done && b->n_handed == b->n_ticks) || (b->n_handed < b->n_ticks && b->ticks[b->n_handed % TICKS].status != -1); });
        if (b->n_handed == b->n_ticks) return;
        rx_bank_round& t = b->ticks[b->n_handed % TICKS];
        lock.unlock();
        int st = t.status;
        const double tc0 = b->profile ? bank_now_us() : 0.0;
        if (!t.frame_jobs.empty()) {
            if (!st) st = b->dev->wait_frames(t);
            if (b->profile) b->p_wait_frames_us += bank_now_us() - tc0;
            for (size_t j = 0; j < t.frame_jobs.size(); j++) st = b->dev->deliver_frame(t, j, st);
            lock.lock();
            for (const auto& f : t.frame_jobs) {
                f.m->frame_status[f.gen % R] = st;                         // this generation's: the slot's next frame writes its own
                f.m->done_gen = f.gen + 1;
                f.m->jobs_in_flight--;
                f.m->cv.notify_all();
            }
            lock.unlock();
            b->cv_done.notify_all();
        }
        if ((b->n_handed & 31) == 31) b->dev->drain_uploads();             // every 32nd round, on this thread (not the worker's): see receiver_bank.hip
        lock.lock();
        b->cv_done.wait(lock, [&] { return t.sync_handed; });
        if (b->profile) b->p_handout_us += bank_now_us() - tc0;
        t.busy = false;
        t.sync_handed = false;
        t.status = -1;
        b->n_handed++;
        lock.unlock();
        b->cv_done.notify_all();
        b->cv_ticks.notify_all();
    }
}
}  // namespace

// ---- what receiver.hip calls ----
int dabgpu_rx_bank_join(int device, float* const* h_stage, dabgpu_rx_member** out) {
    *out = nullptr;
    if (device < 0 || device >= 16) { dabgpu_set_error("receiver bank: device %d out of range", device); return DABGPU_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> g(g_banks_mu);
    dabgpu_rx_bank* b = g_banks[device];
    int st = DABGPU_OK;
    if (!b) {
        rx_bank_device* dev = nullptr;
        if ((st = dabgpu_rx_bank_device_open(device, &dev))) return st;
        b = new dabgpu_rx_bank();
        b->device = device;
        b->dev = dev;
        if (const char* e = std::getenv("DABGPU_BANK_PROFILE")) b->profile = std::atoi(e) != 0;
        if (const char* e = std::getenv("DABGPU_BANK_GATHER_US")) b->gather_us = std::atoi(e);
        if (const char* e = std::getenv("DABGPU_BANK_UPLOADS")) b->n_up = std::min(RX_BANK_UPLOADS, std::max(0, std::atoi(e)));
        if (const char* e = std::getenv("DABGPU_BANK_ROUNDS")) b->max_rounds = std::min(TICKS, std::max(1, std::atoi(e)));
        b->worker = std::thread(worker_main, b);
        b->completer = std::thread(completer_main, b);
        b->sync_completer = std::thread(sync_completer_main, b);
        g_banks[device] = b;
        static bool registered = false;                                    // (the device runtime registered its own teardown earlier: this one runs before it)
        if (!registered) { registered = true; std::atexit(dabgpu_rx_bank_shutdown); }
    }
    dabgpu_rx_member* m = new dabgpu_rx_member();
    m->bank = b;
    m->h_stage = h_stage;
    {
        std::lock_guard<std::mutex> lock(b->mu);
        for (int k = 0; k < MAXM && m->slot < 0; k++) if (!b->members[k]) { b->members[k] = m; m->slot = k; }
        if (m->slot < 0) { dabgpu_set_error("receiver bank: more than %d receivers on one device", MAXM); st = DABGPU_ERR_INVALID_ARG; }
        else b->refs++;
    }
    if (!st) st = b->dev->member_open(m);
    if (st) {
        if (m->slot >= 0) { std::lock_guard<std::mutex> lock(b->mu); b->members[m->slot] = nullptr; b->refs--; }
        delete m;
        return st;
    }
    b->attached++;
    *out = m;
    return DABGPU_OK;
}

namespace {
void bank_free(dabgpu_rx_bank* b) { delete b->dev; delete b; }               // (its threads were joined)
}

void dabgpu_rx_bank_leave(dabgpu_rx_member* m) {
    if (!m) return;
    dabgpu_rx_bank* b = m->bank;
    {
        // (a stopped bank: its threads handed out every job before they returned, and none was accepted since)
        std::unique_lock<std::mutex> lock(b->mu);
        m->cv.wait(lock, [m] { return m->jobs_in_flight == 0; });
        b->members[m->slot] = nullptr;
        b->refs--;
    }
    b->dev->member_close(m);
    delete m;
    // the bank itself stays for the life of the process (its threads are joined by dabgpu_rx_bank_shutdown, which the library's unload calls) -- unless it
    // was shut down over this member's head: then the last member to leave frees it
    bool last;
    { std::lock_guard<std::mutex> g(g_banks_mu); last = --b->attached == 0 && b->detached; }
    if (last) bank_free(b);
}

dabgpu_frame_session* dabgpu_rx_bank_session(dabgpu_rx_member* m) { return m->ses; }

int dabgpu_rx_bank_set_subchannels(dabgpu_rx_member* m, const dabgpu_subchannel* subs, int n, int decode_fic) {
    if (n < 0 || n > 64 || (n && !subs)) { dabgpu_set_error("receiver bank: invalid sub-channel list"); return DABGPU_ERR_INVALID_ARG; }
    std::vector<uint32_t> off((size_t)n), nb((size_t)n);
    uint32_t total = 0;
    if (n) {
        std::vector<dabgpu_msc_plan> plans;
        const int st = dabgpu_host_build_msc_plans(subs, n, plans, nullptr, nullptr, nullptr);
        if (st) return st;
    }
    for (int k = 0; k < n; k++) {
        int pi[4], lx[4], bytes = 0;
        if (dabgpu_subchannel_plan(&subs[k], pi, lx, &bytes) < 0) { dabgpu_set_error("receiver bank: sub-channel %d has an invalid protection profile", k); return DABGPU_ERR_INVALID_ARG; }
        off[(size_t)k] = total; nb[(size_t)k] = (uint32_t)bytes; total += (uint32_t)bytes;
    }
    dabgpu_rx_bank* b = m->bank;
    std::lock_guard<std::mutex> lock(b->mu);
    // the decoders' list is process-wide (dabgpu_frame_batcher): every member reports the same one; it applies from the next tick on
    b->subs.assign(subs, subs + n); b->sub_off = off; b->sub_n = nb; b->cif_out = total; b->fic = decode_fic != 0;
    return DABGPU_OK;
}

namespace {
// under the bank's mutex, before a job is queued: a bank that was shut down takes none (its worker returns on an empty queue and nothing may follow)
int refuse_if_stopped(const dabgpu_rx_bank* b, const char* what) {
    if (!b->stop) return DABGPU_OK;
    dabgpu_set_error("%s: the receiver bank was shut down", what);
    return DABGPU_ERR_UNSUPPORTED;
}
}  // namespace

int dabgpu_rx_bank_reset(dabgpu_rx_member* m) {
    dabgpu_rx_bank* b = m->bank;
    {
        std::lock_guard<std::mutex> lock(b->mu);
        if (const int st = refuse_if_stopped(b, "receiver_reset")) return st;
        rx_bank_job j{}; j.kind = rx_bank_job::RESET; j.m = m; b->jobs.push_back(j); m->jobs_in_flight++;
    }
    b->cv_jobs.notify_one();
    return DABGPU_OK;
}

int dabgpu_rx_bank_post_sync(dabgpu_rx_member* m, const dabgpu_sync_cfg* cfg, int stage, size_t prs_sample) {
    dabgpu_rx_bank* b = m->bank;
    {
        std::lock_guard<std::mutex> lock(b->mu);
        if (m->sync_state != 0) { dabgpu_set_error("receiver_submit_sync: the previous record has not been collected (dabgpu_receiver_wait_sync)"); return DABGPU_ERR_INVALID_ARG; }
        if (const int st = refuse_if_stopped(b, "receiver_submit_sync")) return st;
    }
    // the member's row of the bank's PRS array is its own until the record has come back (one synchroniser at a time per member)
    memcpy(b->dev->prs_row(m->slot), m->h_stage[stage] + 2 * prs_sample, NFFT * 2 * sizeof(float));
    {
        std::lock_guard<std::mutex> lock(b->mu);
        if (const int st = refuse_if_stopped(b, "receiver_submit_sync")) return st;
        rx_bank_job j{}; j.kind = rx_bank_job::SYNC; j.m = m; j.stage = stage; j.sample = prs_sample; j.cfg = *cfg;
        b->jobs.push_back(j);
        m->sync_state = 1;
        m->jobs_in_flight++;
        m->last_post_us = bank_now_us();
    }
    b->cv_jobs.notify_one();
    return DABGPU_OK;
}

int dabgpu_rx_bank_sync_pending(dabgpu_rx_member* m) { std::lock_guard<std::mutex> lock(m->bank->mu); return m->sync_state != 0; }

int dabgpu_rx_bank_wait_sync(dabgpu_rx_member* m, dabgpu_sync_state* out, float* h_impulse, float* h_freq_response) {
    dabgpu_rx_bank* b = m->bank;
    std::unique_lock<std::mutex> lock(b->mu);
    if (m->sync_state == 0) { dabgpu_set_error("receiver_wait_sync: no synchronisation was submitted"); return DABGPU_ERR_NOT_READY; }
    m->cv.wait(lock, [m] { return m->sync_state == 3; });
    m->sync_state = 0;
    if (m->sync_status) { dabgpu_set_error("receiver bank: the tick that carried the synchroniser failed"); return m->sync_status; }
    *out = m->sync_rec;
    if (h_impulse) memcpy(h_impulse, m->sync_imp.data(), NFFT * sizeof(float));
    if (h_freq_response && m->sync_coarse) memcpy(h_freq_response, m->sync_frq.data(), NFFT * sizeof(float));
    return DABGPU_OK;
}

int dabgpu_rx_bank_post_frame(dabgpu_rx_member* m, int stage, size_t frame_sample, float beta, int want_views, int tie, uint64_t* generation) {
    dabgpu_rx_bank* b = m->bank;
    uint64_t gen;
    int n_up;
    {
        std::lock_guard<std::mutex> lock(b->mu);
        if (const int st = refuse_if_stopped(b, "receiver_submit_frame")) return st;
        if (m->next_gen >= m->done_gen + (uint64_t)(R - 1)) {
            dabgpu_set_error("receiver_submit_frame: %d frames submitted and not yet collected (at most %d)", (int)(m->next_gen - m->done_gen), R - 1);
            return DABGPU_ERR_NOT_READY;
        }
        gen = m->next_gen;                                                 // (only the member's own thread posts)
        n_up = b->n_up > 0 ? b->n_up : (b->refs <= 12 ? 1 : RX_BANK_UPLOADS);
    }
    // The member uploads its frame itself, now: the samples cross PCIe while the rounds under way run, not inside the round that demodulates them
    // (32 frames of a round are 1 ms of PCIe in front of the round's synchronisers otherwise)
    const int up_k = m->slot % n_up;
    const float* d = nullptr;
    const int st = b->dev->upload(m, stage, frame_sample, gen, up_k, &d);
    if (st) return st;
    {
        std::lock_guard<std::mutex> lock(b->mu);
        if (const int st2 = refuse_if_stopped(b, "receiver_submit_frame")) return st2;     // (stopped during the upload: the copy is made, no round reads it)
        rx_bank_job j{}; j.kind = rx_bank_job::FRAME; j.m = m; j.stage = stage; j.sample = frame_sample; j.beta = beta; j.want_views = want_views; j.tie = tie;
        j.gen = gen; j.d_iq = d; j.up = up_k;
        m->next_gen = gen + 1;
        b->jobs.push_back(j);                                              // (after the copy was enqueued: the round's event on that stream lies behind it)
        m->stage_state[stage] = 2;
        m->jobs_in_flight++;
        m->last_post_us = bank_now_us();
        m->posted_since_record = true;
        if (generation) *generation = gen;
    }
    b->cv_jobs.notify_one();
    return DABGPU_OK;
}

// the staging buffer `stage` may be written again: the frame that was read from it has been uploaded
int dabgpu_rx_bank_wait_stage(dabgpu_rx_member* m, int stage) {
    dabgpu_rx_bank* b = m->bank;
    {
        std::lock_guard<std::mutex> lock(b->mu);
        if (m->stage_state[stage] == 0) return DABGPU_OK;
    }
    const int st = b->dev->wait_stage(m, stage);
    { std::lock_guard<std::mutex> lock(b->mu); m->stage_state[stage] = 0; }
    return st;
}

int dabgpu_rx_bank_wait_frame(dabgpu_rx_member* m, uint64_t generation, dabgpu_receiver_frame* out) {
    dabgpu_rx_bank* b = m->bank;
    {
        std::unique_lock<std::mutex> lock(b->mu);
        if (generation >= m->next_gen) { dabgpu_set_error("receiver_wait_frame: generation %llu was never submitted", (unsigned long long)generation); return DABGPU_ERR_NOT_READY; }
        m->cv.wait(lock, [&] { return m->done_gen > generation; });
        // (the status of THIS generation: its place is written again when generation + R is handed out, and then the frame is gone anyway -- fetch_frame says so)
        const int st = m->done_gen <= generation + (uint64_t)R ? m->frame_status[generation % R] : DABGPU_OK;
        if (st) { dabgpu_set_error("receiver bank: the tick that carried the frame failed"); return st; }
    }
    return b->dev->fetch_frame(m, generation, out);
}

void dabgpu_rx_bank_census(int device, int* members, int* refs) {
    std::lock_guard<std::mutex> g(g_banks_mu);
    dabgpu_rx_bank* b = device >= 0 && device < 16 ? g_banks[device] : nullptr;
    *members = *refs = -1;
    if (!b) return;
    std::lock_guard<std::mutex> lock(b->mu);
    *members = (int)std::count_if(b->members, b->members + MAXM, [](const dabgpu_rx_member* m) { return m != nullptr; });
    *refs = b->refs;
}

void dabgpu_rx_bank_shutdown(void) {
    std::lock_guard<std::mutex> g(g_banks_mu);
    for (auto& b : g_banks) {
        if (!b) continue;
        { std::lock_guard<std::mutex> lock(b->mu); b->stop = true; }
        b->cv_jobs.notify_all(); b->cv_done.notify_all();
        if (b->worker.joinable()) b->worker.join();
        if (b->completer.joinable()) b->completer.join();
        if (b->sync_completer.joinable()) b->sync_completer.join();
        // (every job that was queued has been handed out: the worker returns on an empty queue only, the completers after its last round)
        if (b->profile && b->n_ticks)
            fprintf(stderr, "receiver bank (device %d): %llu rounds, %llu with frames; %.2f frames and %.2f synchronisers per round; per round us: enqueue %.1f, completer { wait sync %.1f, "
                            "wait frames %.1f, whole hand-out %.1f }; worker idle %.1f\n", b->device, (unsigned long long)b->n_ticks, (unsigned long long)b->p_ticks_with_frames,
                    (double)b->p_frame_jobs / (double)b->n_ticks, (double)b->p_sync_jobs / (double)b->n_ticks, b->p_enqueue_us / (double)b->n_ticks, b->p_wait_sync_us / (double)b->n_ticks,
                    b->p_wait_frames_us / (double)b->n_ticks, b->p_handout_us / (double)b->n_ticks, b->p_worker_idle_us / (double)b->n_ticks);
        // members left (a receiver destroyed behind this call): they keep the stopped bank -- their results stay fetchable, what they post is refused -- and
        // the last of them to leave frees it
        if (b->attached > 0) b->detached = true;
        else bank_free(b);
        b = nullptr;
    }
}
