// receiver_bank.hip -- many receivers of one process behind ONE pair of device streams ("all code words of all ensembles in one launch",
// for the drop-in classes).  VERDICT r5 item 4b: N OFDM_Demod objects, each with a receiver pipeline of its own (receiver.hip: three streams, ~20
// runtime calls and ~12 small device operations per frame), saturated at 6.5-7.3 k frames/s whatever N -- the device front end's limit, ~1 % of what
// the batch entry points do.  A BANKED receiver (dabgpu_receiver_create with DABGPU_RX_BANKED) keeps the whole dabgpu_receiver_* interface, but its
// submit_* calls only POST a job; one worker thread per device takes what has been posted since its last round -- at most one job per receiver, in
// posting order -- and issues it as one TICK:
//   stream A   H2D of the posted PRS slots -> ONE ofdm_sync_kernel over the member slots (active mask) -> D2H of the records
//              H2D of the posted frames into a compact batch -> gather of the members' offsets -> ONE ofdm_demod_kernel (+ phase kernel) over the batch
//              -> scatter of the soft bits into the members' history rings and of the fine-frequency words into their device records -> D2H
//   stream B   ONE dabgpu_decode_ring_layout over the member rings (inactive members skipped) -> D2H of the result arrays
// and a second thread hands the finished ticks' results to the members (their result slots are the frame session's, so FIC_Decoder / MSC_Decoder
// fetch exactly as from a private receiver).  No artificial wait: under load the ticks fill by themselves (while one is being enqueued the other
// receivers post), at low load a tick is one receiver's job.  Arithmetic, per-receiver ordering (frame k's fine-frequency update precedes frame
// k + 1's synchroniser) and every output are those of the private pipeline: the same kernels run on the same inputs
// (tests/test_gpu_cpp_mirror.py, tests/test_gpu_receiver.py run both forms).
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <stdio.h>
#include <string.h>
#include <time.h>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "receiver_bank.h"

namespace {
constexpr int MAXM = DABGPU_RX_BANK_MAX, H = dabgpu_frame_session::H, TICKS = 8;
constexpr size_t FRAME_SAMPLES = DABGPU_NB_FRAME_SAMPLES, FRAME_BITS = DABGPU_NB_FRAME_BITS, NFFT = DABGPU_NB_FFT;

// per tick, uploaded in one copy: which member every batch entry belongs to, where its soft bits go, which members sync / decode
struct tick_table {
    int32_t sync_active[MAXM];      // ofdm_sync_kernel's mask over member slots
    int32_t newest[MAXM];           // decode: ring slot of the frame of this tick, -1 = no frame
    int32_t slot_of[MAXM];          // batch entry j -> member slot
    int32_t ring_of[MAXM];          // batch entry j -> history ring slot (generation % H)
    const float* iq_of[MAXM];       // batch entry j -> where its member uploaded the frame's samples
};

__global__ void bank_gather_kernel(const dabgpu_sync_state* __restrict__ st, const tick_table* __restrict__ tab, int n, float* __restrict__ freq, float* __restrict__ fine) {
    const int j = (int)threadIdx.x;
    if (j < n) {
        const dabgpu_sync_state s = st[tab->slot_of[j]];
        freq[j] = s.freq_coarse + s.freq_fine;                       // ofdm_demodulator.cpp:672
        fine[j] = s.freq_fine;
    }
}
// the samples of batch entry j, from the buffer its member uploaded them to, into the compact batch the demodulation kernel reads
__global__ void bank_gather_iq_kernel(float* __restrict__ batch, const tick_table* __restrict__ tab) {
    const int j = (int)blockIdx.y;
    const uint4* src = reinterpret_cast<const uint4*>(tab->iq_of[j]);
    uint4* dst = reinterpret_cast<uint4*>(batch + (size_t)j * FRAME_SAMPLES * 2);
    constexpr size_t N = FRAME_SAMPLES * 2 * sizeof(float) / 16;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
// soft bits of batch entry j -> its member's ring slot; the updated fine-frequency word -> the member's device record
__global__ void bank_scatter_kernel(const int8_t* __restrict__ bits, int8_t* __restrict__ hist, const tick_table* __restrict__ tab, const float* __restrict__ fine,
                                    dabgpu_sync_state* __restrict__ st) {
    const int j = (int)blockIdx.y;
    const int slot = tab->slot_of[j];
    const uint4* src = reinterpret_cast<const uint4*>(bits + (size_t)j * FRAME_BITS);
    uint4* dst = reinterpret_cast<uint4*>(hist + ((size_t)slot * H + (size_t)tab->ring_of[j]) * FRAME_BITS);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < FRAME_BITS / 16; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) st[slot].freq_fine = fine[j];
}
}  // namespace

struct rx_bank_job {
    enum Kind { SYNC, FRAME, RESET } kind;
    dabgpu_rx_member* m;
    int stage;
    size_t sample;
    float beta;
    uint64_t gen;
    int want_views, tie;
    dabgpu_sync_cfg cfg;
    const float* d_iq;              // FRAME: the member's upload buffer that holds the samples
    int up;                         // FRAME: the upload stream the member's copy went to
};

struct dabgpu_rx_member {
    dabgpu_rx_bank* bank = nullptr;
    int slot = -1;
    dabgpu_frame_session* ses = nullptr;        // the member's result store (what the decoders fetch from)
    float* const* h_stage = nullptr;            // the receiver's staging buffers
    // reader -> worker -> completer, all under bank->mu
    int sync_state = 0;                         // 0 none, 1 posted, 2 enqueued, 3 done
    int sync_status = DABGPU_OK;
    bool sync_coarse = false;
    dabgpu_sync_state sync_rec;
    std::vector<float> sync_imp, sync_frq;
    float* d_iq = nullptr;                      // [2][frame]: the member uploads frame g to half g % 2 when it posts it (see dabgpu_rx_bank_post_frame)
    int stage_state[3] = {0, 0, 0};             // 0 free, 2 a frame was posted from it: its upload is enqueued (stage_ev recorded)
    hipEvent_t stage_ev[3] = {nullptr, nullptr, nullptr};
    uint64_t next_gen = 0;                      // next generation to post
    uint64_t done_gen = 0;                      // generations < done_gen have their results in the session's slots
    int frame_status = DABGPU_OK;
    int jobs_in_flight = 0;
    std::condition_variable cv;                 // the member's own threads wait here (on bank->mu): a hand-out wakes the members it concerns, not all of them
    double last_post_us = -1e18;                // when the member posted last (the worker's gathering rule)
    double last_record_us = -1e18;              // when a synchroniser's record was handed to the member last, and whether it has posted a frame since
    bool posted_since_record = true;
    // views (display buffers), allocated at first use
    float* d_fft = nullptr; float* d_dq = nullptr;
};

struct rx_bank_tick {
    tick_table* h_tab = nullptr;                // pinned
    dabgpu_sync_state* h_states = nullptr;      // pinned [MAXM]
    float* h_imp = nullptr; float* h_frq = nullptr;   // pinned [MAXM][NFFT]
    float* h_scal = nullptr;                    // pinned [2][MAXM]: fine after the update | total phase
    uint8_t* h_out = nullptr; size_t h_out_cap = 0;   // pinned: decode outputs of the tick [n_ens] x (fib | fres | mres | msc)
    hipEvent_t ev_sync = nullptr, ev_demod = nullptr, ev_copied = nullptr, ev_done = nullptr;
    std::vector<rx_bank_job> sync_jobs, frame_jobs;
    int n_ens = 0;                              // member slots covered by the decode
    bool decoded = false, fic = false;
    std::vector<dabgpu_subchannel> subs; std::vector<uint32_t> sub_off, sub_n; uint32_t cif_out = 0;
    int status = DABGPU_OK;
    bool busy = false;                          // enqueued, not yet handed out by the completers
    bool sync_handed = false;                   // the synchronisers' records of the round are with their members
};

struct dabgpu_rx_bank {
    int device = 0;
    dabgpu_ctx* ctx = nullptr;                  // tables; its stream = stream B (decode), its scratch = the decoder's
    hipStream_t a = nullptr;
    static constexpr int NUP = 3;               // upload streams (member slot % NUP): frames cross PCIe on several DMA engines at once
    hipStream_t up[NUP] = {nullptr, nullptr, nullptr};
    hipEvent_t up_ev[NUP] = {nullptr, nullptr, nullptr};
    int n_up = 0;                                // DABGPU_BANK_UPLOADS: how many of them are used; 0 = one up to 12 members, all of them beyond (measured: a round of
                                                 // 8 members waits on ONE event instead of three -- 12.0-13.9 k frames/s against 9.5-11.3 k -- and 32 members' uploads
                                                 // overlap on three DMA engines -- 17.2-18.5 k against 13.9-14.6 k on one)
    float* d_prs = nullptr; float* d_iq = nullptr; int8_t* d_bits = nullptr; int8_t* d_hist = nullptr;
    dabgpu_sync_state* d_states = nullptr; float* d_imp = nullptr; float* d_frq = nullptr;
    float* d_corr = nullptr; float* d_freq = nullptr; float* d_fine = nullptr; float* d_total = nullptr;
    tick_table* d_tab = nullptr;                // [TICKS]
    uint8_t* d_out = nullptr; size_t d_out_cap = 0;
    rx_bank_tick ticks[TICKS];
    uint64_t n_ticks = 0;                       // ticks enqueued
    uint64_t n_handed = 0;                      // ticks whose frames were handed out (and that are free again)
    uint64_t n_sync_handed = 0;                 // ticks whose synchroniser records were handed out
    float* h_prs = nullptr;                     // pinned [MAXM][NFFT] c32: the members copy their PRS slot here when they post (ONE upload per round)
    dabgpu_rx_member* members[MAXM] = {nullptr};
    // the decoders' subscription (process-wide in the classes above: dabgpu_frame_batcher)
    std::vector<dabgpu_subchannel> subs; std::vector<uint32_t> sub_off, sub_n; uint32_t cif_out = 0; bool fic = false;
    std::mutex mu;
    std::condition_variable cv_jobs, cv_done, cv_ticks;
    std::deque<rx_bank_job> jobs;
    bool stop = false;
    std::thread worker, completer, sync_completer;
    int refs = 0;
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

size_t out_bytes(size_t n_ens, size_t n_sub, size_t cif_out) {
    return n_ens * (4 * 96 + (4 + 4 * n_sub) * sizeof(dabgpu_codeword_result) + 4 * cif_out);
}
struct out_ptrs { uint8_t* fib; dabgpu_codeword_result* fres; dabgpu_codeword_result* mres; uint8_t* msc; };
out_ptrs out_layout(uint8_t* base, size_t n_ens, size_t n_sub, size_t cif_out) {
    out_ptrs p;
    p.fib = base;
    p.fres = reinterpret_cast<dabgpu_codeword_result*>(base + n_ens * 4 * 96);
    p.mres = p.fres + n_ens * 4;
    p.msc = reinterpret_cast<uint8_t*>(p.mres + n_ens * 4 * n_sub);
    (void)cif_out;
    return p;
}

#define BK(call) do { st = dabgpu_check_hip((call), #call); if (st) return st; } while (0)

int bank_alloc(dabgpu_rx_bank* b) {
    int st;
    BK(hipMalloc((void**)&b->d_prs, (size_t)MAXM * NFFT * 2 * sizeof(float)));
    BK(hipMalloc((void**)&b->d_iq, (size_t)MAXM * FRAME_SAMPLES * 2 * sizeof(float)));
    BK(hipMalloc((void**)&b->d_bits, (size_t)MAXM * FRAME_BITS));
    BK(hipMalloc((void**)&b->d_hist, (size_t)MAXM * H * FRAME_BITS));
    BK(hipMemsetAsync(b->d_hist, 0, (size_t)MAXM * H * FRAME_BITS, b->a));          // (stream A, not the NULL stream; join() synchronises it)
    BK(hipMalloc((void**)&b->d_states, (size_t)MAXM * sizeof(dabgpu_sync_state)));
    BK(hipMemsetAsync(b->d_states, 0, (size_t)MAXM * sizeof(dabgpu_sync_state), b->a));
    BK(hipMalloc((void**)&b->d_imp, (size_t)MAXM * NFFT * sizeof(float)));
    BK(hipMalloc((void**)&b->d_frq, (size_t)MAXM * NFFT * sizeof(float)));
    BK(hipMalloc((void**)&b->d_corr, (size_t)MAXM * DABGPU_NB_FRAME_SYMBOLS * 2 * sizeof(float)));
    BK(hipMalloc((void**)&b->d_freq, (size_t)MAXM * sizeof(float)));
    BK(hipMalloc((void**)&b->d_fine, (size_t)2 * MAXM * sizeof(float)));            // [fine after the update | total phase]: one copy back per round
    b->d_total = b->d_fine + MAXM;
    BK(hipMalloc((void**)&b->d_tab, (size_t)TICKS * sizeof(tick_table)));
    BK(hipHostMalloc((void**)&b->h_prs, (size_t)MAXM * NFFT * 2 * sizeof(float), hipHostMallocDefault));
    for (int k = 0; k < dabgpu_rx_bank::NUP; k++) {
        BK(hipStreamCreateWithFlags(&b->up[k], hipStreamNonBlocking));
        BK(hipEventCreateWithFlags(&b->up_ev[k], dabgpu_wait_event_flags(true)));
    }
    for (auto& t : b->ticks) {
        BK(hipHostMalloc((void**)&t.h_tab, sizeof(tick_table), hipHostMallocDefault));
        BK(hipHostMalloc((void**)&t.h_states, (size_t)MAXM * sizeof(dabgpu_sync_state), hipHostMallocDefault));
        BK(hipHostMalloc((void**)&t.h_imp, (size_t)MAXM * NFFT * sizeof(float), hipHostMallocDefault));
        BK(hipHostMalloc((void**)&t.h_frq, (size_t)MAXM * NFFT * sizeof(float), hipHostMallocDefault));
        BK(hipHostMalloc((void**)&t.h_scal, (size_t)2 * MAXM * sizeof(float), hipHostMallocDefault));
        BK(hipEventCreateWithFlags(&t.ev_sync, dabgpu_wait_event_flags(true)));
        BK(hipEventCreateWithFlags(&t.ev_demod, dabgpu_wait_event_flags(true)));
        BK(hipEventCreateWithFlags(&t.ev_copied, dabgpu_wait_event_flags(true)));
        BK(hipEventCreateWithFlags(&t.ev_done, dabgpu_wait_event_flags(true)));
    }
    return DABGPU_OK;
}

// one tick on the two streams; returns the first failure (the tick's jobs are then completed with it)
int enqueue_tick(dabgpu_rx_bank* b, rx_bank_tick& t, uint64_t tick_no) {
    int st;
    dabgpu_ctx* c = b->ctx;
    hipStream_t a = b->a, q = c->stream;
    tick_table& tab = *t.h_tab;
    const int nS = (int)t.sync_jobs.size(), nF = (int)t.frame_jobs.size();
    int hi = -1;
    for (int k = 0; k < MAXM; k++) { tab.sync_active[k] = 0; tab.newest[k] = -1; tab.slot_of[k] = 0; tab.ring_of[k] = 0; tab.iq_of[k] = nullptr; }
    for (const auto& j : t.sync_jobs) { tab.sync_active[j.m->slot] = 1; if (j.m->slot > hi) hi = j.m->slot; }
    for (int j = 0; j < nF; j++) {
        const rx_bank_job& f = t.frame_jobs[(size_t)j];
        tab.slot_of[j] = f.m->slot; tab.ring_of[j] = (int)(f.gen % H); tab.iq_of[j] = f.d_iq;
        tab.newest[f.m->slot] = (int)(f.gen % H);
        if (f.m->slot > hi) hi = f.m->slot;
    }
    t.n_ens = hi + 1;
    tick_table* d_tab = b->d_tab + (tick_no % TICKS);
    BK(hipMemcpyAsync(d_tab, t.h_tab, sizeof(tick_table), hipMemcpyHostToDevice, a));
    // ---- frames ----
    t.decoded = false;
    bool frames_enqueued = false;
    if (nF) {
        // the uploads -- 1.5 MB per frame -- were enqueued by the members when they posted (on upload stream slot % NUP, BEFORE the job entered the queue):
        // an event recorded now on each of those streams lies behind them.  They crossed PCIe while the previous round ran and this one waited to be
        // formed; the round copies them (device to device, ~1 us each) into the compact batch the demodulation kernel reads.
        bool used[dabgpu_rx_bank::NUP] = {false, false, false};
        for (const auto& f : t.frame_jobs) used[f.up] = true;
        for (int k = 0; k < dabgpu_rx_bank::NUP; k++) if (used[k]) { BK(hipEventRecord(b->up_ev[k], b->up[k])); BK(hipStreamWaitEvent(a, b->up_ev[k], 0)); }
        bank_gather_iq_kernel<<<dim3(16, (unsigned)nF), 256, 0, a>>>(b->d_iq, d_tab);
        BK(hipGetLastError());
        bank_gather_kernel<<<1, 64, 0, a>>>(b->d_states, d_tab, nF, b->d_freq, b->d_fine);
        BK(hipGetLastError());
        const float beta = t.frame_jobs[0].beta;
        if ((st = dabgpu_ofdm_demod_frames(c, b->d_iq, (size_t)nF, b->d_freq, b->d_bits, b->d_corr, nullptr, nullptr, 0, 0, a))) return st;
        if ((st = dabgpu_ofdm_phase_update(c, b->d_corr, (size_t)nF, beta, b->d_total, b->d_fine, a))) return st;
        // display views: one more pass per frame that asked for them (a GUI polls one receiver)
        for (int j = 0; j < nF; j++) {
            const rx_bank_job& f = t.frame_jobs[(size_t)j];
            if (!f.want_views) continue;
            dabgpu_rx_member* m = f.m;
            const size_t fft_bytes = (size_t)(DABGPU_NB_FRAME_SYMBOLS + 1) * NFFT * 2 * sizeof(float), dq_bytes = (size_t)(DABGPU_NB_FRAME_SYMBOLS - 1) * DABGPU_NB_DATA_CARRIERS * 2 * sizeof(float);
            if (!m->d_fft) BK(hipMalloc((void**)&m->d_fft, fft_bytes));
            if (!m->d_dq) BK(hipMalloc((void**)&m->d_dq, dq_bytes));
            dabgpu_frame_session::slot& sl = m->ses->slots[f.gen % dabgpu_frame_session::R];
            if (sl.h_fft_cap < fft_bytes) { if (sl.h_fft) (void)hipHostFree(sl.h_fft); sl.h_fft = nullptr; sl.h_fft_cap = 0; BK(hipHostMalloc((void**)&sl.h_fft, fft_bytes, hipHostMallocDefault)); sl.h_fft_cap = fft_bytes; }
            if (sl.h_dq_cap < dq_bytes) { if (sl.h_dq) (void)hipHostFree(sl.h_dq); sl.h_dq = nullptr; sl.h_dq_cap = 0; BK(hipHostMalloc((void**)&sl.h_dq, dq_bytes, hipHostMallocDefault)); sl.h_dq_cap = dq_bytes; }
            // (into a scratch row of the batch: the soft bits of this pass are the ones the batched pass wrote)
            if ((st = dabgpu_ofdm_demod_frames(c, b->d_iq + (size_t)j * FRAME_SAMPLES * 2, 1, b->d_freq + j, b->d_bits + (size_t)j * FRAME_BITS, b->d_corr + (size_t)j * DABGPU_NB_FRAME_SYMBOLS * 2, m->d_fft, m->d_dq, 0, 0, a))) return st;
            BK(hipMemcpyAsync(sl.h_fft, m->d_fft, fft_bytes, hipMemcpyDeviceToHost, a));
            BK(hipMemcpyAsync(sl.h_dq, m->d_dq, dq_bytes, hipMemcpyDeviceToHost, a));
        }
        // the ring slot frame g + 4 of a member goes to is read by the decode of its frame g (5 frames = 16 CIFs + the frame's own 4): a member has
        // one frame per tick at most, so the decode of tick T - 4 is the youngest that may still read what this tick overwrites
        if (tick_no >= 4) BK(hipStreamWaitEvent(a, b->ticks[(tick_no - 4) % TICKS].ev_done, 0));
        bank_scatter_kernel<<<dim3(8, (unsigned)nF), 256, 0, a>>>(b->d_bits, b->d_hist, d_tab, b->d_fine, b->d_states);
        BK(hipGetLastError());
        BK(hipEventRecord(t.ev_demod, a));
        frames_enqueued = true;
    }
    // ---- synchronisers: behind the frames' fine-frequency updates, in front of the decode's launches and the bulky copies back ----
    if (nS) {
        int lo = MAXM, up = -1;
        for (const auto& j : t.sync_jobs) { lo = j.m->slot < lo ? j.m->slot : lo; up = j.m->slot > up ? j.m->slot : up; }
        // (the members copied their PRS slots into the bank's pinned array when they posted: one upload of the range that holds this round's)
        BK(hipMemcpyAsync(b->d_prs + (size_t)lo * NFFT * 2, b->h_prs + (size_t)lo * NFFT * 2, (size_t)(up - lo + 1) * NFFT * 2 * sizeof(float), hipMemcpyHostToDevice, a));
        const dabgpu_sync_cfg& cfg = t.sync_jobs[0].cfg;
        const bool coarse = cfg.is_coarse_freq_correction != 0;
        const dabgpu_mode_tables& mode1 = c->modes[1];
        BK(dabgpu_launch_sync(b->d_prs, NFFT, t.n_ens, &cfg, b->d_states, b->d_imp, coarse ? b->d_frq : nullptr, c->d_tw, mode1.prs, mode1.prs_time_ref, d_tab->sync_active, 1, a));
        BK(hipMemcpyAsync(t.h_states, b->d_states, (size_t)t.n_ens * sizeof(dabgpu_sync_state), hipMemcpyDeviceToHost, a));
        BK(hipMemcpyAsync(t.h_imp, b->d_imp, (size_t)t.n_ens * NFFT * sizeof(float), hipMemcpyDeviceToHost, a));
        if (coarse) BK(hipMemcpyAsync(t.h_frq, b->d_frq, (size_t)t.n_ens * NFFT * sizeof(float), hipMemcpyDeviceToHost, a));
    }
    BK(hipEventRecord(t.ev_sync, a));
    // ---- decode (stream B): enqueued behind the synchronisers -- its ~8 runtime calls used to sit in front of the synchroniser launch every reader waits for ----
    if (frames_enqueued) {
        const size_t n_sub = t.subs.size();
        if (t.fic || n_sub) {
            const size_t need = out_bytes((size_t)t.n_ens, n_sub, t.cif_out);
            if (b->d_out_cap < need) {
                BK(hipStreamSynchronize(q));
                if (b->d_out) (void)hipFree(b->d_out);
                b->d_out = nullptr; b->d_out_cap = 0;
                BK(hipMalloc((void**)&b->d_out, need));
                b->d_out_cap = need;
            }
            if (t.h_out_cap < need) {
                if (t.h_out) (void)hipHostFree(t.h_out);
                t.h_out = nullptr; t.h_out_cap = 0;
                BK(hipHostMalloc((void**)&t.h_out, need, hipHostMallocDefault));
                t.h_out_cap = need;
            }
            const out_ptrs o = out_layout(b->d_out, (size_t)t.n_ens, n_sub, t.cif_out);
            BK(hipStreamWaitEvent(q, t.ev_demod, 0));
            const int tie = t.frame_jobs[0].tie;
            if (n_sub) {
                if (t.fic) st = dabgpu_decode_ring_layout(c, b->d_hist, (size_t)t.n_ens, (size_t)H * FRAME_BITS, H, d_tab->newest, t.subs.data(), (int)n_sub, o.fib, o.fres, o.msc,
                                                         (size_t)4 * t.cif_out, o.mres, tie, DABGPU_BITS_NATURAL, q);
                else st = dabgpu_msc_decode_ring(c, b->d_hist, (size_t)t.n_ens, (size_t)H * FRAME_BITS, H, d_tab->newest, t.subs.data(), (int)n_sub, o.msc, (size_t)4 * t.cif_out, o.mres, tie, q);
            } else {
                st = dabgpu_fic_decode_ring(c, b->d_hist, (size_t)t.n_ens, (size_t)H * FRAME_BITS, d_tab->newest, o.fib, o.fres, tie, q);
            }
            if (st) return st;
            BK(hipMemcpyAsync(t.h_out, b->d_out, need, hipMemcpyDeviceToHost, q));
            t.decoded = true;
        }
    }
    if (frames_enqueued) {
        // the soft bits go straight to the page-locked buffer of the member's result slot (one copy per frame: what the delivery thread hands to the
        // observers is that buffer -- a compact copy per round plus a 230 KB memcpy per frame on the completer thread capped the bank at ~15 k frames/s)
        for (int j = 0; j < nF; j++) {
            const rx_bank_job& f = t.frame_jobs[(size_t)j];
            BK(hipMemcpyAsync(f.m->ses->slots[f.gen % dabgpu_frame_session::R].h_bits, b->d_bits + (size_t)j * FRAME_BITS, FRAME_BITS, hipMemcpyDeviceToHost, a));
        }
        BK(hipMemcpyAsync(t.h_scal, b->d_fine, (size_t)(MAXM + nF) * sizeof(float), hipMemcpyDeviceToHost, a));      // fine[0..nF) ... total[0..nF)
        BK(hipEventRecord(t.ev_copied, a));
    }
    BK(hipEventRecord(t.ev_done, q));
    return DABGPU_OK;
}

void worker_main(dabgpu_rx_bank* b) {
    pthread_setname_np(pthread_self(), "dabgpu-bank");
    (void)hipSetDevice(b->device);
    for (;;) {
        std::unique_lock<std::mutex> lock(b->mu);
        const double ti0 = b->profile ? bank_now_us() : 0.0;
        b->cv_jobs.wait(lock, [b] { return b->stop || !b->jobs.empty(); });
        if (b->profile && b->n_ticks) b->p_worker_idle_us += bank_now_us() - ti0;       // (not the wait for the very first job: the members are still being constructed)
        if (b->stop && b->jobs.empty()) return;
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
            for (int spin = 0; spin < 4 && !follows(); spin++) b->cv_jobs.wait_for(lock, std::chrono::microseconds(50), follows);
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
            if (b->refs > 1 && !all_in()) b->cv_jobs.wait_for(lock, std::chrono::microseconds(b->gather_us), all_in);
        }
        // Rounds are not enqueued ahead of the device: a round takes what is queued when it is formed, and with a deep queue of rounds under way every
        // job that arrives meanwhile becomes a small round of its own at the END of that queue -- many small rounds, each paying the fixed costs, each
        // member waiting for all of them (measured at 32 members: 4 frames per round, 8 rounds deep, 3 ms from posting a synchroniser to its record).
        // At most `max_rounds` are under way; what arrives while they run forms the next one, whose size so follows the load (group commit).
        b->cv_ticks.wait(lock, [b] { return b->n_ticks - b->n_handed < (uint64_t)b->max_rounds; });
        const uint64_t tick_no = b->n_ticks;
        rx_bank_tick& t = b->ticks[tick_no % TICKS];
        b->cv_ticks.wait(lock, [&] { return !t.busy; });                  // (the completer hands ticks out in order: at most TICKS are under way)
        t.sync_jobs.clear(); t.frame_jobs.clear();
        int taken[MAXM] = {0};                                             // 0 nothing yet, 1 its frame is in (its next synchroniser may follow), 2 closed
        std::vector<rx_bank_job> resets;
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
            else resets.push_back(*it);
            it = b->jobs.erase(it);
        }
        t.subs = b->subs; t.sub_off = b->sub_off; t.sub_n = b->sub_n; t.cif_out = b->cif_out; t.fic = b->fic;
        t.busy = true;
        b->n_ticks = tick_no + 1;
        lock.unlock();
        int st = DABGPU_OK;
        for (const auto& r : resets) {                                     // :277-289, behind everything enqueued for the member so far
            const int e = dabgpu_check_hip(hipMemsetAsync(b->d_states + r.m->slot, 0, sizeof(dabgpu_sync_state), b->a), "hipMemsetAsync(bank reset)");
            if (e && !st) st = e;
        }
        const double te0 = b->profile ? bank_now_us() : 0.0;
        if (!st) st = enqueue_tick(b, t, tick_no);
        if (b->profile) { b->p_enqueue_us += bank_now_us() - te0; b->p_sync_jobs += t.sync_jobs.size(); b->p_frame_jobs += t.frame_jobs.size(); b->p_ticks_with_frames += t.frame_jobs.empty() ? 0 : 1; }
        lock.lock();
        t.status = st;
        for (const auto& j : t.sync_jobs) j.m->sync_state = 2;
        for (const auto& r : resets) { r.m->jobs_in_flight--; r.m->cv.notify_all(); }
        lock.unlock();
        b->cv_done.notify_all();                                           // (the two completers)
    }
}

// The synchronisers' records, round by round: the readers wait for them (they cannot finish buffering the frame before), so they do not queue
// behind the decode of the same or an earlier round
void sync_completer_main(dabgpu_rx_bank* b) {
    pthread_setname_np(pthread_self(), "dabgpu-bk-sync");
    (void)hipSetDevice(b->device);
    for (;;) {
        std::unique_lock<std::mutex> lock(b->mu);
        b->cv_done.wait(lock, [b] { return (b->stop && b->n_sync_handed == b->n_ticks) || (b->n_sync_handed < b->n_ticks && b->ticks[b->n_sync_handed % TICKS].status != -1); });
        if (b->n_sync_handed == b->n_ticks) return;
        rx_bank_tick& t = b->ticks[b->n_sync_handed % TICKS];
        lock.unlock();
        int st = t.status;
        const double tc0 = b->profile ? bank_now_us() : 0.0;
        if (!st && !t.sync_jobs.empty()) st = dabgpu_check_hip(hipEventSynchronize(t.ev_sync), "hipEventSynchronize(bank sync)");
        if (b->profile) b->p_wait_sync_us += bank_now_us() - tc0;
        lock.lock();
        for (const auto& j : t.sync_jobs) {
            dabgpu_rx_member* m = j.m;
            m->sync_status = st;
            if (!st) {
                m->sync_rec = t.h_states[m->slot];
                m->sync_coarse = j.cfg.is_coarse_freq_correction != 0;
                m->sync_imp.assign(t.h_imp + (size_t)m->slot * NFFT, t.h_imp + (size_t)(m->slot + 1) * NFFT);
                if (m->sync_coarse) m->sync_frq.assign(t.h_frq + (size_t)m->slot * NFFT, t.h_frq + (size_t)(m->slot + 1) * NFFT);
            }
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

// The frames, round by round: waits for the device, copies every frame's results to its member's result store, wakes the members, frees the round
void completer_main(dabgpu_rx_bank* b) {
    pthread_setname_np(pthread_self(), "dabgpu-bk-frm");
    (void)hipSetDevice(b->device);
    for (;;) {
        std::unique_lock<std::mutex> lock(b->mu);
        b->cv_done.wait(lock, [b] { return (b->stop && b->n_handed == b->n_ticks) || (b->n_handed < b->n_ticks && b->ticks[b->n_handed % TICKS].status != -1); });
        if (b->n_handed == b->n_ticks) return;
        rx_bank_tick& t = b->ticks[b->n_handed % TICKS];
        lock.unlock();
        int st = t.status;
        const double tc0 = b->profile ? bank_now_us() : 0.0;
        if (!t.frame_jobs.empty()) {
            if (!st) st = dabgpu_check_hip(hipEventSynchronize(t.ev_copied), "hipEventSynchronize(bank copies)");
            if (!st) st = dabgpu_check_hip(hipEventSynchronize(t.ev_done), "hipEventSynchronize(bank decode)");
            if (b->profile) b->p_wait_frames_us += bank_now_us() - tc0;
            const size_t n_sub = t.subs.size();
            const out_ptrs o = out_layout(t.h_out, (size_t)t.n_ens, n_sub, t.cif_out);
            for (size_t j = 0; j < t.frame_jobs.size(); j++) {
                const rx_bank_job& f = t.frame_jobs[j];
                dabgpu_rx_member* m = f.m;
                dabgpu_frame_session* s = m->ses;
                std::lock_guard<std::mutex> sg(s->mu);
                dabgpu_frame_session::slot& sl = s->slots[f.gen % dabgpu_frame_session::R];
                sl.gen = ~0ull;
                sl.fic = false; sl.subs.clear(); sl.sub_off.clear(); sl.sub_n.clear(); sl.cif_out = 0;
                if (!st && t.decoded) {
                    const size_t need = 4 * 96 + (4 + 4 * n_sub) * sizeof(dabgpu_codeword_result) + (size_t)4 * t.cif_out;
                    if (sl.h_block_cap < need) {
                        if (sl.h_block) (void)hipHostFree(sl.h_block);
                        sl.h_block = nullptr; sl.h_block_cap = 0;
                        if (hipHostMalloc((void**)&sl.h_block, need, hipHostMallocDefault) != hipSuccess) { st = DABGPU_ERR_HIP; dabgpu_set_error("bank: hipHostMalloc(result block)"); }
                        else sl.h_block_cap = need;
                    }
                    if (!st) {
                        sl.h_fib = sl.h_block;
                        sl.h_fres = reinterpret_cast<dabgpu_codeword_result*>(sl.h_block + 4 * 96);
                        sl.h_mres = sl.h_fres + 4;
                        sl.h_msc = reinterpret_cast<uint8_t*>(sl.h_mres + 4 * n_sub);
                        const size_t e = (size_t)m->slot;
                        if (t.fic) { memcpy(sl.h_fib, o.fib + e * 4 * 96, 4 * 96); memcpy(sl.h_fres, o.fres + e * 4, 4 * sizeof(dabgpu_codeword_result)); }
                        if (n_sub) { memcpy(sl.h_mres, o.mres + e * 4 * n_sub, 4 * n_sub * sizeof(dabgpu_codeword_result)); memcpy(sl.h_msc, o.msc + e * 4 * t.cif_out, (size_t)4 * t.cif_out); }
                        sl.fic = t.fic; sl.subs = t.subs; sl.sub_off = t.sub_off; sl.sub_n = t.sub_n; sl.cif_out = t.cif_out;
                    }
                }
                // (sl.h_bits: the round's device-to-host copy wrote it, enqueue_tick)
                if (!sl.h_aux && hipHostMalloc((void**)&sl.h_aux, 4 * sizeof(float), hipHostMallocDefault) != hipSuccess) { if (!st) { st = DABGPU_ERR_HIP; dabgpu_set_error("bank: hipHostMalloc(aux)"); } }
                if (sl.h_aux) { sl.h_aux[0] = t.h_scal[j]; sl.h_aux[1] = t.h_scal[MAXM + j]; }
                sl.pending = false;
                sl.gen = f.gen;
            }
            lock.lock();
            for (const auto& f : t.frame_jobs) {
                f.m->frame_status = st ? st : f.m->frame_status;
                f.m->done_gen = f.gen + 1;
                f.m->jobs_in_flight--;
                f.m->cv.notify_all();
            }
            lock.unlock();
            b->cv_done.notify_all();
        }
        // The upload streams are never waited for on the host while something is in flight on them (the members' stage events have long fired when they are
        // looked at), and the HIP runtime releases a queue's finished commands only when somebody does: without this, every frame left a copy command and
        // 1.5 markers behind (2.4 KB of heap per frame, pinned and device memory of their signals: tools/exp/leakhist.c, profiles/r06/ab_notes.md).  Every 32nd
        // round, on this thread (not the worker's): a wait for the few uploads in flight.
        if ((b->n_handed & 31) == 31) for (int k = 0; k < dabgpu_rx_bank::NUP; k++) (void)hipStreamSynchronize(b->up[k]);
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

void bank_free(dabgpu_rx_bank* b) {
    (void)hipSetDevice(b->device);
    if (b->a) (void)hipStreamSynchronize(b->a);
    if (b->ctx) (void)hipStreamSynchronize(b->ctx->stream);
    void* dev[] = {b->d_prs, b->d_iq, b->d_bits, b->d_hist, b->d_states, b->d_imp, b->d_frq, b->d_corr, b->d_freq, b->d_fine, b->d_tab, b->d_out};
    if (b->h_prs) (void)hipHostFree(b->h_prs);
    for (void* p : dev) if (p) (void)hipFree(p);
    for (auto& t : b->ticks) {
        void* host[] = {t.h_tab, t.h_states, t.h_imp, t.h_frq, t.h_scal, t.h_out};
        for (void* p : host) if (p) (void)hipHostFree(p);
        hipEvent_t evs[] = {t.ev_sync, t.ev_demod, t.ev_copied, t.ev_done};
        for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e);
    }
    if (b->a) (void)hipStreamDestroy(b->a);
    for (hipStream_t u : b->up) if (u) { (void)hipStreamSynchronize(u); (void)hipStreamDestroy(u); }
    for (hipEvent_t e : b->up_ev) if (e) (void)hipEventDestroy(e);
    if (b->ctx) dabgpu_destroy(b->ctx);
    delete b;
}
}  // namespace

// ---- what receiver.hip calls ----
int dabgpu_rx_bank_join(int device, float* const* h_stage, dabgpu_rx_member** out) {
    *out = nullptr;
    if (device < 0 || device >= 16) { dabgpu_set_error("receiver bank: device %d out of range", device); return DABGPU_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> g(g_banks_mu);
    dabgpu_rx_bank* b = g_banks[device];
    int st;
    if (!b) {
        b = new dabgpu_rx_bank();
        for (auto& t : b->ticks) t.status = -1;
        b->device = device;
        if (const char* e = std::getenv("DABGPU_BANK_PROFILE")) b->profile = std::atoi(e) != 0;
        if (const char* e = std::getenv("DABGPU_BANK_GATHER_US")) b->gather_us = std::atoi(e);
        if (const char* e = std::getenv("DABGPU_BANK_UPLOADS")) b->n_up = std::min((int)dabgpu_rx_bank::NUP, std::max(0, std::atoi(e)));
        if (const char* e = std::getenv("DABGPU_BANK_ROUNDS")) b->max_rounds = std::min(TICKS, std::max(1, std::atoi(e)));
        st = dabgpu_create(&b->ctx, device, nullptr, nullptr);
        if (!st) {
            int least = 0, greatest = 0;
            st = dabgpu_check_hip(hipDeviceGetStreamPriorityRange(&least, &greatest), "hipDeviceGetStreamPriorityRange");
            if (!st) st = dabgpu_check_hip(hipStreamCreateWithPriority(&b->a, hipStreamNonBlocking, greatest), "hipStreamCreateWithPriority(bank)");
        }
        if (!st) st = bank_alloc(b);
        if (st) { bank_free(b); return st; }
        b->worker = std::thread(worker_main, b);
        b->completer = std::thread(completer_main, b);
        b->sync_completer = std::thread(sync_completer_main, b);
        g_banks[device] = b;
        static bool registered = false;                                    // (the HIP runtime registered its own teardown earlier: this one runs before it)
        if (!registered) { registered = true; std::atexit(dabgpu_rx_bank_shutdown); }
    }
    (void)hipSetDevice(device);
    dabgpu_rx_member* m = new dabgpu_rx_member();
    m->bank = b;
    m->h_stage = h_stage;
    st = dabgpu_frame_session_create_store(&m->ses, b->ctx);
    for (int k = 0; k < 3 && !st; k++) st = dabgpu_check_hip(hipEventCreateWithFlags(&m->stage_ev[k], dabgpu_wait_event_flags(true)), "hipEventCreate(bank member)");
    if (!st) st = dabgpu_check_hip(hipMalloc((void**)&m->d_iq, (size_t)2 * FRAME_SAMPLES * 2 * sizeof(float)), "hipMalloc(bank member samples)");
    // the rounds copy a frame's soft bits straight into the result slot's page-locked buffer (the session frees them)
    for (int k = 0; k < dabgpu_frame_session::R && !st; k++)
        st = dabgpu_check_hip(hipHostMalloc((void**)&m->ses->slots[k].h_bits, FRAME_BITS, hipHostMallocDefault), "hipHostMalloc(bank member soft bits)");
    if (!st) {
        std::lock_guard<std::mutex> lock(b->mu);
        for (int k = 0; k < MAXM && m->slot < 0; k++) if (!b->members[k]) { b->members[k] = m; m->slot = k; }
        if (m->slot < 0) { dabgpu_set_error("receiver bank: more than %d receivers on one device", MAXM); st = DABGPU_ERR_INVALID_ARG; }
        else b->refs++;
    }
    if (!st) st = dabgpu_check_hip(hipMemsetAsync(b->d_states + m->slot, 0, sizeof(dabgpu_sync_state), b->a), "hipMemsetAsync(bank member state)");
    if (!st) st = dabgpu_check_hip(hipMemsetAsync(b->d_hist + (size_t)m->slot * H * FRAME_BITS, 0, (size_t)H * FRAME_BITS, b->a), "hipMemsetAsync(bank member history)");
    if (!st) st = dabgpu_check_hip(hipStreamSynchronize(b->a), "hipStreamSynchronize(bank member)");
    if (st) {
        if (m->slot >= 0) { std::lock_guard<std::mutex> lock(b->mu); b->members[m->slot] = nullptr; b->refs--; }
        for (hipEvent_t e : m->stage_ev) if (e) (void)hipEventDestroy(e);
        if (m->d_iq) (void)hipFree(m->d_iq);
        if (m->ses) dabgpu_frame_session_destroy(m->ses);
        delete m;
        return st;
    }
    *out = m;
    return DABGPU_OK;
}

void dabgpu_rx_bank_leave(dabgpu_rx_member* m) {
    if (!m) return;
    dabgpu_rx_bank* b = m->bank;
    {
        std::unique_lock<std::mutex> lock(b->mu);
        m->cv.wait(lock, [m] { return m->jobs_in_flight == 0; });
        b->members[m->slot] = nullptr;
        b->refs--;
    }
    (void)hipSetDevice(b->device);
    for (hipEvent_t e : m->stage_ev) if (e) (void)hipEventDestroy(e);
    if (m->d_iq) (void)hipFree(m->d_iq);
    if (m->d_fft) (void)hipFree(m->d_fft);
    if (m->d_dq) (void)hipFree(m->d_dq);
    dabgpu_frame_session_destroy(m->ses);
    delete m;
    // the bank itself stays for the life of the process (its threads are joined by dabgpu_rx_bank_shutdown, which the library's unload calls)
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

int dabgpu_rx_bank_reset(dabgpu_rx_member* m) {
    dabgpu_rx_bank* b = m->bank;
    { std::lock_guard<std::mutex> lock(b->mu); rx_bank_job j{}; j.kind = rx_bank_job::RESET; j.m = m; b->jobs.push_back(j); m->jobs_in_flight++; }
    b->cv_jobs.notify_one();
    return DABGPU_OK;
}

int dabgpu_rx_bank_post_sync(dabgpu_rx_member* m, const dabgpu_sync_cfg* cfg, int stage, size_t prs_sample) {
    dabgpu_rx_bank* b = m->bank;
    {
        std::lock_guard<std::mutex> lock(b->mu);
        if (m->sync_state != 0) { dabgpu_set_error("receiver_submit_sync: the previous record has not been collected (dabgpu_receiver_wait_sync)"); return DABGPU_ERR_INVALID_ARG; }
    }
    // the member's row of the bank's pinned PRS array is its own until the record has come back (one synchroniser at a time per member)
    memcpy(b->h_prs + (size_t)m->slot * NFFT * 2, m->h_stage[stage] + 2 * prs_sample, NFFT * 2 * sizeof(float));
    {
        std::lock_guard<std::mutex> lock(b->mu);
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
        if (m->next_gen >= m->done_gen + (uint64_t)(dabgpu_frame_session::R - 1)) {
            dabgpu_set_error("receiver_submit_frame: %d frames submitted and not yet collected (at most %d)", (int)(m->next_gen - m->done_gen), dabgpu_frame_session::R - 1);
            return DABGPU_ERR_NOT_READY;
        }
        gen = m->next_gen;                                                 // (only the member's own thread posts)
        n_up = b->n_up > 0 ? b->n_up : (b->refs <= 12 ? 1 : (int)dabgpu_rx_bank::NUP);
    }
    // The member uploads its frame itself, now: the samples cross PCIe while the rounds under way run, not inside the round that demodulates them
    // (32 frames of a round are 1 ms of PCIe in front of the round's synchronisers otherwise).  Half gen % 2 of the member's device buffer: frame g - 2,
    // which used it, was read by the gather of its round, and that round lies on stream A in front of the synchroniser whose record this frame
    // was cut with (a member's jobs run in posting order; the synchroniser of frame g is posted after frame g - 1).
    (void)hipSetDevice(b->device);
    float* d = m->d_iq + (size_t)(gen % 2) * FRAME_SAMPLES * 2;
    const int up_k = m->slot % n_up;
    hipStream_t u = b->up[up_k];
    int st = dabgpu_check_hip(hipMemcpyAsync(d, m->h_stage[stage] + 2 * frame_sample, FRAME_SAMPLES * 2 * sizeof(float), hipMemcpyHostToDevice, u), "hipMemcpyAsync(bank frame)");
    if (!st) st = dabgpu_check_hip(hipEventRecord(m->stage_ev[stage], u), "hipEventRecord(bank stage)");
    if (st) return st;
    {
        std::lock_guard<std::mutex> lock(b->mu);
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
    (void)hipSetDevice(b->device);
    const int st = dabgpu_check_hip(hipEventSynchronize(m->stage_ev[stage]), "hipEventSynchronize(bank stage)");
    { std::lock_guard<std::mutex> lock(b->mu); m->stage_state[stage] = 0; }
    return st;
}

int dabgpu_rx_bank_wait_frame(dabgpu_rx_member* m, uint64_t generation, dabgpu_receiver_frame* out) {
    dabgpu_rx_bank* b = m->bank;
    {
        std::unique_lock<std::mutex> lock(b->mu);
        if (generation >= m->next_gen) { dabgpu_set_error("receiver_wait_frame: generation %llu was never submitted", (unsigned long long)generation); return DABGPU_ERR_NOT_READY; }
        m->cv.wait(lock, [&] { return m->done_gen > generation; });
        if (m->frame_status) { dabgpu_set_error("receiver bank: the tick that carried the frame failed"); return m->frame_status; }
    }
    dabgpu_frame_session::slot& sl = m->ses->slots[generation % dabgpu_frame_session::R];
    if (sl.gen != generation) { dabgpu_set_error("receiver_wait_frame: generation %llu is gone", (unsigned long long)generation); return DABGPU_ERR_NOT_READY; }
    out->generation = generation;
    out->bits = sl.h_bits;
    out->n_bits = FRAME_BITS;
    out->freq_fine = sl.h_aux[0];
    out->total_phase = sl.h_aux[1];
    out->fft = sl.h_fft;
    out->dqpsk = sl.h_dq;
    return DABGPU_OK;
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
        if (b->profile && b->n_ticks)
            fprintf(stderr, "receiver bank (device %d): %llu rounds, %llu with frames; %.2f frames and %.2f synchronisers per round; per round us: enqueue %.1f, completer { wait sync %.1f, "
                            "wait frames %.1f, whole hand-out %.1f }; worker idle %.1f\n", b->device, (unsigned long long)b->n_ticks, (unsigned long long)b->p_ticks_with_frames,
                    (double)b->p_frame_jobs / (double)b->n_ticks, (double)b->p_sync_jobs / (double)b->n_ticks, b->p_enqueue_us / (double)b->n_ticks, b->p_wait_sync_us / (double)b->n_ticks,
                    b->p_wait_frames_us / (double)b->n_ticks, b->p_handout_us / (double)b->n_ticks, b->p_worker_idle_us / (double)b->n_ticks);
        bank_free(b);
        b = nullptr;
    }
}
