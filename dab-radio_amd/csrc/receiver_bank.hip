// receiver_bank.hip -- the receiver bank's DEVICE half: the work of a round on the device, behind the rx_bank_device interface of receiver_bank_sched.h
// (receiver_bank_sched.cpp is the host scheduling half: the job queue, the threads, round formation, the order of the hand-outs).
// Many receivers of one process behind ONE pair of device streams ("all code words of all ensembles in one launch",
// for the drop-in classes).  VERDICT r5 item 4b: N OFDM_Demod objects, each with a receiver pipeline of its own (receiver.hip: three streams, ~20
// runtime calls and ~12 small device operations per frame), saturated at 6.5-7.3 k frames/s whatever N -- the device front end's limit, ~1 % of what
// the batch entry points do.  A BANKED receiver (dabgpu_receiver_create with DABGPU_RX_BANKED) keeps the whole dabgpu_receiver_* interface, but its
// submit_* calls only POST a job; one worker thread per device takes what has been posted since its last round -- at most one job per receiver, in
// posting order -- and issues it as one TICK:
//   stream A   H2D of the posted PRS slots -> ONE ofdm_sync_kernel over the member slots (active mask) -> D2H of the records
//              H2D of the posted frames into a compact batch -> gather of the members' offsets -> ONE ofdm_demod_kernel (+ phase kernel) over the batch
//              -> scatter of the soft bits into the members' history rings and of the fine-frequency words into their device records -> D2H
//   stream B   ONE dabgpu_decode_ring_layout over the member rings (inactive members skipped) -> D2H of the result arrays
// and two more threads hand the finished ticks' results to the members, one the synchronisers' records, one the frames (their result slots are the frame
// session's, so FIC_Decoder / MSC_Decoder fetch exactly as from a private receiver).  No artificial wait: under load the ticks fill by themselves (while one is being enqueued the other
// receivers post), at low load a tick is one receiver's job.  Arithmetic, per-receiver ordering (frame k's fine-frequency update precedes frame
// k + 1's synchroniser) and every output are those of the private pipeline: the same kernels run on the same inputs
// (tests/test_gpu_cpp_mirror.py, tests/test_gpu_receiver.py run both forms).
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <stdio.h>
#include <string.h>
#include <time.h>
#include <vector>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "receiver_bank_sched.h"

namespace {
constexpr int MAXM = DABGPU_RX_BANK_MAX, H = dabgpu_frame_session::H, TICKS = RX_BANK_TICKS, NUP = RX_BANK_UPLOADS;
static_assert(RX_BANK_SLOTS == dabgpu_frame_session::R, "the scheduler's post_frame counts the session's result slots");
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

struct rx_member_device {
    float* d_iq = nullptr;                      // [2][frame]: the member uploads frame g to half g % 2 when it posts it (see upload)
    hipEvent_t stage_ev[3] = {nullptr, nullptr, nullptr};   // recorded behind the upload of the frame posted from that staging buffer
    // views (display buffers), allocated at first use
    float* d_fft = nullptr; float* d_dq = nullptr;
};

namespace {
struct rx_bank_tick {
    tick_table* h_tab = nullptr;                // pinned
    dabgpu_sync_state* h_states = nullptr;      // pinned [MAXM]
    float* h_imp = nullptr; float* h_frq = nullptr;   // pinned [MAXM][NFFT]
    float* h_scal = nullptr;                    // pinned [2][MAXM]: fine after the update | total phase
    uint8_t* h_out = nullptr; size_t h_out_cap = 0;   // pinned: decode outputs of the tick [n_ens] x (fib | fres | mres | msc)
    hipEvent_t ev_sync = nullptr, ev_demod = nullptr, ev_copied = nullptr, ev_done = nullptr;
    int n_ens = 0;                              // member slots covered by the decode
    bool decoded = false;
};

size_t out_bytes(size_t n_ens, size_t n_sub, size_t cif_out) {
    return n_ens * (4 * 96 + (4 + 4 * n_sub) * sizeof(dabgpu_codeword_result) + 4 * cif_out);
}
struct out_ptrs { uint8_t* fib; dabgpu_codeword_result* fres; dabgpu_codeword_result* mres; uint8_t* msc; };
out_ptrs out_layout(uint8_t* base, size_t n_ens, size_t n_sub) {
    out_ptrs p;
    p.fib = base;
    p.fres = reinterpret_cast<dabgpu_codeword_result*>(base + n_ens * 4 * 96);
    p.mres = p.fres + n_ens * 4;
    p.msc = reinterpret_cast<uint8_t*>(p.mres + n_ens * 4 * n_sub);
    return p;
}

#define BK(call) do { st = dabgpu_check_hip((call), #call); if (st) return st; } while (0)

struct hip_bank final : rx_bank_device {
    int device = 0;
    dabgpu_ctx* ctx = nullptr;                  // tables; its stream = stream B (decode), its scratch = the decoder's
    hipStream_t a = nullptr;
    hipStream_t up[NUP] = {nullptr, nullptr, nullptr};   // upload streams: the scheduler says which one a member's frame takes (DABGPU_BANK_UPLOADS)
    hipEvent_t up_ev[NUP] = {nullptr, nullptr, nullptr};
    float* d_prs = nullptr; float* d_iq = nullptr; int8_t* d_bits = nullptr; int8_t* d_hist = nullptr;
    dabgpu_sync_state* d_states = nullptr; float* d_imp = nullptr; float* d_frq = nullptr;
    float* d_corr = nullptr; float* d_freq = nullptr; float* d_fine = nullptr; float* d_total = nullptr;
    tick_table* d_tab = nullptr;                // [TICKS]
    uint8_t* d_out = nullptr; size_t d_out_cap = 0;
    rx_bank_tick ticks[TICKS];
    float* h_prs = nullptr;                     // pinned [MAXM][NFFT] c32: the members copy their PRS slot here when they post (ONE upload per round)

    int open();
    ~hip_bank() override;
    void bind_thread() override { (void)hipSetDevice(device); }
    float* prs_row(int slot) override { return h_prs + (size_t)slot * NFFT * 2; }
    int member_open(dabgpu_rx_member* m) override;
    void member_close(dabgpu_rx_member* m) override;
    int enqueue_tick(const rx_bank_round& r);
    int enqueue(const rx_bank_round& r) override;
    int wait_sync(const rx_bank_round& r) override { return dabgpu_check_hip(hipEventSynchronize(ticks[r.no % TICKS].ev_sync), "hipEventSynchronize(bank sync)"); }
    void hand_sync(const rx_bank_round& r, size_t k) override;
    int wait_frames(const rx_bank_round& r) override {
        const int st = dabgpu_check_hip(hipEventSynchronize(ticks[r.no % TICKS].ev_copied), "hipEventSynchronize(bank copies)");
        return st ? st : dabgpu_check_hip(hipEventSynchronize(ticks[r.no % TICKS].ev_done), "hipEventSynchronize(bank decode)");
    }
    int deliver_frame(const rx_bank_round& r, size_t j, int st) override;
    int upload(dabgpu_rx_member* m, int stage, size_t frame_sample, uint64_t gen, int up_k, const float** d) override;
    int wait_stage(dabgpu_rx_member* m, int stage) override {
        (void)hipSetDevice(device);
        return dabgpu_check_hip(hipEventSynchronize(m->dev->stage_ev[stage]), "hipEventSynchronize(bank stage)");
    }
    // The upload streams are never waited for on the host while something is in flight on them (the members' stage events have long fired when they are
    // looked at), and the HIP runtime releases a queue's finished commands only when somebody does: without this, every frame left a copy command and
    // 1.5 markers behind (2.4 KB of heap per frame, pinned and device memory of their signals: tools/exp/leakhist.c, profiles/r06/ab_notes.md).  The frames'
    // completer calls it every 32nd round: a wait for the few uploads in flight.
    void drain_uploads() override { for (int k = 0; k < NUP; k++) (void)hipStreamSynchronize(up[k]); }
    int fetch_frame(dabgpu_rx_member* m, uint64_t generation, dabgpu_receiver_frame* out) override;
};

int hip_bank::open() {
    int st;
    if ((st = dabgpu_create(&ctx, device, nullptr, nullptr))) return st;
    int least = 0, greatest = 0;
    if ((st = dabgpu_check_hip(hipDeviceGetStreamPriorityRange(&least, &greatest), "hipDeviceGetStreamPriorityRange"))) return st;
    if ((st = dabgpu_check_hip(hipStreamCreateWithPriority(&a, hipStreamNonBlocking, greatest), "hipStreamCreateWithPriority(bank)"))) return st;
    BK(hipMalloc((void**)&d_prs, (size_t)MAXM * NFFT * 2 * sizeof(float)));
    BK(hipMalloc((void**)&d_iq, (size_t)MAXM * FRAME_SAMPLES * 2 * sizeof(float)));
    BK(hipMalloc((void**)&d_bits, (size_t)MAXM * FRAME_BITS));
    BK(hipMalloc((void**)&d_hist, (size_t)MAXM * H * FRAME_BITS));
    BK(hipMemsetAsync(d_hist, 0, (size_t)MAXM * H * FRAME_BITS, a));          // (stream A, not the NULL stream; join() synchronises it)
    BK(hipMalloc((void**)&d_states, (size_t)MAXM * sizeof(dabgpu_sync_state)));
    BK(hipMemsetAsync(d_states, 0, (size_t)MAXM * sizeof(dabgpu_sync_state), a));
    BK(hipMalloc((void**)&d_imp, (size_t)MAXM * NFFT * sizeof(float)));
    BK(hipMalloc((void**)&d_frq, (size_t)MAXM * NFFT * sizeof(float)));
    BK(hipMalloc((void**)&d_corr, (size_t)MAXM * DABGPU_NB_FRAME_SYMBOLS * 2 * sizeof(float)));
    BK(hipMalloc((void**)&d_freq, (size_t)MAXM * sizeof(float)));
    BK(hipMalloc((void**)&d_fine, (size_t)2 * MAXM * sizeof(float)));            // [fine after the update | total phase]: one copy back per round
    d_total = d_fine + MAXM;
    BK(hipMalloc((void**)&d_tab, (size_t)TICKS * sizeof(tick_table)));
    BK(hipHostMalloc((void**)&h_prs, (size_t)MAXM * NFFT * 2 * sizeof(float), hipHostMallocDefault));
    for (int k = 0; k < NUP; k++) {
        BK(hipStreamCreateWithFlags(&up[k], hipStreamNonBlocking));
        BK(hipEventCreateWithFlags(&up_ev[k], dabgpu_wait_event_flags(true)));
    }
    for (auto& t : ticks) {
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
int hip_bank::enqueue_tick(const rx_bank_round& r) {
    int st;
    dabgpu_ctx* c = ctx;
    rx_bank_tick& t = ticks[r.no % TICKS];
    const uint64_t tick_no = r.no;
    hipStream_t q = c->stream;
    tick_table& tab = *t.h_tab;
    const int nS = (int)r.sync_jobs.size(), nF = (int)r.frame_jobs.size();
    int hi = -1;
    for (int k = 0; k < MAXM; k++) { tab.sync_active[k] = 0; tab.newest[k] = -1; tab.slot_of[k] = 0; tab.ring_of[k] = 0; tab.iq_of[k] = nullptr; }
    for (const auto& j : r.sync_jobs) { tab.sync_active[j.m->slot] = 1; if (j.m->slot > hi) hi = j.m->slot; }
    for (int j = 0; j < nF; j++) {
        const rx_bank_job& f = r.frame_jobs[(size_t)j];
        tab.slot_of[j] = f.m->slot; tab.ring_of[j] = (int)(f.gen % H); tab.iq_of[j] = f.d_iq;
        tab.newest[f.m->slot] = (int)(f.gen % H);
        if (f.m->slot > hi) hi = f.m->slot;
    }
    t.n_ens = hi + 1;
    tick_table* dtab = d_tab + (tick_no % TICKS);
    BK(hipMemcpyAsync(dtab, t.h_tab, sizeof(tick_table), hipMemcpyHostToDevice, a));
    // ---- frames ----
    t.decoded = false;
    bool frames_enqueued = false;
    if (nF) {
        // the uploads -- 1.5 MB per frame -- were enqueued by the members when they posted (on upload stream slot % NUP, BEFORE the job entered the queue):
        // an event recorded now on each of those streams lies behind them.  They crossed PCIe while the previous round ran and this one waited to be
        // formed; the round copies them (device to device, ~1 us each) into the compact batch the demodulation kernel reads.
        bool used[NUP] = {false, false, false};
        for (const auto& f : r.frame_jobs) used[f.up] = true;
        for (int k = 0; k < NUP; k++) if (used[k]) { BK(hipEventRecord(up_ev[k], up[k])); BK(hipStreamWaitEvent(a, up_ev[k], 0)); }
        bank_gather_iq_kernel<<<dim3(16, (unsigned)nF), 256, 0, a>>>(d_iq, dtab);
        BK(hipGetLastError());
        bank_gather_kernel<<<1, 64, 0, a>>>(d_states, dtab, nF, d_freq, d_fine);
        BK(hipGetLastError());
        const float beta = r.frame_jobs[0].beta;
        if ((st = dabgpu_ofdm_demod_frames(c, d_iq, (size_t)nF, d_freq, d_bits, d_corr, nullptr, nullptr, 0, 0, a))) return st;
        if ((st = dabgpu_ofdm_phase_update(c, d_corr, (size_t)nF, beta, d_total, d_fine, a))) return st;
        // display views: one more pass per frame that asked for them (a GUI polls one receiver)
        for (int j = 0; j < nF; j++) {
            const rx_bank_job& f = r.frame_jobs[(size_t)j];
            if (!f.want_views) continue;
            dabgpu_rx_member* m = f.m;
            const size_t fft_bytes = (size_t)(DABGPU_NB_FRAME_SYMBOLS + 1) * NFFT * 2 * sizeof(float), dq_bytes = (size_t)(DABGPU_NB_FRAME_SYMBOLS - 1) * DABGPU_NB_DATA_CARRIERS * 2 * sizeof(float);
            if (!m->dev->d_fft) BK(hipMalloc((void**)&m->dev->d_fft, fft_bytes));
            if (!m->dev->d_dq) BK(hipMalloc((void**)&m->dev->d_dq, dq_bytes));
            dabgpu_frame_session::slot& sl = m->ses->slots[f.gen % dabgpu_frame_session::R];
            if (sl.h_fft_cap < fft_bytes) { if (sl.h_fft) (void)hipHostFree(sl.h_fft); sl.h_fft = nullptr; sl.h_fft_cap = 0; BK(hipHostMalloc((void**)&sl.h_fft, fft_bytes, hipHostMallocDefault)); sl.h_fft_cap = fft_bytes; }
            if (sl.h_dq_cap < dq_bytes) { if (sl.h_dq) (void)hipHostFree(sl.h_dq); sl.h_dq = nullptr; sl.h_dq_cap = 0; BK(hipHostMalloc((void**)&sl.h_dq, dq_bytes, hipHostMallocDefault)); sl.h_dq_cap = dq_bytes; }
            // (into a scratch row of the batch: the soft bits of this pass are the ones the batched pass wrote)
            if ((st = dabgpu_ofdm_demod_frames(c, d_iq + (size_t)j * FRAME_SAMPLES * 2, 1, d_freq + j, d_bits + (size_t)j * FRAME_BITS, d_corr + (size_t)j * DABGPU_NB_FRAME_SYMBOLS * 2, m->dev->d_fft, m->dev->d_dq, 0, 0, a))) return st;
            BK(hipMemcpyAsync(sl.h_fft, m->dev->d_fft, fft_bytes, hipMemcpyDeviceToHost, a));
            BK(hipMemcpyAsync(sl.h_dq, m->dev->d_dq, dq_bytes, hipMemcpyDeviceToHost, a));
        }
        // the ring slot frame g + 4 of a member goes to is read by the decode of its frame g (5 frames = 16 CIFs + the frame's own 4): a member has
        // one frame per tick at most, so the decode of tick T - 4 is the youngest that may still read what this tick overwrites
        if (tick_no >= 4) BK(hipStreamWaitEvent(a, ticks[(tick_no - 4) % TICKS].ev_done, 0));
        bank_scatter_kernel<<<dim3(8, (unsigned)nF), 256, 0, a>>>(d_bits, d_hist, dtab, d_fine, d_states);
        BK(hipGetLastError());
        BK(hipEventRecord(t.ev_demod, a));
        frames_enqueued = true;
    }
    // ---- synchronisers: behind the frames' fine-frequency updates, in front of the decode's launches and the bulky copies back ----
    if (nS) {
        int lo = MAXM, up = -1;
        for (const auto& j : r.sync_jobs) { lo = j.m->slot < lo ? j.m->slot : lo; up = j.m->slot > up ? j.m->slot : up; }
        // (the members copied their PRS slots into the bank's pinned array when they posted: one upload of the range that holds this round's)
        BK(hipMemcpyAsync(d_prs + (size_t)lo * NFFT * 2, h_prs + (size_t)lo * NFFT * 2, (size_t)(up - lo + 1) * NFFT * 2 * sizeof(float), hipMemcpyHostToDevice, a));
        const dabgpu_sync_cfg& cfg = r.sync_jobs[0].cfg;
        const bool coarse = cfg.is_coarse_freq_correction != 0;
        if ((st = dabgpu_launch_sync(c, 1, d_prs, NFFT, t.n_ens, &cfg, d_states, d_imp, coarse ? d_frq : nullptr, dtab->sync_active, a))) return st;
        BK(hipMemcpyAsync(t.h_states, d_states, (size_t)t.n_ens * sizeof(dabgpu_sync_state), hipMemcpyDeviceToHost, a));
        BK(hipMemcpyAsync(t.h_imp, d_imp, (size_t)t.n_ens * NFFT * sizeof(float), hipMemcpyDeviceToHost, a));
        if (coarse) BK(hipMemcpyAsync(t.h_frq, d_frq, (size_t)t.n_ens * NFFT * sizeof(float), hipMemcpyDeviceToHost, a));
    }
    BK(hipEventRecord(t.ev_sync, a));
    // ---- decode (stream B): enqueued behind the synchronisers -- its ~8 runtime calls used to sit in front of the synchroniser launch every reader waits for ----
    if (frames_enqueued) {
        const size_t n_sub = r.subs.size();
        if (r.fic || n_sub) {
            const size_t need = out_bytes((size_t)t.n_ens, n_sub, r.cif_out);
            if (d_out_cap < need) {
                BK(hipStreamSynchronize(q));
                if (d_out) (void)hipFree(d_out);
                d_out = nullptr; d_out_cap = 0;
                BK(hipMalloc((void**)&d_out, need));
                d_out_cap = need;
            }
            if (t.h_out_cap < need) {
                if (t.h_out) (void)hipHostFree(t.h_out);
                t.h_out = nullptr; t.h_out_cap = 0;
                BK(hipHostMalloc((void**)&t.h_out, need, hipHostMallocDefault));
                t.h_out_cap = need;
            }
            const out_ptrs o = out_layout(d_out, (size_t)t.n_ens, n_sub);
            BK(hipStreamWaitEvent(q, t.ev_demod, 0));
            const int tie = r.frame_jobs[0].tie;
            if (n_sub) {
                if (r.fic) st = dabgpu_decode_ring_layout(c, d_hist, (size_t)t.n_ens, (size_t)H * FRAME_BITS, H, dtab->newest, r.subs.data(), (int)n_sub, o.fib, o.fres, o.msc,
                                                         (size_t)4 * r.cif_out, o.mres, tie, DABGPU_BITS_NATURAL, q);
                else st = dabgpu_msc_decode_ring(c, d_hist, (size_t)t.n_ens, (size_t)H * FRAME_BITS, H, dtab->newest, r.subs.data(), (int)n_sub, o.msc, (size_t)4 * r.cif_out, o.mres, tie, q);
            } else {
                st = dabgpu_fic_decode_ring(c, d_hist, (size_t)t.n_ens, (size_t)H * FRAME_BITS, dtab->newest, o.fib, o.fres, tie, q);
            }
            if (st) return st;
            BK(hipMemcpyAsync(t.h_out, d_out, need, hipMemcpyDeviceToHost, q));
            t.decoded = true;
        }
    }
    if (frames_enqueued) {
        // the soft bits go straight to the page-locked buffer of the member's result slot (one copy per frame: what the delivery thread hands to the
        // observers is that buffer -- a compact copy per round plus a 230 KB memcpy per frame on the completer thread capped the bank at ~15 k frames/s)
        for (int j = 0; j < nF; j++) {
            const rx_bank_job& f = r.frame_jobs[(size_t)j];
            BK(hipMemcpyAsync(f.m->ses->slots[f.gen % dabgpu_frame_session::R].h_bits, d_bits + (size_t)j * FRAME_BITS, FRAME_BITS, hipMemcpyDeviceToHost, a));
        }
        BK(hipMemcpyAsync(t.h_scal, d_fine, (size_t)(MAXM + nF) * sizeof(float), hipMemcpyDeviceToHost, a));      // fine[0..nF) ... total[0..nF)
        BK(hipEventRecord(t.ev_copied, a));
    }
    BK(hipEventRecord(t.ev_done, q));
    return DABGPU_OK;
}

int hip_bank::enqueue(const rx_bank_round& r) {
    int st = DABGPU_OK;
    for (const auto& j : r.resets) {                                       // :277-289, behind everything enqueued for the member so far
        const int e = dabgpu_check_hip(hipMemsetAsync(d_states + j.m->slot, 0, sizeof(dabgpu_sync_state), a), "hipMemsetAsync(bank reset)");
        if (e && !st) st = e;
    }
    return st ? st : enqueue_tick(r);
}

void hip_bank::hand_sync(const rx_bank_round& r, size_t k) {
    const rx_bank_tick& t = ticks[r.no % TICKS];
    dabgpu_rx_member* m = r.sync_jobs[k].m;
    m->sync_rec = t.h_states[m->slot];
    m->sync_coarse = r.sync_jobs[k].cfg.is_coarse_freq_correction != 0;
    m->sync_imp.assign(t.h_imp + (size_t)m->slot * NFFT, t.h_imp + (size_t)(m->slot + 1) * NFFT);
    if (m->sync_coarse) m->sync_frq.assign(t.h_frq + (size_t)m->slot * NFFT, t.h_frq + (size_t)(m->slot + 1) * NFFT);
}

// copies the frame's results out of the round's page-locked arrays into its member's result store
int hip_bank::deliver_frame(const rx_bank_round& r, size_t j, int st) {
    const rx_bank_tick& t = ticks[r.no % TICKS];
    const size_t n_sub = r.subs.size();
    const out_ptrs o = out_layout(t.h_out, (size_t)t.n_ens, n_sub);
    const rx_bank_job& f = r.frame_jobs[j];
    dabgpu_rx_member* m = f.m;
    dabgpu_frame_session* s = m->ses;
    std::lock_guard sg(s->mu);
    dabgpu_frame_session::slot& sl = s->slots[f.gen % dabgpu_frame_session::R];
    sl.gen = ~0ull;
    sl.fic = false; sl.subs.clear(); sl.sub_off.clear(); sl.sub_n.clear(); sl.cif_out = 0;
    if (!st && t.decoded) {
        const size_t need = 4 * 96 + (4 + 4 * n_sub) * sizeof(dabgpu_codeword_result) + (size_t)4 * r.cif_out;
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
            if (r.fic) { memcpy(sl.h_fib, o.fib + e * 4 * 96, 4 * 96); memcpy(sl.h_fres, o.fres + e * 4, 4 * sizeof(dabgpu_codeword_result)); }
            if (n_sub) { memcpy(sl.h_mres, o.mres + e * 4 * n_sub, 4 * n_sub * sizeof(dabgpu_codeword_result)); memcpy(sl.h_msc, o.msc + e * 4 * r.cif_out, (size_t)4 * r.cif_out); }
            sl.fic = r.fic; sl.subs = r.subs; sl.sub_off = r.sub_off; sl.sub_n = r.sub_n; sl.cif_out = r.cif_out;
        }
    }
    // (sl.h_bits: the round's device-to-host copy wrote it, enqueue_tick)
    if (!sl.h_aux && hipHostMalloc((void**)&sl.h_aux, 4 * sizeof(float), hipHostMallocDefault) != hipSuccess) { if (!st) { st = DABGPU_ERR_HIP; dabgpu_set_error("bank: hipHostMalloc(aux)"); } }
    if (sl.h_aux) { sl.h_aux[0] = t.h_scal[j]; sl.h_aux[1] = t.h_scal[MAXM + j]; }
    sl.pending = false;
    sl.gen = f.gen;
    return st;
}

// Half gen % 2 of the member's device buffer: frame g - 2, which used it, was read by the gather of its round, and that round lies on stream A in front
// of the synchroniser whose record this frame was cut with (a member's jobs run in posting order; the synchroniser of frame g is posted after frame g - 1).
int hip_bank::upload(dabgpu_rx_member* m, int stage, size_t frame_sample, uint64_t gen, int up_k, const float** d_out_iq) {
    (void)hipSetDevice(device);
    float* d = m->dev->d_iq + (size_t)(gen % 2) * FRAME_SAMPLES * 2;
    hipStream_t u = up[up_k];
    int st = dabgpu_check_hip(hipMemcpyAsync(d, m->h_stage[stage] + 2 * frame_sample, FRAME_SAMPLES * 2 * sizeof(float), hipMemcpyHostToDevice, u), "hipMemcpyAsync(bank frame)");
    if (!st) st = dabgpu_check_hip(hipEventRecord(m->dev->stage_ev[stage], u), "hipEventRecord(bank stage)");
    *d_out_iq = d;
    return st;
}

int hip_bank::fetch_frame(dabgpu_rx_member* m, uint64_t generation, dabgpu_receiver_frame* out) {
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

int hip_bank::member_open(dabgpu_rx_member* m) {
    (void)hipSetDevice(device);
    rx_member_device* d = m->dev = new rx_member_device();
    int st = dabgpu_frame_session_create_store(&m->ses, ctx);
    for (int k = 0; k < 3 && !st; k++) st = dabgpu_check_hip(hipEventCreateWithFlags(&d->stage_ev[k], dabgpu_wait_event_flags(true)), "hipEventCreate(bank member)");
    if (!st) st = dabgpu_check_hip(hipMalloc((void**)&d->d_iq, (size_t)2 * FRAME_SAMPLES * 2 * sizeof(float)), "hipMalloc(bank member samples)");
    // the rounds copy a frame's soft bits straight into the result slot's page-locked buffer (the session frees them)
    for (int k = 0; k < dabgpu_frame_session::R && !st; k++)
        st = dabgpu_check_hip(hipHostMalloc((void**)&m->ses->slots[k].h_bits, FRAME_BITS, hipHostMallocDefault), "hipHostMalloc(bank member soft bits)");
    if (!st) st = dabgpu_check_hip(hipMemsetAsync(d_states + m->slot, 0, sizeof(dabgpu_sync_state), a), "hipMemsetAsync(bank member state)");
    if (!st) st = dabgpu_check_hip(hipMemsetAsync(d_hist + (size_t)m->slot * H * FRAME_BITS, 0, (size_t)H * FRAME_BITS, a), "hipMemsetAsync(bank member history)");
    if (!st) st = dabgpu_check_hip(hipStreamSynchronize(a), "hipStreamSynchronize(bank member)");
    if (st) member_close(m);
    return st;
}

void hip_bank::member_close(dabgpu_rx_member* m) {
    (void)hipSetDevice(device);
    for (hipEvent_t e : m->dev->stage_ev) if (e) (void)hipEventDestroy(e);
    void* dev[] = {m->dev->d_iq, m->dev->d_fft, m->dev->d_dq};
    for (void* p : dev) if (p) (void)hipFree(p);
    if (m->ses) dabgpu_frame_session_destroy(m->ses);
    delete m->dev;
}

hip_bank::~hip_bank() {
    (void)hipSetDevice(device);
    if (a) (void)hipStreamSynchronize(a);
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    void* dev[] = {d_prs, d_iq, d_bits, d_hist, d_states, d_imp, d_frq, d_corr, d_freq, d_fine, d_tab, d_out};
    if (h_prs) (void)hipHostFree(h_prs);
    for (void* p : dev) if (p) (void)hipFree(p);
    for (auto& t : ticks) {
        void* host[] = {t.h_tab, t.h_states, t.h_imp, t.h_frq, t.h_scal, t.h_out};
        for (void* p : host) if (p) (void)hipHostFree(p);
        hipEvent_t evs[] = {t.ev_sync, t.ev_demod, t.ev_copied, t.ev_done};
        for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e);
    }
    if (a) (void)hipStreamDestroy(a);
    for (hipStream_t u : up) if (u) { (void)hipStreamSynchronize(u); (void)hipStreamDestroy(u); }
    for (hipEvent_t e : up_ev) if (e) (void)hipEventDestroy(e);
    if (ctx) dabgpu_destroy(ctx);
}
}  // namespace

int dabgpu_rx_bank_device_open(int device, rx_bank_device** out) {
    hip_bank* b = new hip_bank();
    b->device = device;
    const int st = b->open();
    if (st) { delete b; return st; }
    *out = b;
    return DABGPU_OK;
}
