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
#include <memory>
#include <new>
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
    dabgpu::DeviceBuffer<float> d_iq;           // [RX_BANK_IQ_FRAMES][frame]: the member uploads frame g to buffer g % RX_BANK_IQ_FRAMES when it posts it (see upload)
    dabgpu::Event stage_ev[3];                  // recorded behind the upload of the frame posted from that staging buffer
    // views (display buffers), allocated at first use
    dabgpu::DeviceBuffer<float> d_fft, d_dq;
};

namespace {
struct rx_bank_tick {
    dabgpu::PinnedBuffer<tick_table> h_tab;
    dabgpu::PinnedBuffer<dabgpu_sync_state> h_states;   // [MAXM]
    dabgpu::PinnedBuffer<float> h_imp, h_frq;           // [MAXM][NFFT]
    dabgpu::PinnedBuffer<float> h_scal;                 // [2][MAXM]: fine after the update | total phase
    dabgpu::PinnedBuffer<uint8_t> h_out;                // decode outputs of the tick [n_ens] x (fib | fres | mres | msc), grow-only
    dabgpu::Event ev_sync, ev_demod, ev_copied, ev_done;
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
    // tables; its stream = stream B (decode), its scratch = the decoder's.  The first member: destroyed after everything below
    std::unique_ptr<dabgpu_ctx, void (*)(dabgpu_ctx*)> ctx{nullptr, dabgpu_destroy};
    dabgpu::Stream a;
    dabgpu::Stream up[NUP];                     // upload streams: the scheduler says which one a member's frame takes (DABGPU_BANK_UPLOADS)
    dabgpu::Event up_ev[NUP];
    dabgpu::DeviceBuffer<float> d_prs, d_iq; dabgpu::DeviceBuffer<int8_t> d_bits, d_hist;
    dabgpu::DeviceBuffer<dabgpu_sync_state> d_states; dabgpu::DeviceBuffer<float> d_imp, d_frq;
    dabgpu::DeviceBuffer<float> d_corr, d_freq, d_fine; float* d_total = nullptr;      // (d_total: into d_fine)
    dabgpu::DeviceBuffer<tick_table> d_tab;     // [TICKS]
    dabgpu::DeviceBuffer<uint8_t> d_out;        // grow-only
    rx_bank_tick ticks[TICKS];
    dabgpu::PinnedBuffer<float> h_prs;          // [MAXM][NFFT] c32: the members copy their PRS slot here when they post (ONE upload per round)

    int open();
    ~hip_bank() override;
    void bind_thread() override { (void)hipSetDevice(device); }
    float* prs_row(int slot) override { return h_prs.get() + (size_t)slot * NFFT * 2; }
    int member_open(dabgpu_rx_member* m) override;
    void member_close(dabgpu_rx_member* m) override;
    int enqueue_tick(const rx_bank_round& r);
    int enqueue(const rx_bank_round& r) override;
    int wait_sync(const rx_bank_round& r) override { return dabgpu_check_hip(hipEventSynchronize(ticks[r.no % TICKS].ev_sync.get()), "hipEventSynchronize(bank sync)"); }
    void hand_sync(const rx_bank_round& r, size_t k) override;
    int wait_frames(const rx_bank_round& r) override {
        const int st = dabgpu_check_hip(hipEventSynchronize(ticks[r.no % TICKS].ev_copied.get()), "hipEventSynchronize(bank copies)");
        return st ? st : dabgpu_check_hip(hipEventSynchronize(ticks[r.no % TICKS].ev_done.get()), "hipEventSynchronize(bank decode)");
    }
    int deliver_frame(const rx_bank_round& r, size_t j, int st) override;
    int upload(dabgpu_rx_member* m, int stage, size_t frame_sample, uint64_t gen, int up_k, const float** d) override;
    int wait_stage(dabgpu_rx_member* m, int stage) override {
        (void)hipSetDevice(device);
        return dabgpu_check_hip(hipEventSynchronize(m->dev->stage_ev[stage].get()), "hipEventSynchronize(bank stage)");
    }
    // The upload streams are never waited for on the host while something is in flight on them (the members' stage events have long fired when they are
    // looked at), and the HIP runtime releases a queue's finished commands only when somebody does: without this, every frame left a copy command and
    // 1.5 markers behind (2.4 KB of heap per frame, pinned and device memory of their signals: tools/exp/leakhist.c, profiles/r06/ab_notes.md).  The frames'
    // completer calls it every 32nd round: a wait for the few uploads in flight.
    void drain_uploads() override { for (int k = 0; k < NUP; k++) (void)hipStreamSynchronize(up[k].get()); }
    int fetch_frame(dabgpu_rx_member* m, uint64_t generation, dabgpu_receiver_frame* out) override;
};

int hip_bank::open() {
    int st;
    dabgpu_ctx* c = nullptr;
    if ((st = dabgpu_create(&c, device, nullptr, nullptr))) return st;
    ctx.reset(c);
    int least = 0, greatest = 0;
    if ((st = dabgpu_check_hip(hipDeviceGetStreamPriorityRange(&least, &greatest), "hipDeviceGetStreamPriorityRange"))) return st;
    if ((st = a.create(hipStreamNonBlocking, greatest, "hipStreamCreateWithPriority(bank)"))) return st;
    // (the labels: the calls as they were written when these messages were first seen)
    if ((st = d_prs.alloc((size_t)MAXM * NFFT * 2, "hipMalloc((void**)&d_prs, (size_t)MAXM * NFFT * 2 * sizeof(float))"))) return st;
    if ((st = d_iq.alloc((size_t)MAXM * FRAME_SAMPLES * 2, "hipMalloc((void**)&d_iq, (size_t)MAXM * FRAME_SAMPLES * 2 * sizeof(float))"))) return st;
    if ((st = d_bits.alloc((size_t)MAXM * FRAME_BITS, "hipMalloc((void**)&d_bits, (size_t)MAXM * FRAME_BITS)"))) return st;
    if ((st = d_hist.alloc((size_t)MAXM * H * FRAME_BITS, "hipMalloc((void**)&d_hist, (size_t)MAXM * H * FRAME_BITS)"))) return st;
    BK(hipMemsetAsync(d_hist.get(), 0, (size_t)MAXM * H * FRAME_BITS, a.get()));          // (stream A, not the NULL stream; join() synchronises it)
    if ((st = d_states.alloc((size_t)MAXM, "hipMalloc((void**)&d_states, (size_t)MAXM * sizeof(dabgpu_sync_state))"))) return st;
    BK(hipMemsetAsync(d_states.get(), 0, (size_t)MAXM * sizeof(dabgpu_sync_state), a.get()));
    if ((st = d_imp.alloc((size_t)MAXM * NFFT, "hipMalloc((void**)&d_imp, (size_t)MAXM * NFFT * sizeof(float))"))) return st;
    if ((st = d_frq.alloc((size_t)MAXM * NFFT, "hipMalloc((void**)&d_frq, (size_t)MAXM * NFFT * sizeof(float))"))) return st;
    if ((st = d_corr.alloc((size_t)MAXM * DABGPU_NB_FRAME_SYMBOLS * 2, "hipMalloc((void**)&d_corr, (size_t)MAXM * DABGPU_NB_FRAME_SYMBOLS * 2 * sizeof(float))"))) return st;
    if ((st = d_freq.alloc((size_t)MAXM, "hipMalloc((void**)&d_freq, (size_t)MAXM * sizeof(float))"))) return st;
    // [fine after the update | total phase]: one copy back per round
    if ((st = d_fine.alloc((size_t)2 * MAXM, "hipMalloc((void**)&d_fine, (size_t)2 * MAXM * sizeof(float))"))) return st;
    d_total = d_fine.get() + MAXM;
    if ((st = d_tab.alloc((size_t)TICKS, "hipMalloc((void**)&d_tab, (size_t)TICKS * sizeof(tick_table))"))) return st;
    if ((st = h_prs.alloc((size_t)MAXM * NFFT * 2, "hipHostMalloc((void**)&h_prs, (size_t)MAXM * NFFT * 2 * sizeof(float), hipHostMallocDefault)"))) return st;
    const unsigned wait_flags = dabgpu_wait_event_flags(true);
    for (int k = 0; k < NUP; k++) {
        if ((st = up[k].create(hipStreamNonBlocking, "hipStreamCreateWithFlags(&up[k], hipStreamNonBlocking)"))) return st;
        if ((st = up_ev[k].create(wait_flags, "hipEventCreateWithFlags(&up_ev[k], dabgpu_wait_event_flags(true))"))) return st;
    }
    for (auto& t : ticks) {
        if ((st = t.h_tab.alloc(1, "hipHostMalloc((void**)&t.h_tab, sizeof(tick_table), hipHostMallocDefault)"))) return st;
        if ((st = t.h_states.alloc((size_t)MAXM, "hipHostMalloc((void**)&t.h_states, (size_t)MAXM * sizeof(dabgpu_sync_state), hipHostMallocDefault)"))) return st;
        if ((st = t.h_imp.alloc((size_t)MAXM * NFFT, "hipHostMalloc((void**)&t.h_imp, (size_t)MAXM * NFFT * sizeof(float), hipHostMallocDefault)"))) return st;
        if ((st = t.h_frq.alloc((size_t)MAXM * NFFT, "hipHostMalloc((void**)&t.h_frq, (size_t)MAXM * NFFT * sizeof(float), hipHostMallocDefault)"))) return st;
        if ((st = t.h_scal.alloc((size_t)2 * MAXM, "hipHostMalloc((void**)&t.h_scal, (size_t)2 * MAXM * sizeof(float), hipHostMallocDefault)"))) return st;
        if ((st = t.ev_sync.create(wait_flags, "hipEventCreateWithFlags(&t.ev_sync, dabgpu_wait_event_flags(true))"))) return st;
        if ((st = t.ev_demod.create(wait_flags, "hipEventCreateWithFlags(&t.ev_demod, dabgpu_wait_event_flags(true))"))) return st;
        if ((st = t.ev_copied.create(wait_flags, "hipEventCreateWithFlags(&t.ev_copied, dabgpu_wait_event_flags(true))"))) return st;
        if ((st = t.ev_done.create(wait_flags, "hipEventCreateWithFlags(&t.ev_done, dabgpu_wait_event_flags(true))"))) return st;
    }
    return DABGPU_OK;
}

// one tick on the two streams; returns the first failure (the tick's jobs are then completed with it)
int hip_bank::enqueue_tick(const rx_bank_round& r) {
    int st;
    dabgpu_ctx* c = ctx.get();
    rx_bank_tick& t = ticks[r.no % TICKS];
    const uint64_t tick_no = r.no;
    hipStream_t q = c->stream;
    tick_table& tab = *t.h_tab.get();
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
    tick_table* dtab = d_tab.get() + (tick_no % TICKS);
    BK(hipMemcpyAsync(dtab, t.h_tab.get(), sizeof(tick_table), hipMemcpyHostToDevice, a.get()));
    // ---- frames ----
    t.decoded = false;
    bool frames_enqueued = false;
    if (nF) {
        // the uploads -- 1.5 MB per frame -- were enqueued by the members when they posted (on upload stream slot % NUP, BEFORE the job entered the queue):
        // an event recorded now on each of those streams lies behind them.  They crossed PCIe while the previous round ran and this one waited to be
        // formed; the round copies them (device to device, ~1 us each) into the compact batch the demodulation kernel reads.
        bool used[NUP] = {false, false, false};
        for (const auto& f : r.frame_jobs) used[f.up] = true;
        for (int k = 0; k < NUP; k++) if (used[k]) { BK(hipEventRecord(up_ev[k].get(), up[k].get())); BK(hipStreamWaitEvent(a.get(), up_ev[k].get(), 0)); }
        bank_gather_iq_kernel<<<dim3(16, (unsigned)nF), 256, 0, a.get()>>>(d_iq.get(), dtab);
        BK(hipGetLastError());
        bank_gather_kernel<<<1, 64, 0, a.get()>>>(d_states.get(), dtab, nF, d_freq.get(), d_fine.get());
        BK(hipGetLastError());
        const float beta = r.frame_jobs[0].beta;
        if ((st = dabgpu_ofdm_demod_frames(c, d_iq.get(), (size_t)nF, d_freq.get(), d_bits.get(), d_corr.get(), nullptr, nullptr, 0, 0, a.get()))) return st;
        if ((st = dabgpu_ofdm_phase_update(c, d_corr.get(), (size_t)nF, beta, d_total, d_fine.get(), a.get()))) return st;
        // display views: one more pass per frame that asked for them (a GUI polls one receiver)
        for (int j = 0; j < nF; j++) {
            const rx_bank_job& f = r.frame_jobs[(size_t)j];
            if (!f.want_views) continue;
            dabgpu_rx_member* m = f.m;
            const size_t fft_bytes = (size_t)(DABGPU_NB_FRAME_SYMBOLS + 1) * NFFT * 2 * sizeof(float), dq_bytes = (size_t)(DABGPU_NB_FRAME_SYMBOLS - 1) * DABGPU_NB_DATA_CARRIERS * 2 * sizeof(float);
            rx_member_device& md = *m->dev;
            if (!md.d_fft && (st = md.d_fft.alloc(fft_bytes / sizeof(float), "hipMalloc((void**)&m->dev->d_fft, fft_bytes)"))) return st;
            if (!md.d_dq && (st = md.d_dq.alloc(dq_bytes / sizeof(float), "hipMalloc((void**)&m->dev->d_dq, dq_bytes)"))) return st;
            dabgpu_frame_session::slot& sl = m->ses->slots[f.gen % dabgpu_frame_session::R];
            // (no wait: the slot's previous frame was delivered before the scheduler let this one be posted)
            if ((st = sl.h_fft.regrow(fft_bytes / sizeof(float), "hipHostMalloc((void**)&sl.h_fft, fft_bytes, hipHostMallocDefault)"))) return st;
            if ((st = sl.h_dq.regrow(dq_bytes / sizeof(float), "hipHostMalloc((void**)&sl.h_dq, dq_bytes, hipHostMallocDefault)"))) return st;
            // (into a scratch row of the batch: the soft bits of this pass are the ones the batched pass wrote)
            if ((st = dabgpu_ofdm_demod_frames(c, d_iq.get() + (size_t)j * FRAME_SAMPLES * 2, 1, d_freq.get() + j, d_bits.get() + (size_t)j * FRAME_BITS, d_corr.get() + (size_t)j * DABGPU_NB_FRAME_SYMBOLS * 2, md.d_fft.get(), md.d_dq.get(), 0, 0, a.get()))) return st;
            BK(hipMemcpyAsync(sl.h_fft.get(), md.d_fft.get(), fft_bytes, hipMemcpyDeviceToHost, a.get()));
            BK(hipMemcpyAsync(sl.h_dq.get(), md.d_dq.get(), dq_bytes, hipMemcpyDeviceToHost, a.get()));
        }
        // the ring slot frame g + 4 of a member goes to is read by the decode of its frame g (5 frames = 16 CIFs + the frame's own 4): a member has
        // one frame per tick at most, so the decode of tick T - 4 is the youngest that may still read what this tick overwrites
        if (tick_no >= 4) BK(hipStreamWaitEvent(a.get(), ticks[(tick_no - 4) % TICKS].ev_done.get(), 0));
        bank_scatter_kernel<<<dim3(8, (unsigned)nF), 256, 0, a.get()>>>(d_bits.get(), d_hist.get(), dtab, d_fine.get(), d_states.get());
        BK(hipGetLastError());
        BK(hipEventRecord(t.ev_demod.get(), a.get()));
        frames_enqueued = true;
    }
    // ---- synchronisers: behind the frames' fine-frequency updates, in front of the decode's launches and the bulky copies back ----
    if (nS) {
        int lo = MAXM, up = -1;
        for (const auto& j : r.sync_jobs) { lo = j.m->slot < lo ? j.m->slot : lo; up = j.m->slot > up ? j.m->slot : up; }
        // (the members copied their PRS slots into the bank's pinned array when they posted: one upload of the range that holds this round's)
        BK(hipMemcpyAsync(d_prs.get() + (size_t)lo * NFFT * 2, h_prs.get() + (size_t)lo * NFFT * 2, (size_t)(up - lo + 1) * NFFT * 2 * sizeof(float), hipMemcpyHostToDevice, a.get()));
        const dabgpu_sync_cfg& cfg = r.sync_jobs[0].cfg;
        const bool coarse = cfg.is_coarse_freq_correction != 0;
        if ((st = dabgpu_launch_sync(c, 1, d_prs.get(), NFFT, t.n_ens, &cfg, d_states.get(), d_imp.get(), coarse ? d_frq.get() : nullptr, dtab->sync_active, a.get()))) return st;
        BK(hipMemcpyAsync(t.h_states.get(), d_states.get(), (size_t)t.n_ens * sizeof(dabgpu_sync_state), hipMemcpyDeviceToHost, a.get()));
        BK(hipMemcpyAsync(t.h_imp.get(), d_imp.get(), (size_t)t.n_ens * NFFT * sizeof(float), hipMemcpyDeviceToHost, a.get()));
        if (coarse) BK(hipMemcpyAsync(t.h_frq.get(), d_frq.get(), (size_t)t.n_ens * NFFT * sizeof(float), hipMemcpyDeviceToHost, a.get()));
    }
    BK(hipEventRecord(t.ev_sync.get(), a.get()));
    // ---- decode (stream B): enqueued behind the synchronisers -- its ~8 runtime calls used to sit in front of the synchroniser launch every reader waits for ----
    if (frames_enqueued) {
        const size_t n_sub = r.subs.size();
        if (r.fic || n_sub) {
            const size_t need = out_bytes((size_t)t.n_ens, n_sub, r.cif_out);
            if (d_out.needs(need)) {
                BK(hipStreamSynchronize(q));
                if ((st = d_out.regrow(need, "hipMalloc((void**)&d_out, need)"))) return st;
            }
            // (no wait: the tick's previous round was handed out before the scheduler reused the tick)
            if ((st = t.h_out.regrow(need, "hipHostMalloc((void**)&t.h_out, need, hipHostMallocDefault)"))) return st;
            const out_ptrs o = out_layout(d_out.get(), (size_t)t.n_ens, n_sub);
            BK(hipStreamWaitEvent(q, t.ev_demod.get(), 0));
            const int tie = r.frame_jobs[0].tie;
            if (n_sub) {
                if (r.fic) st = dabgpu_decode_ring_layout(c, d_hist.get(), (size_t)t.n_ens, (size_t)H * FRAME_BITS, H, dtab->newest, r.subs.data(), (int)n_sub, o.fib, o.fres, o.msc,
                                                         (size_t)4 * r.cif_out, o.mres, tie, DABGPU_BITS_NATURAL, q);
                else st = dabgpu_msc_decode_ring(c, d_hist.get(), (size_t)t.n_ens, (size_t)H * FRAME_BITS, H, dtab->newest, r.subs.data(), (int)n_sub, o.msc, (size_t)4 * r.cif_out, o.mres, tie, q);
            } else {
                st = dabgpu_fic_decode_ring(c, d_hist.get(), (size_t)t.n_ens, (size_t)H * FRAME_BITS, dtab->newest, o.fib, o.fres, tie, q);
            }
            if (st) return st;
            BK(hipMemcpyAsync(t.h_out.get(), d_out.get(), need, hipMemcpyDeviceToHost, q));
            t.decoded = true;
        }
    }
    if (frames_enqueued) {
        // the soft bits go straight to the page-locked buffer of the member's result slot (one copy per frame: what the delivery thread hands to the
        // observers is that buffer -- a compact copy per round plus a 230 KB memcpy per frame on the completer thread capped the bank at ~15 k frames/s)
        for (int j = 0; j < nF; j++) {
            const rx_bank_job& f = r.frame_jobs[(size_t)j];
            BK(hipMemcpyAsync(f.m->ses->slots[f.gen % dabgpu_frame_session::R].h_bits.get(), d_bits.get() + (size_t)j * FRAME_BITS, FRAME_BITS, hipMemcpyDeviceToHost, a.get()));
        }
        BK(hipMemcpyAsync(t.h_scal.get(), d_fine.get(), (size_t)(MAXM + nF) * sizeof(float), hipMemcpyDeviceToHost, a.get()));      // fine[0..nF) ... total[0..nF)
        BK(hipEventRecord(t.ev_copied.get(), a.get()));
    }
    BK(hipEventRecord(t.ev_done.get(), q));
    return DABGPU_OK;
}

int hip_bank::enqueue(const rx_bank_round& r) {
    int st = DABGPU_OK;
    for (const auto& j : r.resets) {                                       // :277-289, behind everything enqueued for the member so far
        const int e = dabgpu_check_hip(hipMemsetAsync(d_states.get() + j.m->slot, 0, sizeof(dabgpu_sync_state), a.get()), "hipMemsetAsync(bank reset)");
        if (e && !st) st = e;
    }
    return st ? st : enqueue_tick(r);
}

void hip_bank::hand_sync(const rx_bank_round& r, size_t k) {
    const rx_bank_tick& t = ticks[r.no % TICKS];
    dabgpu_rx_member* m = r.sync_jobs[k].m;
    m->sync_rec = t.h_states.get()[m->slot];
    m->sync_coarse = r.sync_jobs[k].cfg.is_coarse_freq_correction != 0;
    m->sync_imp.assign(t.h_imp.get() + (size_t)m->slot * NFFT, t.h_imp.get() + (size_t)(m->slot + 1) * NFFT);
    if (m->sync_coarse) m->sync_frq.assign(t.h_frq.get() + (size_t)m->slot * NFFT, t.h_frq.get() + (size_t)(m->slot + 1) * NFFT);
}

// copies the frame's results out of the round's page-locked arrays into its member's result store
int hip_bank::deliver_frame(const rx_bank_round& r, size_t j, int st) {
    const rx_bank_tick& t = ticks[r.no % TICKS];
    const size_t n_sub = r.subs.size();
    const out_ptrs o = out_layout(t.h_out.get(), (size_t)t.n_ens, n_sub);
    const rx_bank_job& f = r.frame_jobs[j];
    dabgpu_rx_member* m = f.m;
    dabgpu_frame_session* s = m->ses;
    std::lock_guard sg(s->mu);
    dabgpu_frame_session::slot& sl = s->slots[f.gen % dabgpu_frame_session::R];
    sl.gen = ~0ull;
    sl.fic = false; sl.subs.clear(); sl.sub_off.clear(); sl.sub_n.clear(); sl.cif_out = 0;
    if (!st && t.decoded) {
        const size_t need = 4 * 96 + (4 + 4 * n_sub) * sizeof(dabgpu_codeword_result) + (size_t)4 * r.cif_out;
        if (sl.h_block.needs(need) && sl.h_block.regrow(need, "bank") != DABGPU_OK) { st = DABGPU_ERR_HIP; dabgpu_set_error("bank: hipHostMalloc(result block)"); }
        if (!st) {
            sl.h_fib = sl.h_block.get();
            sl.h_fres = reinterpret_cast<dabgpu_codeword_result*>(sl.h_fib + 4 * 96);
            sl.h_mres = sl.h_fres + 4;
            sl.h_msc = reinterpret_cast<uint8_t*>(sl.h_mres + 4 * n_sub);
            const size_t e = (size_t)m->slot;
            if (r.fic) { memcpy(sl.h_fib, o.fib + e * 4 * 96, 4 * 96); memcpy(sl.h_fres, o.fres + e * 4, 4 * sizeof(dabgpu_codeword_result)); }
            if (n_sub) { memcpy(sl.h_mres, o.mres + e * 4 * n_sub, 4 * n_sub * sizeof(dabgpu_codeword_result)); memcpy(sl.h_msc, o.msc + e * 4 * r.cif_out, (size_t)4 * r.cif_out); }
            sl.fic = r.fic; sl.subs = r.subs; sl.sub_off = r.sub_off; sl.sub_n = r.sub_n; sl.cif_out = r.cif_out;
        }
    }
    // (sl.h_bits: the round's device-to-host copy wrote it, enqueue_tick)
    if (!sl.h_aux && sl.h_aux.alloc(4, "bank") != DABGPU_OK) { if (!st) { st = DABGPU_ERR_HIP; dabgpu_set_error("bank: hipHostMalloc(aux)"); } }
    if (sl.h_aux) { sl.h_aux.get()[0] = t.h_scal.get()[j]; sl.h_aux.get()[1] = t.h_scal.get()[MAXM + j]; }
    sl.pending = false;
    sl.gen = f.gen;
    return st;
}

// Buffer gen % RX_BANK_IQ_FRAMES of the member's device buffer, on an upload stream that waits for nothing: frame gen - RX_BANK_IQ_FRAMES, which used it, has
// been handed out -- post_frame lets gen in only while gen < done_gen + R - 1 -- so the completer's host wait for its round, gather included, came before this
// copy was enqueued.  (Two buffers, on the argument that a synchroniser is posted between two frames, were overwritten by the third of the up to R - 1 frames
// that may be posted with none in between: the round of frame g records its event on the upload stream behind the uploads of g + 1 and g + 2.)
int hip_bank::upload(dabgpu_rx_member* m, int stage, size_t frame_sample, uint64_t gen, int up_k, const float** d_out_iq) {
    (void)hipSetDevice(device);
    float* d = m->dev->d_iq.get() + (size_t)(gen % RX_BANK_IQ_FRAMES) * FRAME_SAMPLES * 2;
    hipStream_t u = up[up_k].get();
    int st = dabgpu_check_hip(hipMemcpyAsync(d, m->h_stage[stage] + 2 * frame_sample, FRAME_SAMPLES * 2 * sizeof(float), hipMemcpyHostToDevice, u), "hipMemcpyAsync(bank frame)");
    if (!st) st = dabgpu_check_hip(hipEventRecord(m->dev->stage_ev[stage].get(), u), "hipEventRecord(bank stage)");
    *d_out_iq = d;
    return st;
}

int hip_bank::fetch_frame(dabgpu_rx_member* m, uint64_t generation, dabgpu_receiver_frame* out) {
    dabgpu_frame_session::slot& sl = m->ses->slots[generation % dabgpu_frame_session::R];
    if (sl.gen != generation) { dabgpu_set_error("receiver_wait_frame: generation %llu is gone", (unsigned long long)generation); return DABGPU_ERR_NOT_READY; }
    out->generation = generation;
    out->bits = sl.h_bits.get();
    out->n_bits = FRAME_BITS;
    out->freq_fine = sl.h_aux.get()[0];
    out->total_phase = sl.h_aux.get()[1];
    out->fft = sl.h_fft.get();
    out->dqpsk = sl.h_dq.get();
    return DABGPU_OK;
}

int hip_bank::member_open(dabgpu_rx_member* m) {
    (void)hipSetDevice(device);
    rx_member_device* d = m->dev = new (std::nothrow) rx_member_device();
    if (!d) return DABGPU_ERR_HIP;
    int st = dabgpu_frame_session_create_store(&m->ses, ctx.get());
    for (int k = 0; k < 3 && !st; k++) st = d->stage_ev[k].create(dabgpu_wait_event_flags(true), "hipEventCreate(bank member)");
    if (!st) st = d->d_iq.alloc((size_t)RX_BANK_IQ_FRAMES * FRAME_SAMPLES * 2, "hipMalloc(bank member samples)");
    // the rounds copy a frame's soft bits straight into the result slot's page-locked buffer (the session owns them)
    for (int k = 0; k < dabgpu_frame_session::R && !st; k++) st = m->ses->slots[k].h_bits.alloc(FRAME_BITS, "hipHostMalloc(bank member soft bits)");
    if (!st) st = dabgpu_check_hip(hipMemsetAsync(d_states.get() + m->slot, 0, sizeof(dabgpu_sync_state), a.get()), "hipMemsetAsync(bank member state)");
    if (!st) st = dabgpu_check_hip(hipMemsetAsync(d_hist.get() + (size_t)m->slot * H * FRAME_BITS, 0, (size_t)H * FRAME_BITS, a.get()), "hipMemsetAsync(bank member history)");
    if (!st) st = dabgpu_check_hip(hipStreamSynchronize(a.get()), "hipStreamSynchronize(bank member)");
    if (st) member_close(m);
    return st;
}

void hip_bank::member_close(dabgpu_rx_member* m) {
    (void)hipSetDevice(device);
    if (m->ses) dabgpu_frame_session_destroy(m->ses);
    delete m->dev;
}

hip_bank::~hip_bank() {
    // the waits only: the members release themselves, the context last (declared first)
    (void)hipSetDevice(device);
    if (a) (void)hipStreamSynchronize(a.get());
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    for (const dabgpu::Stream& u : up) if (u) (void)hipStreamSynchronize(u.get());
}
}  // namespace

int dabgpu_rx_bank_device_open(int device, rx_bank_device** out) {
    *out = nullptr;
    hip_bank* b = new (std::nothrow) hip_bank();
    if (!b) return DABGPU_ERR_HIP;
    b->device = device;
    const int st = b->open();
    if (st) { delete b; return st; }
    *out = b;
    return DABGPU_OK;
}
