// dabgpu_internal.h -- shared between the translation units of libdabgpu.so (not installed)
// Who owns what the runtime hands out (device and pinned memory, events, streams), and who only points at it: device_mem.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <mutex>
#include <vector>

#include "dabgpu.h"
#include "dabgpu_host_logic.h"
#include "device_mem.h"

// device tables of one transmission mode, one allocation (starting at prs)
struct dabgpu_mode_tables {
    float* prs;                      // PRS spectrum, n_fft complex
    float* prs_time_ref;             // conj(IFFT(relative_phase(PRS))), coarse-sync reference
    int* mapper;                     // carrier mapper: soft bit n sits on carrier mapper[n]
    int* inv_map;                    // its inverse: carrier c carries soft bit inv_map[c]
    uint16_t* inv_map16;             // the same as uint16_t (the mode I demodulator and transmitter read it)
};

// Device scratch slots of a context (dabgpu_scratch), numbered in this order: one grow-only buffer each (a captured graph holds their
// addresses).  Entry points that never run inside one another share slots.
enum dabgpu_scratch_slot : int {
    SCR_DEMOD_CORR,            // 0: cyclic-prefix correlations the caller of a mode I demodulation did not ask for
    // 1-6: single-frame host forms (*_host_sync, *_stream_frame_sync): IQ in, soft bits out, frequency words (or [net, fine, total phase]),
    // correlations, total phases, FFT view; the transmitter's host form: IQ out, payload in BITS, the caller's PRS in FFT
    SCR_HOST_IQ, SCR_HOST_BITS, SCR_HOST_FREQ, SCR_HOST_CORR, SCR_HOST_PHASE, SCR_HOST_FFT,
    // shared, as SCR_TUNE_TAIL below: the transmitter's host form has neither correlations nor frequency words, its TII lists and counts live there
    SCR_HOST_TII_LIST = SCR_HOST_CORR, SCR_HOST_TII_COUNT = SCR_HOST_FREQ,
    SCR_SYNC_SYM = SCR_HOST_FFT + 1, SCR_SYNC_STATE, SCR_SYNC_RESP,     // 7-9: ofdm_sync_host_sync: PRS symbol, record, responses
    SCR_CW_DESCS, SCR_VIT_WAVE, SCR_MSC_PLANS,       // 10-12: codeword descriptors, wave Viterbi state, MSC plans
    SCR_HOST_DQPSK,                                  // 13: DQPSK view of the single-frame host form
    SCR_CW_SRC, SCR_CW_OUT, SCR_CW_RESULT,           // 14-16: one codeword from host memory
    SCR_VIT_GROUPS, SCR_VIT_SYM, SCR_VIT_DEC,        // 17-19: lane / octet Viterbi: groups, kept soft bits, decisions
    SCR_CONVERT_IN, SCR_CONVERT_OUT, SCR_RAW_IQ,     // 20-22: host-buffer format conversion; ofdm_demod_frames_raw's converted block
    SCR_MODE_CORR, SCR_TUNE_TAIL = SCR_MODE_CORR,    // 23, shared: ofdm_demod_frames_mode's unwanted correlations, ofdm_tune's phase tail
    SCR_LANE_SUBS, SCR_VIT_SCHED,                    // 24-25: MSC lane -> sub-channel table, puncturing schedules
    SCR_BER_TABLES, SCR_BER_HOST,                    // 26-27: channel BER: a multiplex's encoder tables; the single-code-word host forms' block
    SCR_NAMED,
    // the FIC decoders' own copies of the decoder slots (scratch_fic): one context decodes the FIC and the MSC on two streams at once
    SCR_FIC_OFFSET = 20,
    SCR_COUNT = SCR_NAMED + SCR_FIC_OFFSET,
};
template <dabgpu_scratch_slot S> constexpr dabgpu_scratch_slot scratch_fic(bool fic) {
    static_assert(S + SCR_FIC_OFFSET >= SCR_NAMED && S < SCR_NAMED, "the FIC copy of this slot would overlap another slot");
    return fic ? dabgpu_scratch_slot(S + SCR_FIC_OFFSET) : S;
}

struct dabgpu_ctx {
    int device = 0;
    int n_cu = 0;
    hipStream_t stream = nullptr;
    float* d_tw = nullptr;           // 2048 x (cos, -sin)
    // [mode]: mode I from the context's PRS and mapper (dabgpu_create), modes II-IV built on first use (dabgpu_mode_tables_of)
    dabgpu_mode_tables modes[5] = {};
    struct dabgpu_vit_tables* d_vit_tables = nullptr;
    int vit_mapping = 0;             // DABGPU_VIT_MAP_* (dabgpu_viterbi_set_mapping)
    // symbols_per_block = 0 of the mode I demodulator: what dabgpu_ofdm_tune measured on this device, per size bucket (ceil log2 of the
    // batch) and kernel variant (loader, soft-bit layout, phase tail); the data path only looks it up (dabgpu_abi.hip)
    struct spb_choice { int bucket; int variant; int spb; };
    std::vector<spb_choice> spb_cache;
    void* scratch[SCR_COUNT] = {};   // grow-only device scratch slots (dabgpu_scratch)
    size_t scratch_bytes[SCR_COUNT] = {};
    std::vector<void*> parked;       // outgrown slots a captured graph may still address (dabgpu_scratch); freed with the context
    bool captured_once = false;      // a capturable entry point of this context has run under hipStreamBeginCapture
    // Host-side entry points (*_host_sync, msc_stream_*, dabplus_process_frame_host_sync) share the context's stream and scratch
    // slots: they serialise on this lock, so decoder objects living on different threads (BasicThreadPool workers,
    // src/basic_radio/basic_radio.cpp:51-60) may share one context.  The batch entry points (device pointers + caller's stream)
    // take no lock: one thread per context, or the caller's own exclusion.
    std::recursive_mutex host_mu;
    // pinned staging ring for small host -> device copies whose source does not outlive the call (descriptor tables, a caller's
    // CIF): copy into a pinned slot, asynchronous DMA from there, an event marks the slot reusable
    struct stage_slot { void* h = nullptr; size_t bytes = 0; hipEvent_t ev = nullptr; bool pending = false; std::mutex mu; };
    stage_slot stage[8];
    unsigned stage_next = 0;
    std::mutex stage_mu;
    // small tables that are a function of the call's arguments only (the sub-channel plans of a multiplex): what was last uploaded where
    // and on which stream -- a call that would upload the same bytes to the same place on the same stream uploads nothing
    // (dabgpu_stage_h2d_cached).  Steady-state decode calls then contain kernel launches only, which is what lets a caller capture them
    // in a HIP graph.
    struct table_copy { void* d = nullptr; hipStream_t s = nullptr; std::vector<unsigned char> bytes; };
    table_copy tables[3];
    std::mutex tables_mu;
};
#define DABGPU_HOST_LOCK(ctx) std::lock_guard<std::recursive_mutex> dabgpu_host_lock_(ctx->host_mu)
// return the status of a HIP call that failed (needs an `int st` in scope)
#define DABGPU_CK(call) do { st = dabgpu_check_hip((call), #call); if (st) return st; } while (0)
// asynchronous host -> device copy on `s` that has consumed h_src when it returns (h_src may be freed or overwritten at once)
extern "C" int dabgpu_stage_h2d(dabgpu_ctx* c, void* d_dst, const void* h_src, size_t bytes, hipStream_t s);
// the same for table `which` (0: sub-channel plans, 1: lane table, 2: channel BER tables) of the context, skipped when nothing changed (see dabgpu_ctx::tables)
extern "C" int dabgpu_stage_h2d_cached(dabgpu_ctx* c, int which, void* d_dst, const void* h_src, size_t bytes, hipStream_t s);

int dabgpu_check_hip(hipError_t e, const char* what);
// Every entry point that launches, allocates or copies first makes the context's device current on the calling thread (a worker
// thread of a one-process multi-GPU host starts on device 0) -- checked: a failed hipSetDevice is the call's status.
int dabgpu_bind_device(const dabgpu_ctx* c);
#define DABGPU_BIND(ctx) do { const int dabgpu_bind_st_ = dabgpu_bind_device(ctx); if (dabgpu_bind_st_) return dabgpu_bind_st_; } while (0)
// The head of every destroy function, `delete obj` its end.  False: no object, or its device cannot be bound -- nothing is freed on a device that is
// not current, the object is left alone whole (leaked, the error set).  True: the device is bound and idle (hipDeviceSynchronize); a destroy that
// waits for less (its own streams, an event) passes device_wait = false and waits itself.
bool dabgpu_destroy_begin(const void* obj, const dabgpu_ctx* c, bool device_wait = true);
// is `s` capturing a graph?  Asked of the runtime once per entry point, thread and stream (dabgpu_bind_device drops the memo)
bool dabgpu_stream_capturing(hipStream_t s);
// flags of the events host threads wait on (receiver pipeline, frame session, receiver bank): DABGPU_EVENT_WAIT=block makes hipEventSynchronize SLEEP
// instead of spinning -- threads that wait for the device then cost no CPU (a container's CPU quota is shared by every waiting thread of a many-receiver
// process), at ~20-50 us more wake-up latency; =spin is the runtime's default.  Unset: `bank_default` for the receiver bank's events, spin elsewhere.
unsigned dabgpu_wait_event_flags(bool bank_default_block);
int dabgpu_scratch(dabgpu_ctx* c, dabgpu_scratch_slot slot, size_t bytes, void** out);
// the same from a capturable entry point launching on `user` (HIP graphs: see the definition)
int dabgpu_scratch(dabgpu_ctx* c, dabgpu_scratch_slot slot, size_t bytes, void** out, hipStream_t user);
// the device tables of a transmission mode (mode I: the context's own), built on first use; DABGPU_ERR_INVALID_ARG for no mode
int dabgpu_mode_tables_of(dabgpu_ctx* c, int mode, const dabgpu_mode_tables** out, const char* who);

// capture formats the demodulators' loaders dequantise themselves (iq_decode.h): 0 = complex float, 1 = u8, 2 = s8, 3 = s16 little
// endian; -1 = none (with an error message naming `who`, when given)
inline int dabgpu_fused_loader(int format, const char* who = nullptr) {
    switch (format) {
    case DABGPU_IQ_RAW_F32L: case DABGPU_IQ_WAV_F32: return 0;
    case DABGPU_IQ_RAW_U8: case DABGPU_IQ_WAV_PCM8: return 1;
    case DABGPU_IQ_RAW_S8: return 2;
    case DABGPU_IQ_RAW_S16L: case DABGPU_IQ_WAV_PCM16: return 3;
    default:
        if (who) dabgpu_set_error("%s: format %d has no fused loader (float32, u8, s8, s16 little endian do)", who, format);
        return -1;
    }
}

// argument checks of the entry points that demodulate into soft bits of mode I (who = the entry point's name in the message)
inline int dabgpu_check_bits_layout(const char* who, int bits_layout) {
    if (bits_layout == DABGPU_BITS_NATURAL || bits_layout == DABGPU_BITS_MSC_CLASSED) return DABGPU_OK;
    dabgpu_set_error("%s: unknown bits_layout %d", who, bits_layout); return DABGPU_ERR_INVALID_ARG;
}
// soft-bit frame stride; IQ (`iq`) aligned to iq_align bytes, soft bits to 16
inline int dabgpu_check_bits_buffers(const char* who, size_t bits_frame_stride, const char* iq, const void* d_iq, int iq_align, const void* d_bits) {
    if (bits_frame_stride != 0 && (bits_frame_stride < DABGPU_NB_FRAME_BITS || (bits_frame_stride & 15))) {
        dabgpu_set_error("%s: bits_frame_stride must be 0 or a multiple of 16 >= 230400", who); return DABGPU_ERR_INVALID_ARG;
    }
    if (((uintptr_t)d_iq & (uintptr_t)(iq_align - 1)) || ((uintptr_t)d_bits & 15)) {
        dabgpu_set_error("%s: %s must be %d-byte, d_bits 16-byte aligned", who, iq, iq_align); return DABGPU_ERR_INVALID_ARG;
    }
    return DABGPU_OK;
}

// per-stream work item of a stream bank round (ofdm_stream.hip -> ofdm_demod.hip)
struct dabgpu_frame_desc {
    int slot;               // output slot of the completed frame, < 0: nothing to demodulate
    int split;              // samples [0, split) come from the stream's frame buffer (even)
    long long tail_off;     // sample offset inside the stream's current block of frame sample `split`
    // retained blocks (dabgpu_stream_bank_process_retained): frame samples [carry_dst, carry_end) (even bounds, inside [0, split)) are read
    // from the stream's PREVIOUS block, frame sample n at block sample carry_off + n; carry_end = 0: none
    int carry_dst, carry_end;
    long long carry_off;
};

// one demodulator launch (dabgpu_launch_demod): every field at the value that leaves it out.  The tables are the launcher's to find.
struct dabgpu_demod_call {
    // input: frames one after the other unless a stride is given; src = the loader (dabgpu_fused_loader)
    const void* d_iq = nullptr;
    int src = 0;
    size_t frame_stride_samples = 0;            // 0 = the mode's frame, frame after frame
    const float* d_freq = nullptr;              // per frame, nullptr = 0
    // outputs
    int8_t* d_bits = nullptr;
    size_t bits_frame_stride = 0;               // 0 = 230400
    int classed = 0;                            // MSC symbols in time-interleaver class order (soft bits only)
    float* d_cp_corr = nullptr;
    float* d_fft = nullptr;                     // display views (modes II-IV: d_fft only, from the size-generic kernel)
    float* d_dqpsk = nullptr;
    // batch
    int n_frames = 0;
    int symbols_per_block = 0;                  // 0 = the mode's default run length
    bool generic_mode1 = false;                 // mode I on the size-generic kernel (dabgpu_ofdm_demod_frames_mode)
    // stream bank round: frame = stream, samples [0, split) from d_iq (the frame buffers), the rest from the caller's block(s) in format src
    const dabgpu_frame_desc* d_desc = nullptr;
    const void* d_block = nullptr;
    size_t block_stride = 0;
    const void* d_prev_block = nullptr;         // retained blocks
    // sync records: frame k starts prs_offset + d_sync[k].fine_time_offset samples into its slice, PLL offset and fine-frequency word are the record's
    dabgpu_sync_state* d_sync = nullptr;
    int prs_offset = 0;
    // phase tail: total phase error and fine-frequency update of every frame (either may be null)
    float* d_total_phase = nullptr;
    float* d_fine_freq = nullptr;
    float beta = 0.0f;
    // soft-decision policy (dabgpu_soft_cfg); DABGPU_SOFT_CSI: d_soft_scale [n_frames] receives the scale of every frame (may be null)
    int soft_policy = DABGPU_SOFT_NORMALISED;
    float soft_level = 64.0f;
    float* d_soft_scale = nullptr;
    bool bank_soft = false;                     // a bank round under DABGPU_SOFT_CSI: d_soft_scale is indexed by the descriptors' bits slot (bank_process_impl only)
    // ... that also stores every completed frame's DQPSK products [75][1536] complex float at d_bank_dqpsk + slot * 75 * 1536, slot = the
    // descriptor's bits slot (dabgpu_stream_bank_set_products); not d_dqpsk, the display view, which is indexed by frame
    bool bank_products = false;
    float* d_bank_dqpsk = nullptr;
};
// plans the call (dabgpu_host_plan_demod) and launches the demodulation kernel of the mode's family, then the phase kernel if the plan asks for it;
// what = how a HIP failure of the mode I launch is reported (the entry points' own wording)
int dabgpu_launch_demod(dabgpu_ctx* c, int mode, const dabgpu_demod_call& a, hipStream_t stream, const char* what = "ofdm_demod_kernel launch");
// the families outside ofdm_demod.hip: a launch from the plan through the table beside the kernels (ofdm_modes.hip, ofdm_wave512.hip)
int dabgpu_enqueue_demod_generic(int mode, const dabgpu_demod_plan& p, const dabgpu_demod_call& a, const float* d_tw, const dabgpu_mode_tables& t,
                                 hipStream_t stream);
int dabgpu_enqueue_demod_wave(int mode, const dabgpu_demod_plan& p, const dabgpu_demod_call& a, const float* d_tw, const dabgpu_mode_tables& t,
                              hipStream_t stream);
// a kernel table has an entry in every place (an initialiser that is too short leaves null pointers behind)
template <class K, size_t N> constexpr bool dabgpu_kernels_all_set(const K (&table)[N]) {
    for (size_t i = 0; i < N; i++) if (table[i] == nullptr) return false;
    return true;
}

extern "C" hipError_t dabgpu_launch_ofdm_phase(const float* d_cp_corr, int n_frames, float beta, float* d_total_phase,
                                               float* d_fine_freq, int fine_freq_stride, const dabgpu_frame_desc* d_desc, int n_sym, int n_fft,
                                               hipStream_t stream);

// OFDM transmitter (ofdm_mod.hip): n_frames frames of `mode` from their payloads (layout DABGPU_TX_PAYLOAD_*) into d_out (format
// DABGPU_IQ_RAW_F32L / _U8), NULL first; d_prs = the PRS spectrum (nb_fft complex float) on the device, nullptr = the mode's own;
// arguments checked by the caller.  d_tii [n_frames][DABGPU_TII_MAX_TX] and d_tii_count [n_frames] (mode I, both or neither): the TII
// symbol in the NULL period of the frames that name transmitters
int dabgpu_launch_ofdm_mod(dabgpu_ctx* c, int mode, const uint8_t* d_payload, int layout, size_t n_frames, const float* d_prs, float freq_norm,
                           void* d_out, int out_format, hipStream_t s, const dabgpu_tii_tx* d_tii = nullptr, const uint8_t* d_tii_count = nullptr);

// ---- channel decode ----
typedef dabgpu_codeword dabgpu_cw_desc;
typedef dabgpu_codeword_result dabgpu_cw_result;
#define DABGPU_CW_LANE_MAPPED 0x80000000u      // internal flag bit of dabgpu_codeword.flags (set by msc_build_descs_kernel)
// (struct dabgpu_vit_group, the lane-per-codeword decoder's unit of work: dabgpu_host_logic.h)
extern "C" hipError_t dabgpu_launch_vit_groups_uniform(dabgpu_vit_group* d_groups, size_t n_cw, uint32_t n_steps,
                                                       const uint32_t* seg_pi, const uint32_t* seg_steps, hipStream_t stream);
// the same groups appended to another launch's (dabgpu_vit_group_base: dabgpu_host_logic.h)
extern "C" hipError_t dabgpu_launch_vit_groups_uniform_at(dabgpu_vit_group* d_groups, size_t n_cw, uint32_t n_steps, const uint32_t* seg_pi,
                                                          const uint32_t* seg_steps, dabgpu_vit_group_base base, hipStream_t stream);
// the two halves of a lane / octet decode: the gather of `kind` (0 general, 1 ring of 4 CIFs, 2 the same in class order, 3 direct)
// over some groups, and the trellis over groups that were gathered
extern "C" hipError_t dabgpu_launch_vit_prep(int kind, const dabgpu_vit_group* d_groups, size_t n_groups, uint32_t max_in_rows,
                                             const dabgpu_cw_desc* d_descs, uint32_t* d_sym, uint32_t groups_per_sub, hipStream_t stream);
extern "C" hipError_t dabgpu_launch_vit_trellis(const dabgpu_vit_group* d_groups, size_t n_groups, const dabgpu_cw_desc* d_descs, uint32_t* d_sym,
                                                uint32_t* d_dec, dabgpu_cw_result* d_results, int tie_rule, const struct dabgpu_vit_tables* d_tables,
                                                const uint2* d_sched, int octet, int n_cu, hipStream_t stream);
extern "C" hipError_t dabgpu_launch_vit_groups_msc(dabgpu_vit_group* d_groups, const struct dabgpu_msc_plan* d_plans,
                                                   const uint64_t* d_lane_subs, int n_lane_sub, int n_sub, size_t n_ens,
                                                   uint32_t groups_per_sub, uint32_t sched_stride, hipStream_t stream);
// schedule tables (one per puncturing schedule of the call): sched_stride entries each.  The trellis kernels read entry t for the steps
// t < n_steps and prefetch up to DABGPU_VIT_SCHED_PREFETCH entries beyond the last step, so sched_stride >= n_steps + DABGPU_VIT_SCHED_PREFETCH;
// callers size the tables with dabgpu_vit_alloc_steps (>= n_steps + 6, static check below)
extern "C" hipError_t dabgpu_launch_vit_sched_uniform(uint2* d_sched, uint32_t sched_stride, const uint32_t* seg_pi, const uint32_t* seg_steps,
                                                      const struct dabgpu_vit_tables* d_tables, hipStream_t stream);
extern "C" hipError_t dabgpu_launch_vit_sched_msc(uint2* d_sched, uint32_t sched_stride, const struct dabgpu_msc_plan* d_plans,
                                                  const uint64_t* d_lane_subs, int n_lane_sub, const struct dabgpu_vit_tables* d_tables,
                                                  hipStream_t stream);
// eight lanes per codeword over prepared groups and their symbol array (viterbi_octet.hip): one 512-thread workgroup per group
extern "C" hipError_t dabgpu_launch_viterbi_octet(const dabgpu_vit_group* d_groups, size_t n_groups, const dabgpu_cw_desc* d_descs,
                                                  const uint32_t* d_sym, uint32_t* d_dec, dabgpu_cw_result* d_results, int tie_rule,
                                                  const struct dabgpu_vit_tables* d_tables, const uint2* d_sched, hipStream_t stream);
extern "C" hipError_t dabgpu_launch_viterbi(const dabgpu_cw_desc* d_descs, int n_cw, uint64_t* d_scratch,
                                            size_t scratch_words_per_wave, int n_waves, int max_out_bytes,
                                            dabgpu_cw_result* d_results, int tie_rule, const dabgpu_vit_tables* d_tables,
                                            hipStream_t stream, int n_first = 0 /* > 0: code words n_first .. n_cw - 1 report into d_results_rest[0 ..] */,
                                            dabgpu_cw_result* d_results_rest = nullptr);
extern "C" hipError_t dabgpu_launch_fic_build(dabgpu_cw_desc* d_descs, const int8_t* d_bits, size_t n_frames,
                                              size_t frame_stride, uint8_t* d_out, const int32_t* d_slots, hipStream_t stream);
extern "C" hipError_t dabgpu_launch_msc_fic_build(dabgpu_cw_desc* d_descs, const int8_t* d_hist, size_t n_ens, size_t ens_stride,
                                                  int hist_frames, int newest_frame_slot, const dabgpu_msc_plan* d_plans, int n_sub,
                                                  uint8_t* d_out, size_t out_ens_stride, int cif_out_bytes, const int32_t* d_slots,
                                                  int classed, const int8_t* d_fic_bits, uint8_t* d_fib_out, hipStream_t stream);
extern "C" hipError_t dabgpu_launch_msc_build(dabgpu_cw_desc* d_descs, const int8_t* d_hist, size_t n_ens, size_t ens_stride,
                                              int hist_frames, int newest_frame_slot, const dabgpu_msc_plan* d_plans, int n_sub,
                                              uint8_t* d_out, size_t out_ens_stride, int cif_out_bytes, const int32_t* d_slots,
                                              int classed, hipStream_t stream);

// one wavefront per codeword over descriptors on the device (dabgpu_decode_abi.hip); fic: in the FIC decoders' copies of the scratch slots;
// n_first > 0: codewords n_first .. n - 1 report into d_results_rest[0 ..]
int dabgpu_run_viterbi(dabgpu_ctx* c, const dabgpu_cw_desc* d_descs, size_t n, uint32_t max_steps, uint32_t max_out_bytes, int tie_rule,
                       dabgpu_codeword_result* d_results, hipStream_t s, bool fic = false, size_t n_first = 0,
                       dabgpu_codeword_result* d_results_rest = nullptr);

// ---- frame session (frame_session.hip) ----
// One receiver's decode state behind the single-stream classes: an 8-frame history of soft bits on the device, the FIC + MSC decode of
// every frame pushed, result slots in pinned host memory (include/dabgpu.h, "Frame session").  Frames arrive either from host memory
// (dabgpu_frame_session_push_frame) or -- the receiver pipeline, receiver.hip -- are demodulated straight into the history slot by a
// producer stream: dabgpu_session_reserve hands the slot out, dabgpu_session_commit chains the decode behind the producer's event.
struct dabgpu_frame_session {
    static constexpr int H = 8, R = 8;
    dabgpu_ctx* ctx = nullptr;
    bool owns_ctx = true;                           // false: a result store of a receiver-bank member (receiver_bank.hip): no history, no stream of its own
    dabgpu::DeviceBuffer<int8_t> d_hist;            // [H][230400]
    // one device block per session, one pinned block per result slot: [4][96] FIB bytes | [4] FIC results | [4][n_sub] MSC results |
    // [4][cif_out] sub-channel bytes -- a frame's results reach the host in ONE copy (they were four; each is an operation on the stream
    // between two trellis launches)
    dabgpu::DeviceBuffer<uint8_t> d_block;
    uint8_t* d_fib = nullptr; dabgpu_codeword_result* d_fres = nullptr;       // (into d_block)
    uint8_t* d_msc = nullptr; dabgpu_codeword_result* d_mres = nullptr;
    std::vector<dabgpu_subchannel> subs;
    std::vector<uint32_t> sub_off, sub_n;           // byte offset / size of a sub-channel inside one CIF's output record
    uint32_t cif_out = 0;
    uint64_t next_gen = 0;                          // next generation to be committed (decode enqueued), in order
    uint64_t next_reserve = 0;                      // next generation to be reserved (>= next_gen: a producer may run ahead of the commits)
    struct slot {
        uint64_t gen = ~0ull; bool fic = false, pending = false;
        std::vector<dabgpu_subchannel> subs; std::vector<uint32_t> sub_off, sub_n; uint32_t cif_out = 0;
        dabgpu::PinnedBuffer<uint8_t> h_block;                                   // laid out like the session's d_block
        uint8_t* h_fib = nullptr; dabgpu_codeword_result* h_fres = nullptr;      // (into h_block) [4][96], [4]
        uint8_t* h_msc = nullptr; dabgpu_codeword_result* h_mres = nullptr;      // (into h_block) [4][cif_out], [4][n_sub]
        dabgpu::Event done;
        dabgpu::Event ev_ready, ev_copied;                                     // receiver pipeline: frame demodulated / its host copies made (producer stream)
        // receiver pipeline only (pinned, allocated at first use): the frame's soft bits, a few scalars of the producer, display views
        dabgpu::PinnedBuffer<int8_t> h_bits; dabgpu::PinnedBuffer<float> h_aux, h_fft, h_dq;
        bool soft_csi = false;                                                   // receiver pipeline: the frame was demodulated under DABGPU_SOFT_CSI (its scale is in h_aux)
    } slots[R];
    std::mutex mu;
};
// the history slot the next frame goes to (*d_frame_bits) and its result slot; waits (host) for the result slot's previous frame, makes
// `producer` wait (device) for the decode that still reads the history slot.  No frame is pushed yet: dabgpu_session_commit does that.
int dabgpu_session_reserve(dabgpu_frame_session* s, hipStream_t producer, uint64_t* gen, int8_t** d_frame_bits, dabgpu_frame_session::slot** sl);
// the frame reserved last is in its history slot once `ready` (recorded on the producer stream) has fired: the session's stream waits for
// it, copies `bits_bytes` soft bits to the slot's h_bits (0 = no copy), decodes, waits for `producer_done` (if given: copies the producer
// still makes to the slot's pinned buffers on its own stream, beside the decode) and records the slot's done event
int dabgpu_session_commit(dabgpu_frame_session* s, uint64_t gen, hipEvent_t ready, size_t bits_bytes, int decode, int decode_fic, int tie_rule,
                          hipEvent_t producer_done = nullptr);
void dabgpu_session_unreserve(dabgpu_frame_session* s, uint64_t gen);
// a session that only STORES results (slots filled by the receiver bank); ctx is borrowed
int dabgpu_frame_session_create_store(dabgpu_frame_session** out, dabgpu_ctx* ctx);
// result slot of a generation, waited for (DABGPU_ERR_NOT_READY: gone or never pushed); call with s->mu held
int dabgpu_session_slot(dabgpu_frame_session* s, uint64_t gen, dabgpu_frame_session::slot** out);

// ---- sync ----
extern "C" hipError_t dabgpu_launch_sync_init(const float* d_prs, const float* d_tw, float* d_prs_time_ref, int n_fft, hipStream_t stream);
// PRS synchronisation of n_streams symbols against the mode's PRS tables (built on first use)
int dabgpu_launch_sync(dabgpu_ctx* c, int mode, const float* d_prs_syms, size_t stride_samples, int n_streams, const dabgpu_sync_cfg* cfg,
                       dabgpu_sync_state* d_states, float* d_impulse, float* d_freq, const int* d_active, hipStream_t stream);
extern "C" hipError_t dabgpu_launch_cif_deinterleave(const int8_t* d_ring, int n_bits, int n_slots, int newest_slot,
                                                     int8_t* d_out, hipStream_t stream);
