/*
 * dabgpu.h -- C ABI of the MI355X-native DAB OFDM-demodulation + channel-decode hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types, `int` status
 * returns (0 = ok, see dabgpu_strerror), no exceptions cross it.  Each entry point names the
 * reference interface (williamyang98/DAB-Radio @ 2025-08-29, paths relative to the repo root)
 * it replaces.  Host-side C++ classes with the reference's own names and signatures
 * (OFDM_Demod, FIC_Decoder, MSC_Decoder, DAB_Viterbi_Decoder, CIF_Deinterleaver) are layered on
 * top of this ABI in dab-radio_amd/host/ ; INTEGRATION.md shows how basic_radio links them.
 *
 * Pointers prefixed d_ are DEVICE pointers (hipMalloc / torch tensor data_ptr), h_ are host.
 * `stream` is a hipStream_t passed as void* (NULL = the HIP default stream, as in HIP itself).  All launches
 * are asynchronous on that stream unless the function name ends in _sync (those use a private stream of the
 * context and return when the results are in host memory).
 *
 * HIP graphs: the batch entry points (dabgpu_ofdm_demod_frames*, dabgpu_ofdm_sync_demod_frames, dabgpu_fic_decode_frames,
 * dabgpu_msc_decode_frames*, dabgpu_decode_frames_layout) enqueue kernels only once they have run ONCE with the same shapes and the
 * same sub-channel list on the stream (scratch is grow-only, tables that depend on the sub-channel list are uploaded when they change):
 * such calls may be issued between hipStreamBeginCapture and hipStreamEndCapture.  A call that would have to upload a table during a
 * capture returns DABGPU_ERR_INVALID_ARG instead of invalidating it, and so does one that would have to grow the context's device scratch.
 * A captured graph holds the addresses of the context's scratch and tables as they were at capture time.  It stays VALID while the context
 * lives -- a later eager call with larger shapes gets new scratch, the outgrown buffers are kept until dabgpu_destroy once a call of the
 * context has run under capture -- and it stays CORRECT only while no call with another sub-channel list, another mapping
 * (dabgpu_viterbi_set_mapping, DABGPU_VIT_HYBRID_K) or larger shapes runs on the same context between its replays: those rewrite the plan and
 * lane tables the graph's kernels read.  One context per captured pipeline.  (tests/test_gpu_graph_capture.py)
 *
 * All functions fail with DABGPU_ERR_NO_DEVICE when no gfx950 device is usable: there is no CPU
 * fallback behind this ABI.
 */
#ifndef DABGPU_H
#define DABGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: symbols_per_block = 0 no longer measures (dabgpu_ofdm_tune does, explicitly); receiver pipeline (dabgpu_receiver_*)
 * 3: dabgpu_receiver_submit_demod / _submit_decode (the OFDM_Demod mirror class needs them) */
#define DABGPU_ABI_VERSION 4

/* Mode I geometry (src/ofdm/dab_ofdm_params_ref.cpp:13-21, src/dab/constants/dab_parameters.h:31-40) */
#define DABGPU_NB_FRAME_SYMBOLS 76
#define DABGPU_NB_SYMBOL_PERIOD 2552
#define DABGPU_NB_NULL_PERIOD   2656
#define DABGPU_NB_FFT           2048
#define DABGPU_NB_CYCLIC_PREFIX 504
#define DABGPU_NB_DATA_CARRIERS 1536
#define DABGPU_NB_FRAME_SAMPLES 196608
#define DABGPU_NB_SYM_BITS      3072
#define DABGPU_NB_FRAME_BITS    230400
#define DABGPU_NB_FIC_BITS      9216
#define DABGPU_NB_FIB_GROUP_BITS 2304
#define DABGPU_NB_CIF_BITS      55296
#define DABGPU_NB_CIFS          4

enum {
    DABGPU_OK = 0,
    DABGPU_ERR_NO_DEVICE = 1,      /* no HIP device / not gfx950 / runtime missing */
    DABGPU_ERR_INVALID_ARG = 2,
    DABGPU_ERR_HIP = 3,            /* a HIP call failed; text via dabgpu_last_error() */
    DABGPU_ERR_NOT_READY = 4,      /* e.g. time de-interleaver has fewer than 16 CIFs */
    DABGPU_ERR_UNSUPPORTED = 5     /* transmission mode other than I */
};
enum { DABGPU_CORE_SCALAR = 0, DABGPU_CORE_SIMD = 1 };    /* values of the `tie_rule` argument: "CORE MODEL" at the channel decoder below */

typedef struct dabgpu_ctx dabgpu_ctx;

const char *dabgpu_strerror(int status);
const char *dabgpu_last_error(void);          /* thread-local detail of the last failure */
int dabgpu_abi_version(void);
/* number of usable gfx950 devices (0 when none; never initialises a HIP context on failure) */
int dabgpu_device_count(void);

/*
 * Context = one device + its constant tables (FFT twiddles, inverse carrier map, conj(PRS), coarse-sync
 * time reference).  Replaces the constructor-time work of OFDM_Demod::OFDM_Demod
 * (src/ofdm/ofdm_demodulator.cpp:80-146): h_prs_fft_ref is get_DAB_PRS_reference() output
 * (2048 complex float, interleaved re/im), h_carrier_mapper is get_DAB_mapper_ref() output (1536 int).
 * Passing NULL for either uses the built-in Mode I tables.
 */
int dabgpu_create(dabgpu_ctx **out, int device, const float *h_prs_fft_ref, const int *h_carrier_mapper);
void dabgpu_destroy(dabgpu_ctx *ctx);
/* Page-lock / release a host buffer that is handed to the *_host_sync entry points repeatedly (hipHostRegister): the copies then run at
 * PCIe speed.  Optional -- unpinned buffers work, slower. */
int dabgpu_host_pin(void *h_buffer, size_t bytes);
int dabgpu_host_unpin(void *h_buffer);
int dabgpu_synchronize(dabgpu_ctx *ctx, void *stream);

/* Built-in Mode I tables, host side (replace get_DAB_PRS_reference src/ofdm/dab_prs_ref.cpp:140,
 * get_DAB_mapper_ref src/ofdm/dab_mapper_ref.cpp:10, and expose the FFT twiddle table of the arithmetic contract) */
int dabgpu_get_prs_fft_ref(int transmission_mode, float *h_out /*[2*2048]*/);
int dabgpu_get_carrier_mapper(int transmission_mode, int *h_out /*[1536]*/);
int dabgpu_get_fft_twiddles(float *h_out /*[2*2048]*/);

/* ------------------------------------------------------------------------------------------------
 * OFDM demodulation of frame-aligned frames: PLL + cyclic-prefix phase error + 2048-pt FFT + DQPSK +
 * frequency de-interleave + soft-bit quantisation, batched over frames.
 * Replaces OFDM_Demod::PipelineThread (src/ofdm/ofdm_demodulator.cpp:650-766) and its callees
 * ApplyPLL, CalculateCyclicPhaseError, CalculateFFT, CalculateDQPSK, CalculateViterbiBits.
 *
 *   d_iq          [n_frames][196608] complex float; frame layout = OFDM_Frame_Buffer's logical layout
 *                 (src/ofdm/ofdm_frame_buffer.h:87-99): 76 symbols x 2552 samples (PRS first) then the
 *                 NULL symbol (2656).  16-byte aligned.
 *   d_freq_offset [n_frames] net normalised frequency offset used by the PLL (coarse + fine), may be NULL (= 0)
 *   d_bits        [n_frames][230400] int8 soft bits, layout of On_OFDM_Frame() (ofdm_demodulator.cpp:635)
 *   d_cp_corr     [n_frames][76] complex float raw cyclic-prefix correlation per symbol, may be NULL
 *   d_fft         [n_frames][77][2048] complex float = GetFrameFFT() content, may be NULL (skips the
 *                 display-only NULL-symbol FFT, ofdm_demodulator.cpp:701-709)
 *   d_dqpsk       [n_frames][75][1536] complex float = GetFrameDataVec() content (X_i * conj(X_{i+1}) per carrier,
 *                 natural carrier order, ofdm_demodulator.cpp:842-865), may be NULL
 *   symbols_per_block  data symbols handled by one workgroup, 1..75; any value gives identical results.  0 = the library chooses, WITHOUT
 *                 measuring (the call stays asynchronous): batches below 512 frames take 25, below 86 frames shorter runs (down to 3) so
 *                 that the batch still spreads over the chip; larger ones take what dabgpu_ofdm_tune recorded for this kernel variant in
 *                 the nearest size bucket, else 25.  Which of 25 / 38 / 75 is fastest depends on the box.
 *   bits_frame_stride  bytes between the soft bits of consecutive frames (0 = 230400, packed); lets the kernel write
 *                 straight into slot k of a per-ensemble frame-history ring (see dabgpu_msc_decode_frames)
 */
int dabgpu_ofdm_demod_frames(dabgpu_ctx *ctx, const float *d_iq, size_t n_frames, const float *d_freq_offset,
                             int8_t *d_bits, float *d_cp_corr, float *d_fft, float *d_dqpsk, int symbols_per_block,
                             size_t bits_frame_stride, void *stream);

/*
 * The same with the frames still in their capture format (dabgpu_iq_format below; n_frames x 196608 IQ samples, 16-byte
 * aligned).  For raw_u8 / raw_s8 / raw_s16l (and wav PCM8 / PCM16 / float32 payloads) the kernel's loader reads the raw
 * samples straight from HBM and dequantises them in registers with the reader arithmetic of
 * examples/app_helpers/app_iq_readers.h:19-44,79-84 -- 2 or 4 bytes per sample instead of 8 and no conversion pass;
 * every other format is converted into context scratch on `stream` first.  Results are bit-identical to
 * dabgpu_iq_convert followed by dabgpu_ofdm_demod_frames.
 */
int dabgpu_ofdm_demod_frames_raw(dabgpu_ctx *ctx, const void *d_raw, int format, size_t n_frames, const float *d_freq_offset,
                                 int8_t *d_bits, float *d_cp_corr, float *d_fft, float *d_dqpsk, int symbols_per_block,
                                 size_t bits_frame_stride, void *stream);

/*
 * Demodulation straight into the frame-history ring the channel decoder reads (dabgpu_msc_decode_frames), with a choice of
 * how the MSC soft bits are laid out there.  Formats with a fused loader only (float32, u8, s8, s16 little endian, and the wav
 * payloads of those); soft bits and the cyclic-prefix correlation only.
 *   DABGPU_BITS_NATURAL      the layout of On_OFDM_Frame() (ofdm_demodulator.cpp:635): identical to dabgpu_ofdm_demod_frames_raw
 *   DABGPU_BITS_MSC_CLASSED  FIC (soft bits 0..9215) as above; inside each of the four CIF rows of 55296 soft bits, bit i is
 *                            stored at (i mod 16) * 3456 + i / 16.  CIF_Deinterleaver takes the bits of class i mod 16 from the
 *                            CIF that is 15 - bitrev4(i mod 16) CIFs old (src/dab/msc/cif_deinterleaver.cpp:57-68); in this order
 *                            each of those reads is contiguous, which cuts the history traffic of the decoder's gather from
 *                            19/4 of the decoded bits to 1 (the permutation itself costs nothing: it rides on the frequency
 *                            de-interleave the kernel performs anyway).  Only the *_layout decoders below read it.
 */
#define DABGPU_BITS_NATURAL 0
#define DABGPU_BITS_MSC_CLASSED 1
int dabgpu_ofdm_demod_frames_history(dabgpu_ctx *ctx, const void *d_raw, int format, size_t n_frames, const float *d_freq_offset,
                                     int8_t *d_bits, float *d_cp_corr, int symbols_per_block, size_t bits_frame_stride,
                                     int bits_layout, void *stream);

/*
 * dabgpu_ofdm_demod_frames_history followed by dabgpu_ofdm_phase_update(d_cp_corr, ...) as one call -- and as ONE launch whenever a
 * workgroup walks a whole frame (symbols_per_block = 75: explicit, or the library's own choice for this batch size): the phase tail
 * (per-symbol atan2, sequential sum, fine-frequency update: ofdm_demodulator.cpp:606-618, :779-840) then runs at the end of the
 * demodulation kernel, on the correlations it has just produced.  Otherwise the tail follows as its own launch.  Results are
 * identical to the two separate calls.  d_total_phase / d_fine_freq as in dabgpu_ofdm_phase_update (either may be NULL).
 */
int dabgpu_ofdm_demod_phase_frames(dabgpu_ctx *ctx, const void *d_raw, int format, size_t n_frames, const float *d_freq_offset,
                                   int8_t *d_bits, float *d_cp_corr, int symbols_per_block, size_t bits_frame_stride, int bits_layout,
                                   float fine_freq_update_beta, float *d_total_phase, float *d_fine_freq, void *stream);

/*
 * Calibration of symbols_per_block = 0, explicit and out of the data path: times the run lengths 25 / 38 / 75 of the demodulation of
 * n_frames frames (>= 512; smaller batches follow a fixed rule and return at once) on the caller's buffers -- ~40 ms of warm-up launches,
 * then three timed rounds over the candidates -- and records the fastest for (loader of `format`, bits_layout, with_phase_tail, size bucket
 * = ceil(log2(n_frames))).  BLOCKS the calling thread (hipEventSynchronize on `stream`; refused while the stream is capturing); d_bits
 * receives the frames' soft bits for a zero carrier offset; with_phase_tail times the candidates with the phase tail of dabgpu_ofdm_demod_phase_frames (on context
 * scratch, not on caller state).  *chosen (may be NULL) = the run length recorded.  Typical use: once at start-up per batch size.
 */
int dabgpu_ofdm_tune(dabgpu_ctx *ctx, const void *d_raw, int format, size_t n_frames, int8_t *d_bits, size_t bits_frame_stride,
                     int bits_layout, int with_phase_tail, void *stream, int *chosen);
/* what symbols_per_block = 0 resolves to for that call shape right now (never 0 for valid arguments) */
int dabgpu_ofdm_tuned_symbols_per_block(dabgpu_ctx *ctx, int format, size_t n_frames, int bits_layout, int with_phase_tail);
/* the run length most recently recorded by dabgpu_ofdm_tune for the size bucket of n_frames, whatever the variant: 25 / 38 / 75
 * (3 .. 25 below 86 frames: the fixed rule), or 0 = nothing recorded for that bucket */
int dabgpu_ofdm_auto_symbols_per_block(dabgpu_ctx *ctx, size_t n_frames);

/*
 * Per-frame scalar tail of the fine-frequency loop: phase[i] = atan2(corr[i]), total = sum_i phase[i]
 * (sequential, i = 0..75), and optionally fine <- fmod(fine - beta*err, wrap).
 * Replaces OFDM_Demod::CoordinatorThread's phase section (ofdm_demodulator.cpp:606-618) +
 * CalculateFineFrequencyError (:779-824) + UpdateFineFrequencyOffset (:829-840).
 *   d_cp_corr     [n_frames][76] complex float (from dabgpu_ofdm_demod_frames)
 *   d_total_phase [n_frames] out, may be NULL
 *   d_fine_freq   [n_frames] in/out, may be NULL (no update)
 */
int dabgpu_ofdm_phase_update(dabgpu_ctx *ctx, const float *d_cp_corr, size_t n_frames, float fine_freq_update_beta,
                             float *d_total_phase, float *d_fine_freq, void *stream);

/* Host-buffer convenience: H2D of the frames, demod, D2H of bits (+ totals); synchronous.
 * h_total_phase may be NULL. This is what the single-stream OFDM_Demod mirror class calls per frame. */
int dabgpu_ofdm_demod_frames_host_sync(dabgpu_ctx *ctx, const float *h_iq, size_t n_frames, const float *h_freq_offset,
                                       int8_t *h_bits, float *h_total_phase, float *h_fft);

/*
 * One frame of one stream, host buffers, synchronous, including the fine-frequency loop update: the PLL runs with
 * freq_coarse + *h_freq_fine, then *h_freq_fine <- fmod(*h_freq_fine - beta * err, wrap) on the device
 * (src/ofdm/ofdm_demodulator.cpp:606-618, :829-840).  h_fft [77][2048] and h_dqpsk [75][1536] complex float may be NULL.
 * This is the per-frame call of the OFDM_Demod mirror class (replaces CoordinatorThread + PipelineThread for one frame).
 */
int dabgpu_ofdm_demod_stream_frame_sync(dabgpu_ctx *ctx, const float *h_iq, float freq_coarse, float *h_freq_fine,
                                        float fine_freq_update_beta, int8_t *h_bits, float *h_total_phase, float *h_fft,
                                        float *h_dqpsk);

/* ------------------------------------------------------------------------------------------------
 * PRS synchronisation: integer-bin frequency offset (coarse) then symbol timing from the impulse response (fine).
 * Replaces OFDM_Demod::RunCoarseFreqSync and ::RunFineTimeSync (src/ofdm/ofdm_demodulator.cpp:360-471, :473-548),
 * one workgroup per stream.  `dabgpu_sync_cfg` mirrors OFDM_Demod_Config::sync (src/ofdm/ofdm_demodulator.h:34-44).
 */
typedef struct {
    float fine_freq_update_beta;              /* 0.9  */
    int   is_coarse_freq_correction;          /* 1    */
    float max_coarse_freq_correction_norm;    /* 0.5  */
    float coarse_freq_slow_beta;              /* 0.1  */
    float impulse_peak_threshold_db;          /* 20   */
    float impulse_peak_distance_probability;  /* 0.15 */
} dabgpu_sync_cfg;

typedef struct {
    float freq_coarse;        /* in/out: m_freq_coarse_offset */
    float freq_fine;          /* in/out: m_freq_fine_offset */
    int   is_found_coarse;    /* in/out: m_is_found_coarse_freq_offset */
    int   fine_time_offset;   /* out: m_fine_time_offset (PRS start relative to the expected position), when sync_valid */
    int   sync_valid;         /* out: 0 = impulse peak below threshold -> the caller must Reset() (:529-532) */
    int   reserved;
} dabgpu_sync_state;

void dabgpu_sync_cfg_default(dabgpu_sync_cfg *cfg);
/*
 *   d_prs_syms   stream s: 2048 complex float starting at d_prs_syms + s * stride_samples (complex samples) =
 *                m_correlation_time_buffer[nb_null_period ...], i.e. the first 2048 samples of the expected PRS slot
 *   d_states     [n_streams] in/out
 *   d_impulse_response / d_freq_response  [n_streams][2048] float dB, may be NULL
 *                (GetImpulseResponse() / GetCoarseFrequencyResponse())
 */
int dabgpu_ofdm_sync(dabgpu_ctx *ctx, const float *d_prs_syms, size_t n_streams, size_t stride_samples,
                     const dabgpu_sync_cfg *cfg, dabgpu_sync_state *d_states, float *d_impulse_response,
                     float *d_freq_response, void *stream);
/* single stream from host memory, synchronous; used by the OFDM_Demod mirror class once per frame */
int dabgpu_ofdm_sync_host_sync(dabgpu_ctx *ctx, const float *h_prs_sym, const dabgpu_sync_cfg *cfg,
                               dabgpu_sync_state *h_state, float *h_impulse_response, float *h_freq_response);

/*
 * One steady-state frame of n receivers in ONE call: PRS synchronisation at the expected position, demodulation from where the impulse
 * peak puts the frame with the offset the synchroniser has just tracked, fine-frequency update -- OFDM_Demod's per-frame sequence
 * RunCoarseFreqSync -> RunFineTimeSync -> PipelineThread (PLL with m_freq_coarse_offset + m_freq_fine_offset) -> CoordinatorThread's
 * UpdateFineFrequencyOffset (src/ofdm/ofdm_demodulator.cpp:360-471, :473-548, :650-766, :606-618), the sync records staying on the device:
 * dabgpu_ofdm_sync followed by a demodulation that reads d_states[k] for its position, its PLL offset and its fine-frequency word.
 *   d_iq      receiver k's samples: complex float at d_iq + 2 * k * stream_stride_samples (8-byte aligned); sample prs_offset_samples of the
 *             slice is where the receiver expects the PRS to begin (what m_correlation_time_buffer[nb_null_period] holds).  The frame's 76
 *             symbols are read from prs_offset_samples + fine_time_offset on; fine_time_offset lies in [-504, 1543], hence
 *             prs_offset_samples >= 504 and stream_stride_samples >= prs_offset_samples + 1544 + 76 * 2552 (also for the last receiver).
 *   d_states  [n_streams] in/out: freq_coarse / freq_fine / is_found_coarse persist from frame to frame; after the call freq_fine holds
 *             the value updated by this frame's cyclic-prefix phase error.  sync_valid = 0: the impulse-peak test failed, nothing was
 *             demodulated for that receiver (d_bits / d_cp_corr / d_total_phase rows untouched) and the caller resets it (:529-532).
 *   d_bits, d_cp_corr (may be NULL), symbols_per_block, bits_frame_stride, bits_layout: as dabgpu_ofdm_demod_frames_history
 *   d_total_phase [n_streams] sum of the 76 cyclic-prefix angles, may be NULL;  beta of the update = cfg->fine_freq_update_beta
 * Results equal dabgpu_ofdm_sync + dabgpu_ofdm_demod_frames_history on the shifted frames + dabgpu_ofdm_phase_update, bit for bit.
 */
int dabgpu_ofdm_sync_demod_frames(dabgpu_ctx *ctx, const float *d_iq, size_t n_streams, size_t stream_stride_samples,
                                  size_t prs_offset_samples, const dabgpu_sync_cfg *cfg, dabgpu_sync_state *d_states, int8_t *d_bits,
                                  float *d_cp_corr, int symbols_per_block, size_t bits_frame_stride, int bits_layout,
                                  float *d_total_phase, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Soft-decision policy of the mode I demodulator.
 *   DABGPU_SOFT_NORMALISED  the reference's (CalculateViterbiBits, ofdm_demodulator.cpp:867-889): every DQPSK product d is divided by
 *                           max(|re d|, |im d|), so every carrier reaches the decoder with the same weight.  The default; the entry
 *                           points without a dabgpu_soft_cfg compute exactly this.
 *   DABGPU_SOFT_CSI         channel-state weighted: the amplitude of d = X_i conj(X_i+1) -- small for a carrier in a fade -- stays in
 *                           the soft bit.  One factor per frame, k = level * 1536 / (2048 P), P = sum of re^2 + im^2 over the 2048
 *                           useful samples of the frame's phase reference symbol (samples 504 .. 2551 of the frame as the loader
 *                           delivers them, before the PLL), puts a component of mean size at +-level; soft bit = -(c k), c = re d
 *                           and -im d, NaN -> 0, clamped to [-127, 127], truncated towards zero.  P zero or not finite, or k not
 *                           finite: k = 0, every soft bit of the frame is 0 (an erasure).  Frequency de-interleave and both layouts
 *                           as ever.  Arithmetic: csrc/softbit_csi_core.h, the device equals dabgpu_soft_scale_host bit for bit.
 * level: [1, 127], default 64; anything else is DABGPU_ERR_INVALID_ARG.  Mode I only, no banked receiver.  The stream bank takes the
 * policy through dabgpu_stream_bank_set_soft: its frames lie in the stream's frame buffer and in the caller's blocks, P is the power of
 * symbol 0 as the bank's loader delivers it (frame-buffer samples as stored, block samples through the reader arithmetic of the format).
 */
#define DABGPU_SOFT_NORMALISED 0
#define DABGPU_SOFT_CSI 1
typedef struct { int policy; float level; } dabgpu_soft_cfg;
void dabgpu_soft_cfg_default(dabgpu_soft_cfg *cfg);
/* k of a frame from the 2048 useful samples (complex float) of its phase reference symbol; 0 for a level outside [1, 127] */
float dabgpu_soft_scale_host(const float *h_prs_useful, float level);
/*
 * dabgpu_ofdm_demod_frames_raw (display views, natural layout) / dabgpu_ofdm_demod_frames_history (either layout, no views) with a
 * soft-decision policy; formats with a fused loader only.  cfg->policy = DABGPU_SOFT_NORMALISED: those calls, byte for byte, and
 * d_soft_scale is not written.  d_soft_scale [n_frames] (may be NULL): k as used.  symbols_per_block = 0 resolves as for the
 * normalised call of the same loader and layout; the result does not depend on it.
 */
int dabgpu_ofdm_demod_frames_soft(dabgpu_ctx *ctx, const void *d_raw, int format, size_t n_frames, const float *d_freq_offset,
                                  int8_t *d_bits, float *d_cp_corr, float *d_fft, float *d_dqpsk, int symbols_per_block,
                                  size_t bits_frame_stride, int bits_layout, const dabgpu_soft_cfg *cfg, float *d_soft_scale,
                                  void *stream);
/* dabgpu_ofdm_sync_demod_frames with a soft-decision policy: the frame position comes from the sync record, and with it the window of
 * P.  A receiver with sync_valid = 0 leaves its d_soft_scale word untouched too. */
int dabgpu_ofdm_sync_demod_frames_soft(dabgpu_ctx *ctx, const float *d_iq, size_t n_streams, size_t stream_stride_samples,
                                       size_t prs_offset_samples, const dabgpu_sync_cfg *cfg, dabgpu_sync_state *d_states,
                                       int8_t *d_bits, float *d_cp_corr, int symbols_per_block, size_t bits_frame_stride,
                                       int bits_layout, float *d_total_phase, const dabgpu_soft_cfg *soft, float *d_soft_scale,
                                       void *stream);

/* ------------------------------------------------------------------------------------------------
 * Channel decoding: punctured K=7 rate-1/4 Viterbi (+ time de-interleave, energy dispersal, FIB CRC16),
 * one wavefront per codeword, batched.
 * Replaces DAB_Viterbi_Decoder::update/chainback (src/dab/algorithms/dab_viterbi_decoder.cpp:114-181) and the
 * vendor/viterbi_decoder core behind it, AdditiveScrambler (src/dab/algorithms/additive_scrambler.h:16-35),
 * CRC_Calculator<uint16_t> as used by the FIC (src/dab/fic/fic_decoder.cpp:19-31,103-116) and
 * CIF_Deinterleaver::Deinterleave (src/dab/msc/cif_deinterleaver.cpp:36-71).
 *
 * tie_rule = the CORE MODEL (the argument keeps its round-1 name): which of the upstream ViterbiDecoderCpp cores the decoder restates.
 *   DABGPU_CORE_SCALAR (0)  ViterbiDecoder_Scalar: uint16_t candidate sums that WRAP, the upper predecessor only when strictly smaller;
 *   DABGPU_CORE_SIMD   (1)  ViterbiDecoder_AVX_u16 / _SSE_u16 / _NEON_u16 -- what src/dab/algorithms/dab_viterbi_decoder.cpp:51-73 selects on
 *                           an AVX2 / SSE4.1 / AArch64 build host, i.e. the reference's default -march=native build on x86: adds_epu16 sums
 *                           that SATURATE at 65535, min_epu16 survivors, decision = cmpeq(survivor, upper candidate): the upper predecessor on ties.
 * For this code and soft bits in [-127, 127] no candidate sum can reach 65535 (at most 60454 + 254 * 19 = 65280: tests/test_independent_pins.py::
 * test_u16_candidate_sums_cannot_reach_65535 derives the bound from the polynomials and attacks it), so the two models give different bytes only
 * where two candidates tie exactly; both are implemented in full anyway.  Neither is pinned to upstream output here (vendor/viterbi_decoder is an
 * empty submodule): "parity unpinned" for the core, DESIGN.md 3.6.  The C++ classes pick the model the reference's build would have picked on
 * the host they run on (DABGPU_VITERBI_CORE=scalar|simd overrides; DABGPU_TIE_RULE=0|1 is the older spelling).
 * Soft bits are int8 in [-127,+127], 0 = punctured/erased (src/viterbi_config.h:11-14); -128 is read as -127.
 */
typedef struct {
    uint64_t d_src;            /* device address. direct (n_slots == 0): first soft bit of the codeword;
                                  ring: first soft bit of this sub-channel inside CIF slot 0 */
    uint64_t d_out;            /* device address of the decoded, descrambled bytes ((n_steps-6)/8 of them) */
    uint32_t n_steps;          /* trellis steps = information bits + 6 tail bits */
    uint32_t seg_pi[4];        /* puncturing vector index PI (1..24) of up to 4 segments, 0 = unused
                                  (src/dab/constants/puncture_codes.h:42-72); the 24-symbol tail PI_X is implicit */
    uint32_t seg_steps[4];     /* trellis steps of each segment = 32 * L (L = number of 128-bit blocks) */
    uint32_t start_state;      /* DAB_Viterbi_Decoder::reset(starting_state) */
    uint32_t n_crc_blocks;     /* > 0: output is that many equal blocks each ending in a CRC16 (FIBs) */
    uint32_t n_slots;          /* 0 = direct; else length of the CIF ring in slots (>= 16) */
    uint32_t newest_slot;      /* ring slot holding the most recent CIF of this codeword */
    uint32_t cifs_per_frame;   /* ring geometry: slot s lives at d_src + (s / cifs_per_frame) * frame_stride */
    uint32_t frame_stride;     /*                                      + (s % cifs_per_frame) * cif_stride   (bytes) */
    uint32_t cif_stride;
    uint32_t end_state;        /* DAB_Viterbi_Decoder::chainback(bytes_out, end_state), normally 0 */
    uint32_t flags;            /* DABGPU_CW_RAW: emit the decoder output without the energy-dispersal XOR */
} dabgpu_codeword;
/* longest code word any decoder entry point takes, in trellis steps (= information bits + 6): the one-wavefront-per-code-word kernel
 * assembles a code word's decoded bytes in LDS (60 KB).  17x the longest DAB code word (a sub-channel of all 864 capacity units at rate 8/9:
 * 27,648 steps); longer inputs return DABGPU_ERR_INVALID_ARG. */
#define DABGPU_MAX_TRELLIS_STEPS 491526u
#define DABGPU_CW_RAW 1u
#define DABGPU_CW_DEPUNCTURED 8u  /* direct codewords only (n_slots == 0): d_src holds the MOTHER code, 4 soft bits per trellis step with the punctured
                                  positions already 0 (the caller ran DAB_Viterbi_Decoder::depuncture_symbols, dab_viterbi_decoder.cpp:131-181,
                                  for whatever puncture vectors and lengths it was given); seg_pi / seg_steps are ignored, n_steps may be any
                                  value in 1 .. DABGPU_MAX_TRELLIS_STEPS, (n_steps - 6) / 8 whole bytes are written.  Always decoded by the WAVE mapping. */
#define DABGPU_CW_CLASSED 4u   /* ring codewords only: every ring row holds its cif_stride soft bits in time-interleaver class order;
                                  input bit i of a slot lives at d_src + slot offset + (i mod 16) * (cif_stride / 16) + i / 16, and
                                  d_src points at the sub-channel's first byte of class 0 (slot 0) */

typedef struct {
    uint64_t path_error;       /* DAB_Viterbi_Decoder::chainback() return value (dab_viterbi_decoder.cpp:124-129) */
    uint32_t crc_ok_mask;      /* bit i = CRC16 of block i matches (only when n_crc_blocks > 0) */
    uint32_t n_out_bytes;
} dabgpu_codeword_result;

/*
 * Three device mappings of the same decoder (identical results, bit for bit):
 *   WAVE   one wavefront per codeword, the 64 trellis states across its lanes (viterbi.hip) -- any batch, any mix of schedules
 *   LANE   one lane per codeword, wavefronts of 64 codewords that share a puncturing schedule (viterbi_lanes.hip) -- ~3x the
 *          throughput once a batch holds thousands of codewords per schedule; needs <= 768 bytes of scratch per trellis step
 *          and 64 codewords
 *   OCTET  eight lanes per codeword, 8 codewords per wavefront (viterbi_octet.hip), over the same groups and scratch as LANE --
 *          for the batches in between: when LANE would leave most SIMDs without a wavefront (64 codewords are indivisible there)
 * AUTO (default) compares a cost model of the three for the call at hand (LANE needs ~0.5 us per trellis step of its longest
 * schedule however small the batch, OCTET ~0.19 us, WAVE ~0.08 us per step of the longest codeword + 0.022 ns per codeword and step +
 * 0.011 us per codeword): e.g. the FIC goes WAVE -> OCTET at ~1000 frames and OCTET -> LANE at ~10000, the 18 x 48 CU multiplex
 * WAVE -> OCTET at ~65 ensembles and OCTET -> LANE at ~560
 * (dabgpu_viterbi_decode_batch: only when every codeword of the batch has the same n_steps / segments; forcing LANE or OCTET on
 * a mixed generic batch runs WAVE).
 */
#define DABGPU_VIT_MAP_AUTO 0
#define DABGPU_VIT_MAP_WAVE 1
#define DABGPU_VIT_MAP_LANE 2
#define DABGPU_VIT_MAP_OCTET 3
int dabgpu_viterbi_set_mapping(dabgpu_ctx *ctx, int mapping);

/* generic batch: h_codewords is a HOST array (copied to the device on `stream`); d_results a DEVICE array [n] */
int dabgpu_viterbi_decode_batch(dabgpu_ctx *ctx, const dabgpu_codeword *h_codewords, size_t n, int tie_rule,
                                dabgpu_codeword_result *d_results, void *stream);

/*
 * FIC of whole frames: for every frame the 4 FIB groups of 2304 soft bits (first 9216 bits of the frame) are
 * decoded with PI_16 x21, PI_15 x3, PI_X, descrambled and CRC-checked.
 * Replaces BasicFICRunner::Process + FIC_Decoder::DecodeFIBGroup (src/basic_radio/basic_fic_runner.cpp:34-49,
 * src/dab/fic/fic_decoder.cpp:53-117) for a batch.
 *   d_bits       frame f starts at d_bits + f * frame_stride (bytes); pass DABGPU_NB_FRAME_BITS for packed frames
 *   d_fib_bytes  [n_frames][4][96]: 3 x (30 data bytes + 2 CRC bytes) per group
 *   d_results    [n_frames][4]
 * dabgpu_fic_decode_* keep their device scratch apart from dabgpu_msc_decode_* / dabgpu_viterbi_decode_batch: one context may
 * decode the FIC and the MSC of a batch concurrently on two streams (the FIC fits into the SIMD time the MSC leaves idle).
 */
int dabgpu_fic_decode_frames(dabgpu_ctx *ctx, const int8_t *d_bits, size_t n_frames, size_t frame_stride,
                             uint8_t *d_fib_bytes, dabgpu_codeword_result *d_results, int tie_rule, void *stream);

/* Sub-channel description: the fields of `Subchannel` the decoder reads (src/dab/database/dab_database_entities.h:179-190) */
typedef struct {
    int start_address;   /* capacity units */
    int length;          /* capacity units */
    int is_uep;
    int uep_prot_index;  /* 0..63, row of the UEP table */
    int eep_prot_level;  /* 0..3 = level 1..4 */
    int eep_type;        /* 0 = EEP-A, 1 = EEP-B */
} dabgpu_subchannel;

/* (PI, L) plan of a sub-channel as MSC_Decoder::DecodeEEP/DecodeUEP derive it (src/dab/msc/msc_decoder.cpp:77-131,
 * src/dab/constants/subchannel_protection_tables.h); returns the number of segments (<= 4) or -1 */
int dabgpu_subchannel_plan(const dabgpu_subchannel *sc, int *pi4, int *l4, int *n_decoded_bytes);
/* DABGPU_OK when the decoders accept the descriptor: a profile of the tables, inside the 864 capacity units of a CIF, and consuming no more
 * soft bits than the sub-channel holds (UEP table row 34 as the reference lists it does: the reference's decoder runs out of symbols inside
 * its third update(), dab_viterbi_decoder.cpp:157-160; here the descriptor is refused); else DABGPU_ERR_INVALID_ARG with the reason in
 * dabgpu_last_error().  Host only, no device needed: what MSC_Decoder's constructor checks before anything is created (ABI 4). */
int dabgpu_subchannel_validate(const dabgpu_subchannel *sc);

/*
 * MSC of whole frames for many ensembles that share one multiplex configuration.  The time de-interleaver reads
 * straight from the history of demodulated frames: d_bits_history holds, per ensemble, `history_frames` (>= 5)
 * frame slots of 230400 soft bits used as a ring; the frame most recently written is slot `newest_frame_slot`.
 * Every call decodes the 4 CIFs of that newest frame for every listed sub-channel (the first 3 frames after a
 * (re)start yield garbage until 16 CIFs are in the ring -- the caller tracks that, as CIF_Deinterleaver's
 * m_total_frames_stored does, cif_deinterleaver.cpp:28-42).
 * Replaces MSC_Decoder::DecodeCIF (src/dab/msc/msc_decoder.cpp:46-115) x 4 CIFs x sub-channels x ensembles.
 *   ensemble e's history starts at d_bits_history + e * ensemble_stride (bytes)
 *   output of (ensemble e, cif c, sub-channel s) is written at d_out + e * out_ensemble_stride + c * B + off_s where
 *   B = sum of decoded bytes of all listed sub-channels and off_s the running sum; d_results is [n_ensembles][4][n_sub]
 */
int dabgpu_msc_decode_frames(dabgpu_ctx *ctx, const int8_t *d_bits_history, size_t n_ensembles, size_t ensemble_stride,
                             int history_frames, int newest_frame_slot, const dabgpu_subchannel *h_subchannels,
                             int n_subchannels, uint8_t *d_out, size_t out_ensemble_stride,
                             dabgpu_codeword_result *d_results, int tie_rule, void *stream);

/* The same reading a history whose MSC part was written in `bits_layout` (dabgpu_ofdm_demod_frames_history) */
int dabgpu_msc_decode_frames_layout(dabgpu_ctx *ctx, const int8_t *d_bits_history, size_t n_ensembles, size_t ensemble_stride,
                                    int history_frames, int newest_frame_slot, const dabgpu_subchannel *h_subchannels,
                                    int n_subchannels, uint8_t *d_out, size_t out_ensemble_stride,
                                    dabgpu_codeword_result *d_results, int tie_rule, int bits_layout, void *stream);

/*
 * FIC + MSC of one transmission frame of every ensemble in ONE call: dabgpu_fic_decode_frames on ring slot newest_frame_slot and
 * dabgpu_msc_decode_frames_layout on the ring, with the arguments and outputs of those two (identical bytes and result records).
 * Replaces BasicRadio::Process's fan-out of a frame to its FIC runner and its MSC runners (src/basic_radio/basic_radio.cpp:41-65).
 * When every sub-channel of the batch runs in a batch mapping (LANE / OCTET) the FIB groups are decoded INSIDE the MSC launch, as
 * further groups of codewords with their own puncturing schedule -- the MSC's groups rarely fill their last round of wavefront
 * slots, so the FIC then costs its gather only; otherwise the two run one after the other as if called separately.
 *   d_fib_bytes [n_ensembles][4][96], d_fic_results [n_ensembles][4]; d_msc_out / d_msc_results as in dabgpu_msc_decode_frames.
 */
int dabgpu_decode_frames_layout(dabgpu_ctx *ctx, const int8_t *d_bits_history, size_t n_ensembles, size_t ensemble_stride,
                                int history_frames, int newest_frame_slot, const dabgpu_subchannel *h_subchannels, int n_subchannels,
                                uint8_t *d_fib_bytes, dabgpu_codeword_result *d_fic_results, uint8_t *d_msc_out,
                                size_t out_ensemble_stride, dabgpu_codeword_result *d_msc_results, int tie_rule, int bits_layout,
                                void *stream);

/* Which mapping the MSC of `n_ensembles` ensembles carrying this multiplex takes right now -- the context's setting (dabgpu_viterbi_set_mapping) or,
 * under DABGPU_VIT_MAP_AUTO, the cost model's choice (one mapping for all sub-channels of a call) -- and the modelled times of WAVE / LANE / OCTET in
 * microseconds (model_us3 may be NULL).  Host only: launches nothing. */
int dabgpu_multiplex_mapping(dabgpu_ctx *ctx, size_t n_ensembles, const dabgpu_subchannel *h_subchannels, int n_subchannels, int *mapping,
                             double *model_us3);

/* Ring forms: ensemble e decodes the frame in slot d_newest_slot[e] of its own frame-history ring d_hist + e*ensemble_stride
 * (each ensemble at its own ring position, as dabgpu_stream_bank_process_ring leaves them); a negative slot skips the ensemble
 * (its result records come back with n_out_bytes = 0).  FIB bytes [n_ensembles][4][96], results [n_ensembles][4]. */
int dabgpu_fic_decode_ring(dabgpu_ctx *ctx, const int8_t *d_hist, size_t n_ensembles, size_t ensemble_stride,
                           const int32_t *d_newest_slot, uint8_t *d_fib_bytes, dabgpu_codeword_result *d_results, int tie_rule,
                           void *stream);
int dabgpu_msc_decode_ring(dabgpu_ctx *ctx, const int8_t *d_hist, size_t n_ensembles, size_t ensemble_stride, int history_frames,
                           const int32_t *d_newest_slot, const dabgpu_subchannel *subchannels, int n_subchannels, uint8_t *d_out,
                           size_t out_ensemble_stride, dabgpu_codeword_result *d_results, int tie_rule, void *stream);

/* dabgpu_decode_frames_layout for rings (dabgpu_fic_decode_ring + dabgpu_msc_decode_ring_layout in one call) */
int dabgpu_decode_ring_layout(dabgpu_ctx *ctx, const int8_t *d_hist, size_t n_ensembles, size_t ensemble_stride, int history_frames,
                              const int32_t *d_newest_slot, const dabgpu_subchannel *subchannels, int n_subchannels,
                              uint8_t *d_fib_bytes, dabgpu_codeword_result *d_fic_results, uint8_t *d_msc_out, size_t out_ensemble_stride,
                              dabgpu_codeword_result *d_msc_results, int tie_rule, int bits_layout, void *stream);

/* msc_decode_ring for rings whose MSC part is in `bits_layout` (dabgpu_stream_bank_process_ring_layout) */
int dabgpu_msc_decode_ring_layout(dabgpu_ctx *ctx, const int8_t *d_hist, size_t n_ensembles, size_t ensemble_stride, int history_frames,
                                  const int32_t *d_newest_slot, const dabgpu_subchannel *subchannels, int n_subchannels, uint8_t *d_out,
                                  size_t out_ensemble_stride, dabgpu_codeword_result *d_results, int tie_rule, int bits_layout,
                                  void *stream);

/* ------------------------------------------------------------------------------------------------
 * Single-stream, host-buffer, synchronous forms used by the C++ mirror classes (one codeword per call).
 */
/* one FIB group: FIC_Decoder::DecodeFIBGroup (src/dab/fic/fic_decoder.cpp:53-117) */
int dabgpu_fic_decode_group_host_sync(dabgpu_ctx *ctx, const int8_t *h_bits /*[2304]*/, uint8_t *h_bytes /*[96]*/,
                                      uint32_t *crc_ok_mask, uint64_t *path_error, int tie_rule);
/* DAB_Viterbi_Decoder reset/update.../chainback collapsed into one call: h_src holds the punctured soft bits of all
 * segments back to back (src/dab/algorithms/dab_viterbi_decoder.cpp:109-129) */
int dabgpu_viterbi_decode_host_sync(dabgpu_ctx *ctx, const int8_t *h_src, size_t n_src, const uint32_t *seg_pi4,
                                    const uint32_t *seg_steps4, uint32_t start_state, uint32_t end_state, uint32_t flags,
                                    uint8_t *h_out, size_t n_out_bytes, uint64_t *path_error, int tie_rule);

/* The general form of DAB_Viterbi_Decoder -- reset(start_state), update(...) any number of times with ANY puncture vector and ANY
 * requested_output_symbols, chainback(bytes_out, end_state) (src/dab/algorithms/dab_viterbi_decoder.cpp:109-181) -- collapsed into one call:
 * the caller de-punctures as it goes (kept symbols copied, punctured positions 0: :154-176) and hands over the mother code.
 *   h_mother     [4 * n_steps] int8, 1 <= n_steps <= DABGPU_MAX_TRELLIS_STEPS = trellis steps since reset()
 *   n_out_bytes  bytes chainback() is asked for: its bits n_out_bytes * 8 - 1 .. 0 are traced back from decision word n_out_bytes * 8 + 5
 *                downwards, starting in end_state (the core's chainback behind :126); n_out_bytes * 8 + 6 <= n_steps (a trace-back that
 *                starts beyond the decoded steps reads decision words the reference never wrote in this run: DABGPU_ERR_INVALID_ARG)
 *   path_error   accumulated renormalisation + metric[end_state] after ALL n_steps steps (:127-128), may be NULL.  (The reference calls the
 *                core's get_error() WITHOUT an argument, dab_viterbi_decoder.cpp:127; which state that reads by default is defined in
 *                vendor/viterbi_decoder, an empty submodule here.  Every in-tree caller chains back from end_state 0, where metric[end_state]
 *                and metric[0] are the same number; for other end states the two readings may differ -- unpinned, like the oracle's.)
 * When the trace-back does not start at the last decoded step the forward pass runs twice (whole length for the path error, the prefix
 * for the bytes): the decisions of a prefix do not depend on what follows. */
int dabgpu_viterbi_decode_depunctured_host_sync(dabgpu_ctx *ctx, const int8_t *h_mother, size_t n_steps, uint32_t start_state,
                                                uint32_t end_state, uint8_t *h_out, size_t n_out_bytes, uint64_t *path_error, int tie_rule);

/* per-sub-channel stream: a 16-slot device ring of the sub-channel's slice of every CIF + its protection plan.
 * Replaces MSC_Decoder + CIF_Deinterleaver state (src/dab/msc/msc_decoder.cpp:26-75, cif_deinterleaver.cpp:13-34). */
typedef struct dabgpu_msc_stream dabgpu_msc_stream;
int dabgpu_msc_stream_create(dabgpu_ctx *ctx, const dabgpu_subchannel *sc, dabgpu_msc_stream **out);
void dabgpu_msc_stream_destroy(dabgpu_msc_stream *s);
/* CIF_Deinterleaver::Consume: h_bits = length*64 soft bits of this sub-channel from one CIF */
int dabgpu_msc_stream_push_cif(dabgpu_msc_stream *s, const int8_t *h_bits);
/* CIF_Deinterleaver::Deinterleave: DABGPU_ERR_NOT_READY until 16 CIFs were pushed */
int dabgpu_msc_stream_deinterleave_sync(dabgpu_msc_stream *s, int8_t *h_out);
/* Deinterleave + DecodeEEP/DecodeUEP of the logical frame completed by the last push; *n_out = decoded bytes.
 * DABGPU_ERR_NOT_READY (and *n_out = 0) until 16 CIFs were pushed (msc_decoder.cpp:60-63) */
int dabgpu_msc_stream_decode_sync(dabgpu_msc_stream *s, uint8_t *h_out, size_t *n_out, uint64_t *path_error, int tie_rule);

/* --------------------------------------------------------------------------------------------------
 * Frame session: one batched decode per transmission frame behind the single-stream classes.
 * BasicRadio::Process fans a frame out to one FIC runner and one MSC runner per sub-channel (src/basic_radio/basic_radio.cpp:41-65),
 * each of which calls its decoder once per FIB group / CIF -- 4 + 4 x sub-channels synchronous round trips per frame.  A session keeps
 * the last 8 frames of soft bits on the device: push_frame copies a frame in ONCE and launches the FIC decode (4 FIB groups) and the
 * time de-interleave + Viterbi + descramble of every registered sub-channel for the frame's 4 CIFs (the batch entry points above with
 * one ensemble), asynchronously; the results of the last 8 frames stay available in host memory and are fetched by
 * (generation, group / sub-channel, CIF).  The mirror classes use it through dab-radio_amd/host/dab/dabgpu_frame_batcher.h, which
 * also decides when a class may take a session result instead of decoding itself (the bytes are identical either way).
 * Thread-safe.  The session owns a device context of its own.
 */
typedef struct dabgpu_frame_session dabgpu_frame_session;
int dabgpu_frame_session_create(dabgpu_frame_session **out, int device);
void dabgpu_frame_session_destroy(dabgpu_frame_session *s);
/* replaces the set of sub-channels decoded for the frames pushed from now on (n <= 64) */
int dabgpu_frame_session_set_subchannels(dabgpu_frame_session *s, const dabgpu_subchannel *h_subchannels, int n);
/* h_bits = the 230400 soft bits of one frame (layout of On_OFDM_Frame()); *generation counts the frames pushed, from 0 */
int dabgpu_frame_session_push_frame(dabgpu_frame_session *s, const int8_t *h_bits, int decode_fic, int tie_rule, uint64_t *generation);
/* DABGPU_ERR_NOT_READY: that generation is gone (more than 8 frames old), was pushed without the FIC / without this sub-channel */
int dabgpu_frame_session_fetch_fib_group(dabgpu_frame_session *s, uint64_t generation, int group, uint8_t *h_bytes /*[96]*/,
                                         uint32_t *crc_ok_mask, uint64_t *path_error);
int dabgpu_frame_session_fetch_cif(dabgpu_frame_session *s, uint64_t generation, const dabgpu_subchannel *sc, int cif,
                                   uint8_t *h_bytes, size_t capacity, size_t *n_bytes, uint64_t *path_error);

/* --------------------------------------------------------------------------------------------------
 * Receiver pipeline: one receiver's per-frame device work without a host wait in between.
 * Replaces the hand-over between OFDM_Demod's reader thread, its coordinator / pipeline threads and the observers that decode the frame
 * (src/ofdm/ofdm_demodulator.cpp:550-577 double buffer + WaitEnd / SignalStart, :581-639 CoordinatorThread; src/basic_radio/basic_radio.cpp:41-65).
 * The OFDM_Demod mirror class is built on it (dab-radio_amd/host/ofdm/ofdm_demodulator.cpp): its reader side buffers samples into a
 * pinned staging buffer and submits, a delivery thread waits for frames and calls the observers.
 *
 *   staging buffer   dabgpu_receiver_stage(): page-locked host memory the caller assembles "NULL symbol | frame" in, as complex float;
 *                    capacity = nb_null_period + (nb_fft - nb_cyclic_prefix) + samples per frame.  dabgpu_receiver_submit_frame moves on to
 *                    the next of three buffers; the one just submitted stays readable (the caller copies the frame's trailing NULL symbol
 *                    out of it for the next correlation window, ofdm_demodulator.cpp:558-562).
 *   frequency state  m_freq_coarse_offset / m_freq_fine_offset / m_is_found_coarse_freq_offset live on the DEVICE: submit_sync runs
 *                    RunCoarseFreqSync + RunFineTimeSync (:360-548) on them, submit_frame demodulates with their sum (:672) and applies the
 *                    frame's fine-frequency update (:606-618, :829-840), dabgpu_receiver_reset zeroes them (:277-289) -- all in submission
 *                    order on one stream, so frame k + 1's synchroniser sees frame k's update without the host having seen it.
 *   decode           frames of a mode I receiver are demodulated straight into the 8-frame history of a frame session
 *                    (dabgpu_receiver_session; see "Frame session" above) and decoded there on a second stream -- the FIC when
 *                    decode_fic, the sub-channels given -- the results fetched with dabgpu_frame_session_fetch_* by generation.
 * Threads: submit_* / stage / reset / set_subchannels / wait_sync from ONE thread (the reader); wait_frame from one other (or the same).
 * At most 7 frames may be submitted and not yet collected with wait_frame (the result slots are a ring of 8).
 */
/*
 * BANKED receivers (ABI 4): dabgpu_receiver_create_banked makes a mode I receiver on the library's own tables that is a member of the device's
 * RECEIVER BANK.  Its interface is the one below, unchanged; its submit_* calls post the work, and one thread per device issues what all members
 * have posted since its last round as ONE synchroniser launch, ONE demodulation launch over a compact batch of the posted frames and ONE FIC + MSC
 * decode over the members' history rings (at most one job per member and round, in posting order: frame k's fine-frequency update still
 * precedes frame k + 1's synchroniser).  A member uploads its frame itself when it posts it (the samples cross PCIe while earlier rounds run); at most
 * two rounds are under way (DABGPU_BANK_ROUNDS), what is posted meanwhile forms the next one -- its size follows the load.  N OFDM_Demod objects of a
 * process then cost ~4 runtime calls per frame and member + ~15 per round instead of ~20 per frame on three streams each (csrc/receiver_bank.hip;
 * DESIGN.md 4.11b).  Outputs are those of the private pipeline, bit for bit.
 * The sub-channel list (dabgpu_receiver_set_subchannels) is the BANK's: the members report one list (the decoders' subscription is process-wide in
 * the classes above); it applies to the rounds enqueued after the call.  A round decodes what it demodulates: frames are posted with dabgpu_receiver_submit_frame (which carries the
 * core model); the two-call form dabgpu_receiver_submit_demod / _submit_decode returns DABGPU_ERR_UNSUPPORTED.  Up to 64 members per device.
 */
typedef struct dabgpu_receiver dabgpu_receiver;
typedef struct {
    uint64_t generation;
    const int8_t *bits;        /* the frame's soft bits, On_OFDM_Frame() layout, in page-locked memory of the receiver: valid until 7 more frames were submitted */
    size_t n_bits;
    float freq_fine;           /* m_freq_fine_offset after this frame's update */
    float total_phase;         /* sum of the frame's cyclic-prefix angles */
    const float *fft;          /* GetFrameFFT() [nb_frame_symbols + 1][nb_fft] complex, only when the frame was submitted with want_views */
    const float *dqpsk;        /* GetFrameDataVec() [nb_frame_symbols - 1][nb_data_carriers] complex, mode I + want_views */
} dabgpu_receiver_frame;
/* h_prs_fft_ref / h_carrier_mapper as for dabgpu_create (mode I; NULL = built-in tables; must be NULL in modes II-IV) */
int dabgpu_receiver_create(dabgpu_receiver **out, int device, int transmission_mode, const float *h_prs_fft_ref, const int *h_carrier_mapper);
int dabgpu_receiver_create_banked(dabgpu_receiver **out, int device);
void dabgpu_receiver_destroy(dabgpu_receiver *rx);
dabgpu_frame_session *dabgpu_receiver_session(dabgpu_receiver *rx);      /* owned by the receiver */
/* what is decoded for the frames submitted from now on (mode I; n <= 64) */
int dabgpu_receiver_set_subchannels(dabgpu_receiver *rx, const dabgpu_subchannel *h_subchannels, int n, int decode_fic);
/* the soft-decision policy of the frames submitted from now on (dabgpu_soft_cfg; the default is DABGPU_SOFT_NORMALISED).  DABGPU_SOFT_CSI:
 * a private mode I receiver only -- a banked receiver and modes II-IV answer DABGPU_ERR_UNSUPPORTED and keep the normalised soft bits */
int dabgpu_receiver_set_soft(dabgpu_receiver *rx, const dabgpu_soft_cfg *cfg);
int dabgpu_receiver_stage(dabgpu_receiver *rx, float **h_stage, size_t *capacity_samples);
int dabgpu_receiver_reset(dabgpu_receiver *rx);
/* PRS slot = nb_fft samples from sample prs_sample of the current staging buffer (m_correlation_time_buffer[nb_null_period ...]); asynchronous */
int dabgpu_receiver_submit_sync(dabgpu_receiver *rx, const dabgpu_sync_cfg *cfg, size_t prs_sample);
/* blocks until the record of the last submit_sync is in host memory: freq_coarse / freq_fine / is_found_coarse after the synchroniser,
 * fine_time_offset, sync_valid (0: the caller resets, :529-532); h_impulse / h_freq_response [nb_fft] dB, may be NULL */
int dabgpu_receiver_wait_sync(dabgpu_receiver *rx, dabgpu_sync_state *out, float *h_impulse, float *h_freq_response);
/* the frame = samples-per-frame samples from sample frame_sample of the current staging buffer (nb_null_period + fine_time_offset); asynchronous:
 * upload, demodulation, fine-frequency update with `beta`, decode, results to host memory.  *generation counts the frames submitted.
 * No synchroniser is required between two frames: up to R - 1 = 7 frames may be submitted one behind the other (each from the staging buffer that is
 * current then; every frame is demodulated with the fine-frequency word the frame before it left), on private and banked receivers alike.  A banked
 * receiver answers DABGPU_ERR_NOT_READY to a frame beyond 7 not yet delivered, and DABGPU_ERR_UNSUPPORTED once its bank was shut down. */
int dabgpu_receiver_submit_frame(dabgpu_receiver *rx, size_t frame_sample, float fine_freq_update_beta, int want_views, int tie_rule,
                                 uint64_t *generation);
/* The same in two calls, for two threads (what the OFDM_Demod mirror does): submit_demod enqueues the upload, the demodulation, the fine-frequency
 * update and the copies of what the host reads, and returns; submit_decode(generation) -- once per frame, in the order of the generations --
 * waits on the HOST until that frame is demodulated and then enqueues its decode.  No stream waits for another on the device (several receivers of
 * a process share hardware queues: a queue whose head waits holds back the other receiver's work behind it), and the thread that frames the stream
 * issues half the runtime calls.  At most 4 frames may be between the two calls (the decode of frame g reads the history slot frame g + 4 overwrites:
 * DABGPU_ERR_NOT_READY); dabgpu_receiver_wait_frame(g) only after submit_decode(g) has returned.  Replaces the same hand-over as above. */
int dabgpu_receiver_submit_demod(dabgpu_receiver *rx, size_t frame_sample, float fine_freq_update_beta, int want_views, uint64_t *generation);
int dabgpu_receiver_submit_decode(dabgpu_receiver *rx, uint64_t generation, int tie_rule);
int dabgpu_receiver_wait_frame(dabgpu_receiver *rx, uint64_t generation, dabgpu_receiver_frame *out);
/* the scale k (DABGPU_SOFT_CSI, dabgpu_soft_scale_host) of a frame dabgpu_receiver_wait_frame has delivered, while its result slot lasts;
 * 0 for a frame demodulated under DABGPU_SOFT_NORMALISED and for a banked receiver.  Feeds receive diversity (see "Receive diversity"). */
int dabgpu_receiver_frame_soft_scale(dabgpu_receiver *rx, uint64_t generation, float *scale);

/* ==================================================================================================
 * Transmission modes II, III and IV (geometries of src/ofdm/dab_ofdm_params_ref.cpp:11-60).
 * The same demodulation pipeline, frame-aligned batches, through a size-generic kernel (FFT 512 / 256 / 1024 with the mode I
 * butterflies and twiddle rule; PLL with apply_pll's scalar tail for symbol periods that are not a multiple of 4).  The DAB
 * layer above the soft bits exists for mode I only in the reference (fic_decoder.cpp:61-72), and here.
 */
/* out9 = {nb_frame_symbols, nb_symbol_period, nb_null_period, nb_fft, nb_cyclic_prefix, nb_data_carriers,
 *         samples per frame (symbols + NULL), soft bits per symbol, soft bits per frame}; host only */
int dabgpu_get_ofdm_params(int transmission_mode, int *out9);
/*   d_iq   [n_frames][samples per frame] complex float, layout as for mode I (symbols, PRS first, then the NULL symbol)
 *   d_bits [n_frames][soft bits per frame] int8, 16-byte aligned;  d_cp_corr [n_frames][nb_frame_symbols] complex float, may be NULL
 *   d_fft  [n_frames][nb_frame_symbols + 1][nb_fft] complex float, may be NULL.  transmission_mode 1 is accepted too
 *   (cross-check of the two kernels). */
int dabgpu_ofdm_demod_frames_mode(dabgpu_ctx *ctx, int transmission_mode, const float *d_iq, size_t n_frames,
                                  const float *d_freq_offset, int8_t *d_bits, float *d_cp_corr, float *d_fft, int symbols_per_block,
                                  void *stream);
int dabgpu_ofdm_phase_update_mode(dabgpu_ctx *ctx, int transmission_mode, const float *d_cp_corr, size_t n_frames,
                                  float fine_freq_update_beta, float *d_total_phase, float *d_fine_freq, void *stream);
/* PRS synchronisation (dabgpu_ofdm_sync) for any mode: d_prs_syms = nb_fft samples per stream; d_impulse / d_freq_response
 * [n_streams][nb_fft].  The PRS spectrum of the mode (get_DAB_PRS_reference, src/ofdm/dab_prs_ref.cpp:140-195) and the
 * coarse-sync reference are built on the context at first use. */
int dabgpu_ofdm_sync_mode(dabgpu_ctx *ctx, int transmission_mode, const float *d_prs_syms, size_t n_streams, size_t stride_samples,
                          const dabgpu_sync_cfg *cfg, dabgpu_sync_state *d_states, float *d_impulse, float *d_freq_response, void *stream);
/* single-stream host-buffer forms used by the OFDM_Demod mirror class in modes II-IV (h_fft [nb_frame_symbols+1][nb_fft]) */
int dabgpu_ofdm_demod_stream_frame_sync_mode(dabgpu_ctx *ctx, int transmission_mode, const float *h_iq, float freq_coarse,
                                             float *h_freq_fine, float fine_freq_update_beta, int8_t *h_bits, float *h_total_phase,
                                             float *h_fft);
int dabgpu_ofdm_sync_host_sync_mode(dabgpu_ctx *ctx, int transmission_mode, const float *h_prs_sym, const dabgpu_sync_cfg *cfg,
                                    dabgpu_sync_state *h_state, float *h_impulse, float *h_freq_response);

/* ==================================================================================================
 * Unsynchronised front end on the device: a bank of n independent receivers whose state between
 * calls -- signal level, NULL-search flags, circular NULL buffer, correlation window, frame buffer, frequency
 * offsets, counters (src/ofdm/ofdm_demodulator.h:131-176) -- lives in HBM.  One dabgpu_stream_bank_process() is one
 * OFDM_Demod::Process(block) for every stream (src/ofdm/ofdm_demodulator.cpp:235-275): L1 signal average (:934-950),
 * NULL power-dip search (:291-347), NULL+PRS read (:349-358), coarse/fine sync (:360-548), symbol read (:550-577),
 * frame demodulation and the fine-frequency loop (:581-639), Reset on a failed impulse-peak test (:277-289,:529-532).
 * Results equal the OFDM_Demod mirror class fed the same blocks, stream by stream, byte for byte.
 */
typedef struct {                      /* OFDM_Demod_Config, src/ofdm/ofdm_demodulator.h:24-45 */
    float signal_l1_update_beta;      /* 0.95 */
    int   signal_l1_nb_samples;       /* 100  */
    int   signal_l1_nb_decimate;      /* 5    */
    float thresh_null_start;          /* 0.35 */
    float thresh_null_end;            /* 0.75 */
    dabgpu_sync_cfg sync;
} dabgpu_stream_cfg;
void dabgpu_stream_cfg_default(dabgpu_stream_cfg *cfg);

typedef struct {
    int32_t state;                    /* OFDM_Demod::State, ofdm_demodulator.h:50-56 */
    float   signal_l1_average;
    float   freq_coarse, freq_fine;
    int32_t is_found_coarse;
    int32_t fine_time_offset;
    int32_t total_frames_read, total_frames_desync;
} dabgpu_stream_status;

typedef struct dabgpu_stream_bank dabgpu_stream_bank;
/* cfg NULL = the reference's defaults. Device memory: 1.64 MB per stream. */
int dabgpu_stream_bank_create(dabgpu_ctx *ctx, size_t n_streams, const dabgpu_stream_cfg *cfg, dabgpu_stream_bank **out);
/* the same for transmission mode 1..4 (get_DAB_OFDM_params, src/ofdm/dab_ofdm_params_ref.cpp:11-60): frames are
 * dabgpu_get_ofdm_params(mode)[8] soft bits each, ring / block limits scale with the mode's frame length; modes II-IV run the
 * size-generic demodulation kernel (dabgpu_ofdm_demod_frames_mode) */
int dabgpu_stream_bank_create_mode(dabgpu_ctx *ctx, int mode, size_t n_streams, const dabgpu_stream_cfg *cfg, dabgpu_stream_bank **out);
void dabgpu_stream_bank_destroy(dabgpu_stream_bank *bank);
int dabgpu_stream_bank_reset(dabgpu_stream_bank *bank, void *stream);     /* every stream back to its constructed state */
/*
 *   d_iq        stream s's block = n_samples complex float at d_iq + 2*s*stream_stride_samples (device, 8-byte aligned)
 *   d_bits      [n_streams][max_frames_per_stream][230400] int8: frame j completed by stream s during this call
 *   d_n_frames  [n_streams] out: frames completed during this call (may be NULL)
 *   max_frames_per_stream >= n_samples / 191400 + 2
 * Launches on `stream`; synchronises with it (the number of rounds depends on the data).
 */
int dabgpu_stream_bank_process(dabgpu_stream_bank *bank, const float *d_iq, size_t stream_stride_samples, size_t n_samples,
                               int8_t *d_bits, size_t max_frames_per_stream, int32_t *d_n_frames, void *stream);
/* The same from blocks still in a capture format (dabgpu_iq_format): d_raw holds n_samples IQ pairs per stream, stream s at
 * byte offset s * stream_stride_samples * sample_bytes.  raw_u8 / raw_s8 / raw_s16l (and wav PCM8 / PCM16 / float32) blocks are
 * read by the bank's kernels themselves -- level windows, NULL search, buffering and the demodulator's frame tails dequantise
 * on the fly with the reader arithmetic, 2-4 bytes per sample instead of 8 and no conversion pass; any other format is first
 * dequantised (dabgpu_iq_convert) into bank-owned scratch (then d_raw and the byte offset between streams must be multiples of 16). */
int dabgpu_stream_bank_process_raw(dabgpu_stream_bank *bank, const void *d_raw, int format, size_t stream_stride_samples,
                                   size_t n_samples, int8_t *d_bits, size_t max_frames_per_stream, int32_t *d_n_frames, void *stream);
/*
 * Retained blocks: dabgpu_stream_bank_process_raw for callers that keep a block's device memory valid and unchanged until the NEXT call
 * has returned -- a ring of device buffers (dabgpu_ingest_* with depth >= 2 is one).  OFDM_Demod::Process copies every sample it is
 * handed into its frame buffer (ofdm_demodulator.cpp:550-577); the bank already reads completed frames where they lie and copies only
 * the unfinished frame at a block's end; here that copy goes too: the next call's demodulator reads the frame's head from d_prev_raw,
 * its tail from d_raw.  Same frames, same state, bit for bit.
 *   d_prev_raw  the block of the previous retained call (same format and stride), NULL at the first call / after a release or reset
 *   format      one the kernels read directly: raw_f32l, raw_u8, raw_s8, raw_s16l, wav PCM8 / PCM16 / float32; mode I banks (banks of
 *               other modes process the call like dabgpu_stream_bank_process_raw)
 * A block shorter than a frame first copies what the previous block still holds (a frame then spans more than two blocks).
 * After a retained call the bank refuses any other process call until dabgpu_stream_bank_release (copies the carried samples out of the
 * last block, which may then be freed) or dabgpu_stream_bank_reset.
 */
int dabgpu_stream_bank_process_retained(dabgpu_stream_bank *bank, const void *d_raw, int format, size_t stream_stride_samples,
                                        size_t n_samples, const void *d_prev_raw, int8_t *d_bits, size_t max_frames_per_stream,
                                        int32_t *d_n_frames, void *stream);
int dabgpu_stream_bank_release(dabgpu_stream_bank *bank, const void *d_prev_raw, int format, size_t stream_stride_samples, void *stream);

/* Ring form for a device-resident pipeline: a completed frame of stream s is written to slot (frames demodulated so far) mod
 * hist_frames of d_hist [n_streams][hist_frames][230400] -- the per-ensemble frame-history ring dabgpu_fic_decode_ring /
 * dabgpu_msc_decode_ring read -- and d_newest_slot[s] receives that slot, or -1 when the stream completed no frame in this
 * call.  At most 191400 samples per call (so that a stream completes at most one frame); format must be one the kernels read
 * directly (raw_f32l, raw_u8, raw_s8, raw_s16l, wav PCM8/PCM16/float32). */
int dabgpu_stream_bank_process_ring(dabgpu_stream_bank *bank, const void *d_raw, int format, size_t stream_stride_samples,
                                    size_t n_samples, int8_t *d_hist, int hist_frames, int32_t *d_newest_slot, void *stream);
/* the same with the MSC part of every frame stored in `bits_layout` (DABGPU_BITS_NATURAL / DABGPU_BITS_MSC_CLASSED, see
 * dabgpu_ofdm_demod_frames_history; mode I banks) -- read the rings with dabgpu_fic_decode_ring + dabgpu_msc_decode_ring_layout */
int dabgpu_stream_bank_process_ring_layout(dabgpu_stream_bank *bank, const void *d_raw, int format, size_t stream_stride_samples,
                                           size_t n_samples, int8_t *d_hist, int hist_frames, int32_t *d_newest_slot,
                                           int bits_layout, void *stream);
/* The ring form with retained blocks (dabgpu_stream_bank_process_retained's contract: d_raw stays valid and unchanged until the NEXT call has
 * returned; d_prev_raw = the previous call's block, NULL at the first call / after a release or reset): the unfinished frame at the end of a
 * block stays where it is and the next call's demodulator reads it there -- in the ring form, whose blocks are shorter than a frame, the copy
 * it saves is half a frame per stream and call on average (and a u8 -> complex float expansion).  A frame that began in the last samples of a
 * block and cannot complete in the next one has those few samples copied at the start of the next call.  Same frames, same state, bit for bit. */
int dabgpu_stream_bank_process_ring_retained(dabgpu_stream_bank *bank, const void *d_raw, int format, size_t stream_stride_samples,
                                             size_t n_samples, const void *d_prev_raw, int8_t *d_hist, int hist_frames,
                                             int32_t *d_newest_slot, int bits_layout, void *stream);
/* the soft-decision policy of every frame the bank demodulates from the next process call on (any of the six forms); default
 * DABGPU_SOFT_NORMALISED.  d_soft_scale (may be NULL): scale_capacity floats on the device; the scale k of the frame written to
 * bits slot j of stream s goes to d_soft_scale[s * max_frames_per_stream + j] (ring forms: s * hist_frames + ring slot) -- the
 * numbering of that call's d_bits / d_hist; a call with n_streams * max_frames_per_stream (hist_frames) > scale_capacity is refused
 * before anything is launched.  Kept across dabgpu_stream_bank_reset, like the bank's configuration.  Mode I banks; a bank of
 * modes II-IV answers DABGPU_ERR_UNSUPPORTED with a reason and keeps the normalised policy.  Synchronises with nothing.
 * Under DABGPU_SOFT_NORMALISED every process call is what it is without this call, and d_soft_scale is never written.  The policy may
 * change between two retained calls: it belongs to the frame that completes, not to the block in which the frame began.  The bank's
 * state machine (level, NULL search, synchroniser, fine-frequency loop) never reads a soft bit: the policy changes no frame count, no
 * frame position and no status field, only the bits. */
int dabgpu_stream_bank_set_soft(dabgpu_stream_bank *bank, const dabgpu_soft_cfg *cfg, float *d_soft_scale, size_t scale_capacity);
int dabgpu_stream_bank_get_soft(const dabgpu_stream_bank *bank, dabgpu_soft_cfg *cfg);
/* The DQPSK products and a sync record of every frame the frames forms complete (dabgpu_stream_bank_process, _process_raw with the fused
 * loaders and the converted path, _process_retained), beside its soft bits: what dabgpu_ofdm_sync_demod_frames_branch writes for frames in
 * aligned slices, from unsynchronised streams.  d_dqpsk [capacity_frames][75][1536] complex float, 16-byte aligned, d_records
 * [capacity_frames], 4-byte aligned; both together, both NULL switches the feature off.  Both are indexed by bits slot, the numbering of
 * d_bits and of set_soft's d_soft_scale: the frame written to bits slot j of stream s is at s * max_frames_per_stream + j.  With the
 * bank's d_soft_scale the three arrays are a dabgpu_diversity_branch as they stand (d_dqpsk, d_scale, d_sync), and d_dqpsk with d_records
 * is the (d_dqpsk, d_sync) pair of dabgpu_dd_profile_frames, dabgpu_sym_profile_frames, dabgpu_clock_estimate_frames and
 * dabgpu_clock_derotate_frames: no copy.
 *   While products are set a frames-form call first zeroes the records of all its n_streams * max_frames_per_stream slots on the caller's
 * stream (sync_valid = 0); every completed frame then writes its products -- bit for bit the d_dqpsk view of dabgpu_ofdm_demod_frames_soft
 * on the assembled frame at the frequency the demodulator used -- and its record: sync_valid = 1, fine_time_offset, freq_coarse and
 * is_found_coarse the stream's when the frame was handed to the demodulator, freq_fine the fine word BEFORE this frame's phase update
 * (float(freq_coarse + freq_fine) is the word the demodulator used), reserved = 0.  A slot without a frame keeps its old products and has
 * a zero record; a frame beyond the caller's capacity lands in the last slot, as the bits do: products, record, scale and bits of that
 * slot belong to the same frame.  Bits, scale words, frame counts and every status field are those of the same bank without products.
 *   Refused while products are set, before anything is launched or converted (no output is touched, no state moves): the ring forms
 * (DABGPU_ERR_UNSUPPORTED); a process call under DABGPU_SOFT_NORMALISED, or without a scale buffer (the consumers need the frame's scale),
 * or with n_streams * max_frames_per_stream > capacity_frames (DABGPU_ERR_INVALID_ARG).
 *   Synchronises with nothing; the bank keeps the addresses; kept across dabgpu_stream_bank_reset.  Mode I banks: a bank of modes II-IV
 * answers DABGPU_ERR_UNSUPPORTED and stays off. */
int dabgpu_stream_bank_set_products(dabgpu_stream_bank *bank, float *d_dqpsk, dabgpu_sync_state *d_records, size_t capacity_frames);
int dabgpu_stream_bank_get_products(const dabgpu_stream_bank *bank, float **d_dqpsk, dabgpu_sync_state **d_records, size_t *capacity_frames);
/* snapshot of every stream's getters (GetState, GetSignalAverage, Get*FrequencyOffset, ...) into host memory; synchronous */
int dabgpu_stream_bank_status(dabgpu_stream_bank *bank, dabgpu_stream_status *h_status, void *stream);

/* ==================================================================================================
 * DAB+ outer code on the device: AAC_Frame_Processor between the channel decoder's bytes and the AAC
 * access units (src/dab/audio/aac_frame_processor.cpp:127-361): super-frame acquisition on the fire code, collection of 5
 * logical frames, RS(120,110) decoding of the interleaved columns (src/dab/algorithms/reed_solomon_decoder.cpp), fire code
 * of the corrected super frame, header walk and access-unit CRCs, re-acquisition after 10 failed super frames.  One
 * wavefront per stream (an (ensemble, sub-channel) pair); acquisition state and the super frame under collection stay in
 * HBM between calls.  Logical frames of 11..1536 bytes (every DAB+ sub-channel up to 512 kbit/s).
 */
typedef struct {
    int32_t rs_failed_index;        /* -1, or the first uncorrectable RS codeword (OnRSError, :336-341): super frame dropped */
    int32_t rs_corrected;           /* symbols reported corrected by the codewords decoded */
    int32_t firecode_ok;            /* fire code of the corrected super frame (:206-209) */
    int32_t header_valid;           /* OnSuperFrameHeader fired; the fields below are meaningful */
    int32_t descriptor;             /* byte 2: rfa | dac_rate | sbr_flag | aac_channel_mode | ps_flag | mpeg_surround_config(3) */
    int32_t num_aus;
    int32_t au_start[8];            /* byte offsets au_start[0..num_aus] inside the super frame (:266-283) */
    int32_t au_walk_stopped_at;     /* -1, or the access unit whose bounds test ended the walk (:291-297) */
    uint32_t au_crc_ok_mask;        /* bit i: OnAccessUnit(i) fired (CRC passed); other walked units: OnAccessUnitCRCError */
    int32_t frame_index;            /* index inside this call of the logical frame that completed the super frame */
    uint32_t firecode_rx_calc;      /* received << 16 | calculated fire code of the corrected super frame (OnFirecodeError arguments) */
    uint16_t au_crc_calc[6];        /* calculated CRC of every walked access unit (OnAccessUnitCRCError arguments) */
    uint16_t reserved[2];
} dabgpu_superframe_result;

typedef struct dabgpu_dabplus_bank dabgpu_dabplus_bank;
int dabgpu_dabplus_bank_create(dabgpu_ctx *ctx, size_t n_streams, dabgpu_dabplus_bank **out);
void dabgpu_dabplus_bank_destroy(dabgpu_dabplus_bank *bank);
int dabgpu_dabplus_bank_reset(dabgpu_dabplus_bank *bank, void *stream);
/*
 * n_frames x AAC_Frame_Processor::Process per stream.  Logical frame f of stream s = d_frame_bytes[s] bytes at
 * d_frames + d_stream_offsets[s] + f*frame_stride_bytes (the layout dabgpu_msc_decode_frames writes: offset of the
 * sub-channel inside one CIF record, stride of a CIF record).
 *   d_superframes [n_streams][max_superframes][superframe_stride_bytes]: every super frame ATTEMPTED in this call (5 frames
 *                 collected), corrected where RS succeeded;  d_results the matching records
 *   d_counts      [n_streams][4]: super frames attempted, logical frames dropped while waiting for a valid fire code,
 *                 received << 16 | calculated fire code of the last dropped frame, logical frames collected so far
 *   max_superframes >= ceil(n_frames / 5), superframe_stride_bytes >= 5 * frame bytes
 * Limits, reported per stream instead of being skipped in silence: a stream whose logical frames exceed 1536 bytes (the reference
 * takes any N >= 11, aac_frame_processor.cpp:129-137) is not processed and gets d_counts[s][1] = -1; a stream whose
 * 5 * frame bytes exceed superframe_stride_bytes gets d_counts[s][1] = -2.  (dabgpu_dabplus_process_frame_host_sync returns
 * DABGPU_ERR_UNSUPPORTED for the first case.)
 */
int dabgpu_dabplus_bank_process(dabgpu_dabplus_bank *bank, const uint8_t *d_frames, const uint64_t *d_stream_offsets,
                                size_t frame_stride_bytes, const uint32_t *d_frame_bytes, int n_frames, uint8_t *d_superframes,
                                size_t superframe_stride_bytes, dabgpu_superframe_result *d_results, int max_superframes,
                                int32_t *d_counts, void *stream);
/* the same, skipping every stream whose flag d_active[s / streams_per_flag] is negative (e.g. the newest-slot array of
 * dabgpu_stream_bank_process_ring with streams ordered ensemble-major: streams_per_flag = DAB+ sub-channels per ensemble) */
int dabgpu_dabplus_bank_process_masked(dabgpu_dabplus_bank *bank, const uint8_t *d_frames, const uint64_t *d_stream_offsets,
                                       size_t frame_stride_bytes, const uint32_t *d_frame_bytes, int n_frames, uint8_t *d_superframes,
                                       size_t superframe_stride_bytes, dabgpu_superframe_result *d_results, int max_superframes,
                                       int32_t *d_counts, const int32_t *d_active, int streams_per_flag, void *stream);
/* one Process(buf) of a one-stream bank with host buffers (the AAC_Frame_Processor mirror class); h_superframe [5*n_bytes] */
int dabgpu_dabplus_process_frame_host_sync(dabgpu_dabplus_bank *bank, const uint8_t *h_frame, uint32_t n_bytes, int *superframe_done,
                                           int *firecode_wait_failed, uint32_t *firecode_wait_rx_calc /* may be NULL */,
                                           dabgpu_superframe_result *h_result, uint8_t *h_superframe);

/* ==================================================================================================
 * Data formats either side of the path.
 *
 * IQ input: the reference's readers (examples/app_helpers/app_iq_readers.h:17-159, app_wav_reader.h:257-470)
 * turn a byte stream into std::complex<float>; here the raw bytes go to the device as they are and one
 * kernel applies the same arithmetic:
 *   quantised integers (app_iq_readers.h:19-44,79-84): (float(v) - BIAS) * (1.0f/MAX_AMPLITUDE), BIAS = 0 and
 *     MAX_AMPLITUDE = float(max) for signed T; BIAS = MAX_AMPLITUDE = float(max/2) + 0.5f for unsigned T;
 *   raw_f32*: bit copy (after the byte swap); raw_f64*: (float)double;
 *   wav: PCM8 (v-127.5f)*(1/127.5f), PCM16 v*(1/32767.f), PCM24 v*(1/8388607.f), PCM32 v*(1/float(INT32_MAX)),
 *     IEEE float 32/64, G.711 A-law / mu-law (app_wav_reader.h:271-456).
 * Soft/hard bit files: examples/app_helpers/app_viterbi_convert_block.h:12-44 (bit i of a byte, LSB first,
 * <-> soft bit +127 / -127; hard = soft >= 0).
 */
typedef enum {
    DABGPU_IQ_RAW_U8 = 0, DABGPU_IQ_RAW_S8,
    DABGPU_IQ_RAW_S16L, DABGPU_IQ_RAW_S16B, DABGPU_IQ_RAW_U16L, DABGPU_IQ_RAW_U16B,
    DABGPU_IQ_RAW_S32L, DABGPU_IQ_RAW_S32B, DABGPU_IQ_RAW_U32L, DABGPU_IQ_RAW_U32B,
    DABGPU_IQ_RAW_F32L, DABGPU_IQ_RAW_F32B, DABGPU_IQ_RAW_F64L, DABGPU_IQ_RAW_F64B,
    DABGPU_IQ_WAV_PCM8, DABGPU_IQ_WAV_PCM16, DABGPU_IQ_WAV_PCM24, DABGPU_IQ_WAV_PCM32,
    DABGPU_IQ_WAV_F32, DABGPU_IQ_WAV_F64, DABGPU_IQ_WAV_ALAW, DABGPU_IQ_WAV_MULAW,
    DABGPU_IQ_NB_FORMATS
} dabgpu_iq_format;

/* mode strings of app_iq_readers.h:107-113 ("raw_u8" ... "raw_f64b") -> dabgpu_iq_format; "wav" and unknown
 * strings return -1 (a wav file's format comes from dabgpu_wav_parse_header). Host only, needs no device. */
int dabgpu_iq_format_from_mode(const char *mode);
/* bytes of one IQ sample (two components) in the given format, 0 for an invalid format. Host only. */
size_t dabgpu_iq_format_sample_bytes(int format);

typedef struct {
    int32_t  iq_format;             /* dabgpu_iq_format of the sample data (DABGPU_IQ_WAV_*) */
    uint16_t audio_format;          /* 1 PCM, 3 IEEE float, 6 A-law, 7 mu-law (after resolving WAVE_FORMAT_EXTENSIBLE) */
    uint16_t total_channels;
    uint32_t samples_per_second;
    uint32_t average_bytes_per_second;
    uint16_t data_block_align_bytes;
    uint16_t bits_per_sample;
    uint32_t data_chunk_size;       /* bytes */
    uint64_t data_chunk_offset;     /* byte offset of the sample data from the start of the file */
} dabgpu_wav_header;
/* wav_read_header (app_wav_reader.h:107-255) over the first n_bytes of a file held in memory; accepts what it
 * accepts (fmt chunk of 16/18/40 bytes, 1 or 2 channels, fact chunk required for non-PCM, non-data chunks skipped)
 * and rejects what it or WavFileReader's constructor rejects (DABGPU_ERR_INVALID_ARG + dabgpu_last_error()).
 * get_iq_file_reader_from_mode_string additionally requires total_channels == 2 (app_iq_readers.h:122-126): callers
 * feeding dabgpu_iq_convert check that. Host only, needs no device. */
int dabgpu_wav_parse_header(const uint8_t *bytes, size_t n_bytes, dabgpu_wav_header *out);

/* d_raw: n_samples IQ pairs in `format` on the device (16-byte aligned); d_iq: n_samples interleaved (re, im) floats */
int dabgpu_iq_convert(dabgpu_ctx *ctx, const void *d_raw, int format, size_t n_samples, float *d_iq, void *stream);
int dabgpu_iq_convert_host_sync(dabgpu_ctx *ctx, const void *h_raw, int format, size_t n_samples, float *h_iq);

/* convert_viterbi_bits_to_bytes (app_viterbi_convert_block.h:28-44): n_bytes output bytes from 8*n_bytes soft bits */
int dabgpu_soft_bits_to_hard_bytes(dabgpu_ctx *ctx, const int8_t *d_bits, size_t n_bytes, uint8_t *d_bytes, void *stream);
/* convert_viterbi_bytes_to_bits (app_viterbi_convert_block.h:12-26) */
int dabgpu_hard_bytes_to_soft_bits(dabgpu_ctx *ctx, const uint8_t *d_bytes, size_t n_bytes, int8_t *d_bits, void *stream);
int dabgpu_soft_bits_to_hard_bytes_host_sync(dabgpu_ctx *ctx, const int8_t *h_bits, size_t n_bytes, uint8_t *h_bytes);
int dabgpu_hard_bytes_to_soft_bits_host_sync(dabgpu_ctx *ctx, const uint8_t *h_bytes, size_t n_bytes, int8_t *h_bits);

/* ------------------------------------------------------------------------------------------------------------------------------
 * OFDM transmitter (src/ofdm/ofdm_modulator.cpp:49-156; examples/simulate_transmitter.cpp:167-178 for the u8 form).
 * n_frames independent frames of `transmission_mode` (1..4), each NULL first in transmission order: nb_null_period +
 * nb_symbol_period * nb_frame_symbols samples (dabgpu_get_ofdm_params(mode)[6]), exactly OFDM_Modulator::ProcessBlock's output.
 * Every frame starts its DQPSK chain from the PRS (ofdm_modulator.cpp:73-76).
 *   d_payload  [n_frames][(nb_frame_symbols - 1) * nb_data_carriers / 4] bytes in layout `payload_layout`:
 *     DABGPU_TX_PAYLOAD_REFERENCE   OFDM_Modulator's input: natural carrier order, 2 bits per carrier LSB first, PHASE_MAP
 *                                   {(-A,-A), (A,-A), (A,A), (-A,A)}, A = 1/sqrt(2) (ofdm_modulator.cpp:95-156)
 *     DABGPU_TX_PAYLOAD_FRAME_BITS  the frame's hard bits as dabgpu_soft_bits_to_hard_bytes writes them (bit i -> byte i/8, bit i%8), in the
 *                                   demodulator's de-interleaved order: bit n of a symbol sets the real part of carrier mapper[n], bit n + NC
 *                                   its imaginary part, z = ((1 - 2 b_n) + j (1 - 2 b_{n+NC})) * A.  Demodulating the result gives back
 *                                   the same hard bits.  Mode I uses the context's carrier mapper.
 *   d_prs_fft_ref  nb_fft complex float on the device (8-byte aligned), or NULL for the mode's table (mode I: the context's)
 *   freq_norm  != 0: apply_pll(frame, freq_norm) with its phase at 0 on each frame's first sample (both output formats).
 *              Cycles per sample, |freq_norm| < 0.5 (tested from 1e-7 to 0.4999, both signs).  The result is apply_pll's bit for bit over
 *              that whole range, and shares its float phase: sample n is rotated by 2 pi n freq_norm to within
 *              2 pi * 2^-22 * (n |freq_norm| + 1) rad -- 2e-4 rad at the end of a mode I frame at 3 kHz, 0.07 rad at |freq_norm| = 0.4999
 *              (measured there: 0.026 rad).  A caller that needs a large shift with a tighter phase shifts the frames itself.
 *   d_out      [n_frames][samples per frame] in out_format, 16-byte aligned:
 *     DABGPU_IQ_RAW_F32L  complex float
 *     DABGPU_IQ_RAW_U8    QuantisedIQ<uint8_t>::from_iq(I * scale, Q * scale), scale = (1.0f / NC * 4.0f) * 127.5f
 * Asynchronous on `stream`.  A bad context, mode, layout or format, or a NULL payload / output with n_frames > 0, returns
 * DABGPU_ERR_INVALID_ARG before any device call. */
enum { DABGPU_TX_PAYLOAD_REFERENCE = 0, DABGPU_TX_PAYLOAD_FRAME_BITS = 1 };
int dabgpu_ofdm_modulate_frames(dabgpu_ctx *ctx, int transmission_mode, const uint8_t *d_payload, int payload_layout,
                                size_t n_frames, const float *d_prs_fft_ref, float freq_norm,
                                void *d_out, int out_format, void *stream);
/* the same from and to host memory (h_prs_fft_ref may be NULL), on the context's stream; returns when h_out is written */
int dabgpu_ofdm_modulate_frames_host_sync(dabgpu_ctx *ctx, int transmission_mode, const uint8_t *h_payload, int payload_layout,
                                          size_t n_frames, const float *h_prs_fft_ref, float freq_norm, void *h_out, int out_format);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Channel encoder (mode I): FIB bodies and sub-channel bytes -> the frame's hard bits (DABGPU_TX_PAYLOAD_FRAME_BITS) -> IQ.
 * ETSI EN 300 401 in the transmit direction; the reference has no channel encoder, the results are pinned to oracle/ and to this
 * library's own decoders (tests/test_gpu_tx_encode.py).
 *
 * dabgpu_tx_encode_plan (host only, no device): the encoding plan of a multiplex.  plans[0 .. n_sub - 1] describe the sub-channels in
 * list order, plans[n_sub] the FIB group (clause 11.2: PI_16 x 21 blocks, PI_15 x 3 blocks, tail PI_X; 96 bytes in, 2304 bits out).
 *   in_offset / in_bytes     the sub-channel's bytes inside one CIF's input record (back to back in list order, as
 *                            dabgpu_decode_frames_layout returns them); *cif_in_bytes = their sum
 *   seg_pi / seg_blocks      clause 11.3: blocks of 128 mother bits punctured with PI (tables 7, 9, 10 as dabgpu_subchannel_plan derives them)
 *   n_words                  32-bit words of input = sum of seg_blocks; the code word's schedule has n_words + 1 entries, the last the tail
 *   kept_bits                bits that survive puncturing (<= length * 64; the capacity units' remaining bits are 0)
 *   sched_offset             first entry of the sub-channel's kept-bit schedule in sched[]; sub-channels with the same segments share one
 *   ring_offset / ring_row_dwords   where the time interleaver's state of the sub-channel sits inside one ring slot (below)
 * sched[k] = {out_bit, keep_mask}: input word w = k - sched_offset yields mother bits 128 w .. 128 w + 127 (4 per input bit, clause
 * 11.1.1, generators 133 171 145 133); of each run of 32, those whose bit is set in keep_mask are kept in order and placed from bit
 * out_bit + (run index) * popcount(keep_mask) of the code word on.  The tail entry covers the 24 mother bits of the six zero bits only.
 * Call with sched = NULL (or too small a sched_capacity) to learn *n_sched; plans must hold n_sub + 1 entries.
 * DABGPU_ERR_INVALID_ARG: a sub-channel outside 0..864 CU, two that overlap, more than 64, a bad protection index, a profile whose code
 * word does not fit its capacity units (table 8's row 34 as listed).  n_sub = 0 is legal: FIC only. */
typedef struct {
    uint32_t start_address, length;       /* capacity units */
    uint32_t in_offset, in_bytes;
    uint32_t seg_pi[4], seg_blocks[4];
    uint32_t n_words, kept_bits;
    uint32_t sched_offset;
    uint32_t ring_offset, ring_row_dwords;
} dabgpu_tx_sub_plan;
typedef struct { uint32_t out_bit, keep_mask; } dabgpu_tx_sched_entry;
int dabgpu_tx_encode_plan(const dabgpu_subchannel *subs, int n_sub, dabgpu_tx_sub_plan *plans, uint32_t *cif_in_bytes,
                          dabgpu_tx_sched_entry *sched, size_t sched_capacity, size_t *n_sched, uint32_t *ring_slot_dwords);

/* Encoder bank: n_ensembles transmitters sharing one multiplex configuration, their time-interleaver state on the device.
 *   FIB CRC16 (5.2.1) -> energy dispersal (10) -> K = 7 rate-1/4 convolutional code with zero tail (11.1) -> puncturing (11.2 FIC,
 *   11.3 MSC) -> 16-CIF time interleaving (12) -> the frame's 230400 bits.
 *   d_fib_data   [n_ensembles][F][4][3][30] FIB bodies; the encoder appends each CRC
 *   d_payload    [n_ensembles][F][4][cif_in_bytes] (4-byte aligned; may be NULL when n_sub = 0)
 *   d_frame_bits [n_ensembles][F] frames of 28800 bytes, frame_stride bytes apart (0 = 28800; a multiple of 16), 16-byte aligned: bit i
 *                of the frame in byte i / 8, bit i % 8, as dabgpu_soft_bits_to_hard_bytes writes them and DABGPU_TX_PAYLOAD_FRAME_BITS reads
 * Bit i of logical frame r of a sub-channel is sent in CIF r + {0,8,4,12,2,10,6,14,1,9,5,13,3,11,7,15}[i % 16]; bits whose logical
 * frame lies before the bank's first frame (or its last reset) are 0, and so are capacity units no sub-channel occupies and a
 * sub-channel's bits beyond its code word.  A call with F frames equals F calls with one.  The frame counter lives on the device:
 * a steady-state call enqueues kernels only and may be captured in a HIP graph; replays continue the sequence.
 * Arguments are checked before any device call.  One bank = one stream at a time. */
typedef struct dabgpu_tx_bank dabgpu_tx_bank;
int dabgpu_tx_bank_create(dabgpu_ctx *ctx, size_t n_ensembles, const dabgpu_subchannel *subs, int n_sub, dabgpu_tx_bank **out);
void dabgpu_tx_bank_destroy(dabgpu_tx_bank *bank);
int dabgpu_tx_bank_reset(dabgpu_tx_bank *bank, void *stream);
int dabgpu_tx_bank_encode_frames(dabgpu_tx_bank *bank, const uint8_t *d_fib_data, const uint8_t *d_payload, size_t n_frames_per_ensemble,
                                 uint8_t *d_frame_bits, size_t frame_stride, void *stream);
/* the encoder followed by dabgpu_ofdm_modulate_frames(mode I, DABGPU_TX_PAYLOAD_FRAME_BITS) on the same stream, through frame bits the
 * bank owns (sized at creation for one frame per ensemble; a call with more grows them, which a capture refuses): d_out
 * [n_ensembles][F][196608] samples in out_format (DABGPU_IQ_RAW_F32L / _U8), identical to the two calls made separately */
int dabgpu_tx_bank_transmit_frames(dabgpu_tx_bank *bank, const uint8_t *d_fib_data, const uint8_t *d_payload, size_t n_frames_per_ensemble,
                                   float freq_norm, void *d_out, int out_format, void *stream);
/* the same from and to host memory, on the context's stream; h_frame_bits [n_ensembles][F][28800] */
int dabgpu_tx_bank_encode_frames_host_sync(dabgpu_tx_bank *bank, const uint8_t *h_fib_data, const uint8_t *h_payload,
                                           size_t n_frames_per_ensemble, uint8_t *h_frame_bits);
int dabgpu_tx_bank_transmit_frames_host_sync(dabgpu_tx_bank *bank, const uint8_t *h_fib_data, const uint8_t *h_payload,
                                             size_t n_frames_per_ensemble, float freq_norm, void *h_out, int out_format);

/* ------------------------------------------------------------------------------------------------------------------------------
 * DAB+ super-frame encoder: AAC access units -> the bytes of a DAB+ sub-channel, five logical frames per super frame.  ETSI TS 102 563
 * clauses 5.2 and 6 in the transmit direction; the consumer is AAC_Frame_Processor (src/dab/audio/aac_frame_processor.cpp:201-320, on the
 * device dabgpu_dabplus_bank_process), which hands the access units back.  Per super frame:
 *   byte 2 = descriptor (rfa | dac_rate | sbr_flag | aac_channel_mode | ps_flag | mpeg_surround_config(3)), then the 12-bit au_start[1 ..
 *   num_aus - 1] packed MSB first (5.2, table 2); the access units at their starts, each followed by its CRC-16-CCITT (start value 0xFFFF,
 *   inverted, MSB first; 5.3.2); the fire code of bytes 2..10 in bytes 0..1; RS(120,110) parity over GF(2^8), p(x) = x^8+x^4+x^3+x^2+1,
 *   roots alpha^0..alpha^9, shortened by 135: code word i = bytes i + j n_rs, j = 0..109, its parity at i + (110 + j) n_rs (6);
 *   the 120 n_rs bytes cut into five logical frames of frame_bytes.
 *
 * dabgpu_dabplus_superframe_layout (host only, no device): where the access units go.  num_aus follows (dac_rate, sbr_flag) of the
 * descriptor as aac_frame_processor.cpp:275-279 reads them (2, 3, 4 or 6), n_rs = frame_bytes / 24, au_start[0] = 3 + ceil(12 (num_aus - 1)
 * / 8), au_start[i + 1] = au_start[i] + au_len[i] + 2; au_len[i] = 0 is legal (the reference's walk accepts it).  Returns 0 and writes
 * au_start[0 .. num_aus] (the rest of au_start[7] zero), or, with au_start untouched,
 *   DABGPU_DABPLUS_TX_BAD_FRAME_SIZE  frame_bytes is not a multiple of 24 in 24..1536 (*num_aus = *n_rs = 0)
 *   DABGPU_DABPLUS_TX_BAD_FILL        au_start[num_aus] != 110 n_rs: the last unit's end is implied by the syntax (:282)
 *   DABGPU_DABPLUS_TX_BAD_START       an au_start[1 .. num_aus - 1] above 4095 does not fit its 12-bit field (possible from n_rs = 38 on)
 * in this order; -1 for a NULL au_len.  au_len holds at least num_aus lengths; au_start, num_aus, n_rs may be NULL. */
enum { DABGPU_DABPLUS_TX_BAD_FRAME_SIZE = 1, DABGPU_DABPLUS_TX_BAD_FILL = 2, DABGPU_DABPLUS_TX_BAD_START = 3 };
int dabgpu_dabplus_superframe_layout(uint32_t frame_bytes, uint8_t descriptor, const uint16_t *au_len, uint16_t *au_start, int *num_aus,
                                     uint32_t *n_rs);
/* n_superframes whole super frames for each of n_streams streams (a stream = an (ensemble, sub-channel) pair); stateless.
 *   d_au_bytes     the payloads (without CRCs) of the access units of super frame k of stream s back to back from d_au_offsets[s][k] on
 *   d_au_len       [n_streams][n_superframes][6] payload bytes; entries from num_aus on are ignored
 *   d_descriptor   [n_streams][n_superframes];  d_frame_bytes [n_streams]
 *   d_frames       logical frame 5 k + j of stream s goes to d_frames + d_stream_offsets[s] + (5 k + j) frame_stride_bytes -- the layout
 *                  dabgpu_dabplus_bank_process reads.  d_frames, the stream offsets and the stride are multiples of 4, frame_stride_bytes >=
 *                  the stream's frame bytes (a stream offset that is not, which the host cannot see, costs byte stores instead of dword
 *                  stores and changes no result).  Only the stream's own frame_bytes bytes per frame are written.  With d_frames a dabgpu_tx_bank
 *                  payload [ens][F][4][cif_in_bytes], d_stream_offsets[s] = e 4 F cif_in_bytes + plan.in_offset, frame_stride_bytes =
 *                  cif_in_bytes, F = 5 and n_superframes = 4 (20 CIFs: the common period of super frames and transmission frames) the
 *                  result is what dabgpu_tx_bank_encode_frames / _transmit_frames read.
 *   d_status       [n_streams][n_superframes]: 0, or the code dabgpu_dabplus_superframe_layout returns for the super frame; a refused
 *                  super frame's five logical frames are written as zeros (which give the receiver a header and no access unit) -- for
 *                  DABGPU_DABPLUS_TX_BAD_FRAME_SIZE the first min(frame_bytes, 1536) bytes of each
 * Asynchronous on `stream`; kernel launches only, so the call may be captured in a HIP graph.  A NULL context, n_superframes < 0, a stride
 * or d_frames that is not a multiple of 4, more than 2^30 super frames, or a NULL pointer with n_streams n_superframes > 0 returns
 * DABGPU_ERR_INVALID_ARG before any device call; n_streams = 0 and n_superframes = 0 are legal and do nothing. */
int dabgpu_dabplus_tx_encode(dabgpu_ctx *ctx, size_t n_streams, int n_superframes, const uint8_t *d_au_bytes, const uint64_t *d_au_offsets,
                             const uint16_t *d_au_len, const uint8_t *d_descriptor, const uint32_t *d_frame_bytes, uint8_t *d_frames,
                             const uint64_t *d_stream_offsets, size_t frame_stride_bytes, int32_t *d_status, void *stream);
/* one stream from and to host memory, on the context's stream: h_au_offsets [n_superframes], h_au_len [n_superframes][6], h_descriptor
 * [n_superframes]; h_frames [5 n_superframes][frame_bytes] back to back; h_status [n_superframes].  Returns when they are written. */
int dabgpu_dabplus_tx_encode_host_sync(dabgpu_ctx *ctx, int n_superframes, const uint8_t *h_au_bytes, const uint64_t *h_au_offsets,
                                       const uint16_t *h_au_len, const uint8_t *h_descriptor, uint32_t frame_bytes, uint8_t *h_frames,
                                       int32_t *h_status);

/* ------------------------------------------------------------------------------------------------------------------------------
 * MSC packet mode with its FEC scheme (EN 300 401 clauses 5.3.2 and 5.3.5), both directions.
 *
 * Receive: MSC_Reed_Solomon_Data_Packet_Processor (src/dab/msc/msc_reed_solomon_data_packet_processor.cpp), the outer code
 * Basic_Data_Packet_Channel runs for a sub-channel with fec_scheme = 1 (src/basic_radio/basic_data_packet_channel.cpp:29-34,74-80),
 * for n_streams streams at once, one wavefront per stream:
 *   walk     ReadPacket over every logical frame (:57-87): 2-byte header = length id (24/48/72/96) | counter | address; address 0x3FE is
 *            a FEC packet whose length field is not believed (:72-75, :150-152); a remainder shorter than 2 bytes or than the packet its
 *            header names is consumed without being stored (:58-61, :78-81)
 *   ring     2472 bytes; a packet that does not fit discards whole packets from the head WITHOUT handing them out (:136-147)
 *   FEC      packets count 0..8; a wrong counter hands out everything stored, FEC packets included, uncorrected (:89-105); counter 8 with a
 *            ring of exactly 2472 bytes corrects the frame, any other fill hands it out uncorrected (:112-120)
 *   correct  (:186-258) 12 rows of RS(204,188) over GF(2^8), p(x) = x^8+x^4+x^3+x^2+1, roots alpha^0..alpha^15, shortened by 51
 *            (src/dab/algorithms/reed_solomon_decoder.cpp as (8, 0x11D, 0, 1, 16, 51)): row y = application bytes i*12 + y, i = 0..187, then
 *            bytes i*12 + y, i = 0..15, of the nine 22-byte FEC data fields.  A row whose locator degree differs from its number of roots
 *            (Decode returns -1) stays as received; otherwise positions 0..187 are written back, parity positions and positions inside the
 *            padding (reported, never applied: reed_solomon_decoder.cpp:464) are not.  Then packets are popped from the corrected 2256 bytes
 *            by their corrected headers until at least 2256 bytes are read -- a header an uncorrectable row left wrong makes this walk
 *            differ from the one at push time and run up to 72 bytes into the FEC packets.  The FEC packets of a corrected frame are not
 *            handed out.
 * is_corrected means "went through the FEC path", not "an error was fixed"; a data packet whose length bits arrive damaged misaligns the
 * walk before any correction can run.  Both are the reference's behaviour.
 * Per packet handed out, the fields of the data-packet header and its CRC (src/dab/msc/msc_data_packet_processor.cpp:60-66, :23-32,
 * :81-92: x^16+x^12+x^5+1, start 0xFFFF, inverted, over the first length - 2 bytes) are recorded; for FEC packets handed out uncorrected
 * they are the same bit fields of those bytes.
 */
typedef struct {
    uint32_t offset;                /* of the packet inside the stream's slot of d_packets */
    uint16_t length;                /* 24 / 48 / 72 / 96 */
    uint16_t address;
    uint8_t continuity_index;
    uint8_t first_last;             /* bit 1 first, bit 0 last (table 7) */
    uint8_t command;
    uint8_t useful_length;
    uint8_t is_corrected;           /* the callback's flag */
    uint8_t crc_ok;
    uint8_t reserved[2];
} dabgpu_packet_record;
typedef struct {
    int32_t frame_index;            /* index inside this call of the logical frame in which the ninth FEC packet arrived */
    int32_t first_record;           /* index of the record of the frame's first packet */
    int8_t rs_count[12];            /* Decode's return value per row: roots found, or -1 */
} dabgpu_packet_fec_frame;

typedef struct dabgpu_packet_bank dabgpu_packet_bank;
int dabgpu_packet_bank_create(dabgpu_ctx *ctx, size_t n_streams, dabgpu_packet_bank **out);
void dabgpu_packet_bank_destroy(dabgpu_packet_bank *bank);
int dabgpu_packet_bank_reset(dabgpu_packet_bank *bank, void *stream);
/* n_frames logical frames per stream, read where dabgpu_dabplus_bank_process reads them (frame f of stream s = d_frame_bytes[s] bytes at
 * d_frames + d_stream_offsets[s] + f frame_stride_bytes); any frame size is accepted.  Ring, heads, fill, discard counters and the last FEC
 * counter of every stream stay in device memory between calls.
 *   d_packets    [n_streams][packet_stride_bytes]: the packets the callback receives, in its order, back to back
 *   d_records    [n_streams][max_records]: one per packet; d_fec_frames [n_streams][max_fec_frames]: one per corrected FEC frame.  Packets
 *                and frames beyond max_records / max_fec_frames are counted, their records are not written
 *   d_counts     [n_streams][4]: packets handed out, bytes handed out, FEC frames corrected, packets discarded without callback
 * A call hands out at most 2472 + n_frames * frame bytes; a stream whose slot is smaller is not processed and gets d_counts[s][1] = -2.
 * Asynchronous on `stream`, one kernel launch, capturable in a HIP graph.  A NULL argument, n_frames < 0, negative max_records /
 * max_fec_frames or streams_per_flag < 1 return DABGPU_ERR_INVALID_ARG before any device call; n_frames = 0 does nothing. */
int dabgpu_packet_bank_process(dabgpu_packet_bank *bank, const uint8_t *d_frames, const uint64_t *d_stream_offsets, size_t frame_stride_bytes,
                               const uint32_t *d_frame_bytes, int n_frames, uint8_t *d_packets, size_t packet_stride_bytes,
                               dabgpu_packet_record *d_records, int max_records, dabgpu_packet_fec_frame *d_fec_frames, int max_fec_frames,
                               int32_t *d_counts, void *stream);
/* the same, skipping every stream whose flag d_active[s / streams_per_flag] is negative (its counts are written as zeros) */
int dabgpu_packet_bank_process_masked(dabgpu_packet_bank *bank, const uint8_t *d_frames, const uint64_t *d_stream_offsets,
                                      size_t frame_stride_bytes, const uint32_t *d_frame_bytes, int n_frames, uint8_t *d_packets,
                                      size_t packet_stride_bytes, dabgpu_packet_record *d_records, int max_records,
                                      dabgpu_packet_fec_frame *d_fec_frames, int max_fec_frames, int32_t *d_counts, const int32_t *d_active,
                                      int streams_per_flag, void *stream);
/* one buffer through a one-stream bank, from and to host memory (the mirror class's ReadPacket loop over one logical frame): h_packets
 * [2472 + n_bytes], h_records [max_records], h_fec_frames [max_fec_frames], h_counts [4] */
int dabgpu_packet_fec_read_host_sync(dabgpu_packet_bank *bank, const uint8_t *h_buf, uint32_t n_bytes, uint8_t *h_packets,
                                     dabgpu_packet_record *h_records, int max_records, dabgpu_packet_fec_frame *h_fec_frames,
                                     int max_fec_frames, int32_t *h_counts);

/* Transmit: data groups -> packets -> FEC frames (2256 application bytes, then nine FEC packets with counter 0..8, address 0x3FE and 6
 * zero padding bytes in the last) -> the bytes of a sub-channel.  The reference has no encoder; the definition is the inverse of the walk
 * above and is pinned by the reference's decoder returning 0 for every row and handing every packet back.
 *
 * dabgpu_packet_tx_layout (host only, no device): cuts whole data groups into packets of packet_length bytes (3 header bytes, up to
 * packet_length - 5 useful bytes, zero padding, CRC) for n_fec_frames FEC frames that begin at stream byte start_byte.  24-byte padding
 * packets (address 0, useful length 0) are inserted so that no packet crosses a logical-frame boundary (5.3.2) and every application data
 * table is exactly 2256 bytes.  A group that cannot end inside the call's frames is not begun; the rest is padding.  A group of 0 bytes is
 * one packet with both flags and useful length 0.
 *   table        [max_entries >= 94 n_fec_frames] one entry per packet, in stream order; frame_first [n_fec_frames + 1]: the first entry of
 *                each FEC frame, and the total
 *   position     of an entry: bytes from the start of the call (FEC frame t begins at 2472 t)
 *   end state    *end_start_byte = start_byte + 2472 n_fec_frames, *end_continuity_index for the next call
 * Returns 0, or in this order DABGPU_PACKET_TX_BAD_ADDRESS (not 1..1021), _BAD_LENGTH (not 24/48/72/96), _BAD_FRAME_BYTES (0 or no
 * multiple of 24), _FRAME_TOO_SMALL (frame_bytes below the packet length), _BAD_GROUP (a group above 8191 bytes), _BAD_START (start_byte
 * no multiple of 24); -1 for a NULL pointer, n_fec_frames outside 0..2^20 or a table that is too small. */
enum { DABGPU_PACKET_TX_BAD_ADDRESS = 1, DABGPU_PACKET_TX_BAD_LENGTH = 2, DABGPU_PACKET_TX_BAD_FRAME_BYTES = 3,
       DABGPU_PACKET_TX_FRAME_TOO_SMALL = 4, DABGPU_PACKET_TX_BAD_GROUP = 5, DABGPU_PACKET_TX_BAD_START = 6, DABGPU_PACKET_TX_BAD_TABLE = 7 };
typedef struct {
    int32_t group;                  /* index of the data group, -1 for a padding packet */
    uint32_t offset;                /* of the packet's useful bytes inside the group */
    uint32_t position;              /* of the packet, bytes from the start of the call */
    uint8_t length;                 /* 24 / 48 / 72 / 96 */
    uint8_t useful;                 /* useful data length, 0 .. length - 5 */
    uint8_t flags;                  /* bit 1 first, bit 0 last */
    uint8_t continuity_index;
} dabgpu_packet_tx_entry;
int dabgpu_packet_tx_layout(const uint32_t *group_len, size_t n_groups, uint32_t address, uint32_t packet_length, uint32_t frame_bytes,
                            uint64_t start_byte, uint32_t continuity_index, int n_fec_frames, dabgpu_packet_tx_entry *table,
                            size_t max_entries, uint32_t *frame_first, size_t *groups_consumed, uint64_t *end_start_byte,
                            uint32_t *end_continuity_index);
/* n_fec_frames FEC frames for each of n_streams streams, one wavefront per (stream, FEC frame); stateless.
 *   d_data           the streams' data groups back to back; group g of stream s is bytes d_group_offsets[G] .. d_group_offsets[G + 1] of it,
 *                    G = d_group_base[s] + g.  d_group_offsets [all groups + 1] uint64, d_group_base [n_streams + 1] uint32: stream s owns
 *                    groups d_group_base[s] .. d_group_base[s + 1]
 *   d_table          [n_streams][table_stride] entries, d_frame_first [n_streams][n_fec_frames + 1] as the layout writes them
 *   d_address, d_frame_bytes [n_streams]; d_start_byte [n_streams] uint64
 *   d_frames         byte k of the call (k = 2472 t + ...) goes to d_frames + d_stream_offsets[s] + F frame_stride_bytes + C with
 *                    F = (start_byte + k) / frame_bytes - start_byte / frame_bytes and C = (start_byte + k) % frame_bytes: the layout
 *                    dabgpu_packet_bank_process reads and a dabgpu_tx_bank payload holds.  A trailing partial logical frame is completed by
 *                    the next call, which the caller points at that frame.
 *   d_status         [n_streams][n_fec_frames]: 0, or DABGPU_PACKET_TX_BAD_ADDRESS / _BAD_FRAME_BYTES / _BAD_START / _BAD_TABLE (the frame's
 *                    entries do not tile its 2256 bytes with valid packets inside logical frames and inside their groups); a refused frame
 *                    is written as 94 padding packets and their FEC packets (nothing at all for frame_bytes = 0)
 * Asynchronous on `stream`, one kernel launch, capturable.  A NULL context, n_fec_frames < 0, more than 2^30 frames, table_stride below 94
 * n_fec_frames, or a NULL pointer with n_streams n_fec_frames > 0 return DABGPU_ERR_INVALID_ARG before any device call; n_streams = 0 and
 * n_fec_frames = 0 are legal and do nothing. */
int dabgpu_packet_tx_encode(dabgpu_ctx *ctx, size_t n_streams, int n_fec_frames, const uint8_t *d_data, const uint64_t *d_group_offsets,
                            const uint32_t *d_group_base, const dabgpu_packet_tx_entry *d_table, size_t table_stride,
                            const uint32_t *d_frame_first, const uint16_t *d_address, const uint32_t *d_frame_bytes,
                            const uint64_t *d_start_byte, uint8_t *d_frames, const uint64_t *d_stream_offsets, size_t frame_stride_bytes,
                            int32_t *d_status, void *stream);
/* one stream from and to host memory: the groups back to back in h_data (h_group_offsets [n_groups]); h_frames [n_logical_frames]
 * [frame_bytes] with n_logical_frames = (start_byte % frame_bytes + 2472 n_fec_frames + frame_bytes - 1) / frame_bytes; bytes the call
 * does not write are left as they are.  h_status [n_fec_frames]. */
int dabgpu_packet_tx_encode_host_sync(dabgpu_ctx *ctx, int n_fec_frames, const uint8_t *h_data, size_t n_data_bytes,
                                      const uint64_t *h_group_offsets, size_t n_groups, const dabgpu_packet_tx_entry *h_table,
                                      const uint32_t *h_frame_first, uint32_t address, uint32_t frame_bytes, uint64_t start_byte,
                                      uint8_t *h_frames, int32_t *h_status);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Channel model: multipath inside the guard interval, carrier offset, timing offset and white Gaussian noise for n_streams
 * independent streams of complex float samples.  The reference has no channel (only examples/apply_frequency_shift.cpp); the definition
 * is this library's own, written once in dab-radio_amd/csrc/channel_core.h for the kernel (channel.hip) and for the host model the
 * tests build from the same header, and pinned to an independent numpy model (tests/channel_model.py, tests/test_channel_model.py:
 * Philox known answers, float output inside the derived bound of DESIGN.md 4.16, noise moments, u8 rounding) and on the device bit for
 * bit to the host model (tests/test_gpu_channel.py).  Transmission-mode agnostic.
 *
 * For stream s, absolute output sample m (the bank's 64-bit position + the sample's index in the call) and input x[0 .. n_in):
 *   z      = sum over the n_taps taps, in list order, of (tap_re[k] + j tap_im[k]) * x[m - start - tap_delay[k]]
 *            wrap != 0: the index is taken modulo n_in (a transmission that repeats); wrap = 0: samples outside the input are 0
 *   phase  = phase0_q64 + m * freq_q64 in unsigned 64-bit arithmetic, cycles as a fraction of 2^64; its top 24 bits are the angle.
 *            Exact, periodic by itself and independent of where calls are split -- unlike the float phase of freq_norm above, which
 *            stays as it is.  freq_q64 = phase0_q64 = 0 skips the rotation (an identity channel returns its input bit for bit).
 *   y      = gain * z * e^(j 2 pi phase) + noise_sigma * (g0 + j g1)
 *   g0, g1 = one Box-Muller pair of Philox4x32-10: key = seed, counter = (low word of m >> 1, high word of m >> 1, s, 0); sample m
 *            takes words 2 (m & 1) and 2 (m & 1) + 1 of the four, uniforms ((w >> 8) + 0.5) * 2^-24 (never 0, |g| <= 5.89).
 *            The noise of a sample depends on (seed, s, m) alone.  noise_sigma = 0 adds nothing and runs no generator.
 * Input sample indices are absolute like m: a call at position p reads x[p - start - delay ...] of the d_in it is given, so a call with
 * a + b samples equals a call with a and then one with b ON THE SAME d_in AND n_in, for any a (the position, on the device, carries the
 * shift).  A caller that holds only the input from absolute sample W on passes that window as d_in and adds W to `start`
 * (dabgpu_channel_bank_set_params); the window has to begin max(tap_delay) samples before the first sample the call needs.
 *
 * dabgpu_channel_plan (host only, no device): checks a parameter list and returns the launch geometry.  Refused with
 * DABGPU_ERR_INVALID_ARG: n_streams outside 1..1048576, NULL params, n_taps outside 1..8, a tap_delay above
 * DABGPU_CHANNEL_MAX_DELAY, gain, noise_sigma or a tap that is not finite, noise_sigma < 0, |start| above 2^62 (with positions up to
 * 2^62, which dabgpu_channel_bank_seek enforces and 70,000 years of DAB samples do not reach, the index m - start - delay stays a plain
 * signed 64-bit number: the kernel reduces a tile's first index modulo n_in once and steps from there).
 *   halo           largest tap_delay of the list rounded up to an even count
 *   block_samples  output samples one workgroup produces (DABGPU_CHANNEL_BLOCK)
 *   lds_bytes      staged input of a workgroup: (block_samples + halo + 2) complex float; 0 when no stream needs staging
 *                  (every stream one tap of delay 0: the kernel then reads the input directly)
 * dabgpu_channel_freq_q64(cycles_per_sample): round(cycles * 2^64) modulo 2^64, for |cycles| <= 0.5 (a double carries 53 bits of it;
 * NaN and values outside give 0).  From Hz: cycles = hz / sample rate (2.048e6 for DAB).  dabgpu_channel_freq_cycles is its inverse
 * into [-0.5, 0.5) (tests/test_channel_plan.py: round trips, both signs, +-0.5). */
#define DABGPU_CHANNEL_MAX_TAPS 8
#define DABGPU_CHANNEL_MAX_DELAY 2047
#define DABGPU_CHANNEL_BLOCK 1024
#define DABGPU_CHANNEL_MAX_POSITION ((int64_t)1 << 62)      /* |start| and the stream position stay below: m - start - delay never wraps */
typedef struct {
    uint64_t freq_q64, phase0_q64;
    int64_t start;
    uint64_t seed;
    float gain, noise_sigma;
    int32_t n_taps;
    int32_t tap_delay[DABGPU_CHANNEL_MAX_TAPS];
    float tap_re[DABGPU_CHANNEL_MAX_TAPS], tap_im[DABGPU_CHANNEL_MAX_TAPS];
    int32_t reserved;
} dabgpu_channel_stream;
typedef struct { uint32_t halo, block_samples, lds_bytes, staged; } dabgpu_channel_geometry;
int dabgpu_channel_plan(const dabgpu_channel_stream *params, size_t n_streams, dabgpu_channel_geometry *out);
uint64_t dabgpu_channel_freq_q64(double cycles_per_sample);
double dabgpu_channel_freq_cycles(uint64_t freq_q64);

/* Channel bank: the parameters of n_streams streams and their common position on the device.
 *   d_in    stream s reads d_in + s * in_stride_samples complex float; in_stride_samples = 0: every stream reads the same input,
 *           otherwise >= n_in and even.  16-byte aligned.  n_in >= 1.
 *   d_out   stream s writes n_out samples from d_out + s * out_stride_bytes on: complex float (DABGPU_IQ_RAW_F32L) or the u8 pairs of
 *           the modulator's quantiser, QuantisedIQ<uint8_t>::from_iq(I * u8_scale, Q * u8_scale) (DABGPU_IQ_RAW_U8).  16-byte aligned,
 *           out_stride_bytes a multiple of 16 that holds n_out samples (0 = n_out samples rounded up to 16 bytes).  Nothing else is written.
 * A call is two launches on `stream`: the channel kernel, then a one-thread kernel that adds n_out to the position.  No host state
 * changes, so a call may be captured in a HIP graph; replays continue the stream, with new noise.  _seek sets the position (0 at
 * creation), _set_params replaces all parameters; both are ordered on `stream` like the calls.  One bank = one stream at a time.
 * The launch geometry (staged or direct kernel, LDS size) is fixed when the bank is created, because a captured call has it baked in:
 * _set_params refuses (DABGPU_ERR_INVALID_ARG) parameters whose halo exceeds the creation's, or that need staging in a bank created with
 * single zero-delay taps only.  Create the bank with the widest profile it will carry; narrower ones are accepted later.
 * Arguments are checked before any device call: the rules are plain C++ (dabgpu_host_logic.cpp), exercised without a device by
 * tests/test_channel_plan.py (null handles, the parameter list) and its fuzzer tests/cpp/channel_plan_fuzz.cpp (every rule of an apply
 * call, both sides), and on the device by tests/test_gpu_channel.py (error strings, output untouched). */
typedef struct dabgpu_channel_bank dabgpu_channel_bank;
int dabgpu_channel_bank_create(dabgpu_ctx *ctx, size_t n_streams, const dabgpu_channel_stream *h_params, dabgpu_channel_bank **out);
void dabgpu_channel_bank_destroy(dabgpu_channel_bank *bank);
int dabgpu_channel_bank_set_params(dabgpu_channel_bank *bank, const dabgpu_channel_stream *h_params, void *stream);
int dabgpu_channel_bank_seek(dabgpu_channel_bank *bank, uint64_t position, void *stream);
int dabgpu_channel_bank_apply(dabgpu_channel_bank *bank, const float *d_in, size_t in_stride_samples, size_t n_in, int wrap, size_t n_out,
                              void *d_out, int out_format, size_t out_stride_bytes, float u8_scale, void *stream);
/* the same from and to host memory on the context's stream: h_in [n_streams] rows in_stride_samples apart (any count >= n_in; 0 = one
 * shared row), h_out [n_streams] rows out_stride_bytes apart (any count that holds n_out samples; 0 = back to back); no alignment rule;
 * only the rows' n_out samples are written.  The bank keeps two grow-only device buffers for this form; a call that needs larger ones
 * than any before it waits for the whole device (hipDeviceSynchronize) before it frees the old: a test and single-stream path, not a
 * batch path.  Returns when h_out is written (tests/test_gpu_channel.py, tests/cpp/channel_model_harness.cpp) */
int dabgpu_channel_bank_apply_host_sync(dabgpu_channel_bank *bank, const float *h_in, size_t in_stride_samples, size_t n_in, int wrap,
                                        size_t n_out, void *h_out, int out_format, size_t out_stride_bytes, float u8_scale);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Channel model, fading taps: Rayleigh and Rice taps with Doppler beside the constant taps above.  A fading stream keeps its
 * dabgpu_channel_stream and adds one dabgpu_channel_fading_stream: per tap k a kind,
 *   DABGPU_TAP_STATIC  the tap is the constant h_k = tap_re[k] + j tap_im[k], exactly as above
 *   DABGPU_TAP_FADING  the tap is h_k * g_k(m) with a complex gain g_k(m) of unit mean power
 * and, for a fading tap, DABGPU_FADING_OSC = 17 exact 64-bit integer oscillators (freq_q64[n], phase_q64[n]) -- n = 0 .. 15 the diffuse
 * part, n = 16 the line of sight -- and two floats amp_diffuse = sqrt(1 / (K + 1)) / 4, amp_los = sqrt(K / (K + 1)) (Rayleigh: K = 0).
 * The gain depends on (table, absolute sample m) alone: a + b samples equal a and then b, at any split.
 *   grid      at the absolute samples 64 j (DABGPU_FADING_GRID = 64): (c_n, s_n) = (cos, sin) of oscillator n's angle at sample 64 j (its
 *             top 24 bits, as for the carrier); S = the sum of the 16 diffuse (c_n, s_n) as a fixed pairwise tree -- level by level
 *             v[i] += v[i ^ 1], v[i ^ 2], v[i ^ 4], v[i ^ 8] -- and G_j = fmaf(amp_los, (c_16, s_16), amp_diffuse * S) per component;
 *             amp_los = 0 evaluates no line of sight and G_j = amp_diffuse * S
 *   between   w = (m & 63) / 64 (exact), j = m >> 6: g(m) = fmaf(w, G_{j+1} - G_j, G_j) per component.  The interpolated form IS the
 *             definition (tests/channel_fading_model.py interpolates as well): at the largest Doppler accepted, 2^-11 cycles per sample
 *             (1000 Hz at 2.048 MHz; L band at 200 km/h stays below 300 Hz), an oscillator turns phi = 0.196 rad per interval and the
 *             chord of a unit phasor is off by at most phi^2 / 8 = 4.8e-3 (4.8e-5 at 100 Hz)
 *   tap       e_k = h_k * g_k(m): (fmaf(-h_im, g_im, h_re * g_re), fmaf(h_im, g_re, h_re * g_im)); z then sums e_k * x[...] over the taps
 *             in list order as above (a static tap enters with h_k itself, no product); gain, rotation, noise and the u8 quantiser are
 *             unchanged.  Written once in dab-radio_amd/csrc/channel_core.h; error bound and measurements: DESIGN.md 4.18.
 *
 * dabgpu_channel_fading_plan (host only, no device): the tables of n_streams streams from their specs.  For stream s, tap k, oscillator
 * n < 16 the four words are Philox4x32-10(key = seed, counter = (n, k, s, 1)) -- the last word keeps them apart from the noise, which
 * counts with 0 --, the arrival angle alpha = 2 pi (n + (w0 + 0.5) 2^-32) / 16 (stratified: the mean over seeds of the time-averaged
 * autocorrelation is J0(2 pi f_D tau)), freq_q64 = dabgpu_channel_freq_q64(doppler_cycles * cos alpha), phase_q64 = (w2 << 32) | w3.
 * The line of sight is n = 16: freq_q64 = dabgpu_channel_freq_q64(doppler_cycles * los_cos[k]), its phase from its own call
 * (counter (16, k, s, 1)).  Static taps and taps past n_taps get kind STATIC and zeroed oscillators.  Refused with
 * DABGPU_ERR_INVALID_ARG: a null pointer, everything dabgpu_channel_plan refuses, doppler_cycles outside [0, 2^-11] (NaN included), a
 * kind that is neither STATIC nor FADING, rice_k negative or not finite, los_cos outside [-1, 1] or not finite (of the taps below
 * n_taps; rice_k and los_cos of static taps are not read).
 * dabgpu_channel_fading_gain_host: g(m) of one tap for m = m0 .. m0 + count - 1 as (re, im) float pairs, computed on the host from the
 * same header ((1, 0) for a static tap); for users who want the channel state, and for the tests.
 * dabgpu_channel_profile: presets AS RECALLED FROM COST 207 AND NOT CHECKED AGAINST THE DOCUMENT, delays rounded to the nearest sample
 * at 2.048 MHz, amplitudes real and normalised to unit total power; two taps that round to one delay stay two taps (they fade
 * independently).  Fills n_taps, tap_delay, tap_re, tap_im of *params (its other fields stay) and kind, rice_k, los_cos of *spec:
 *   "tu6"   0, 0.2, 0.5, 1.6, 2.3, 5.0 us at -3, 0, -2, -6, -8, -10 dB, all Rayleigh
 *   "ra6"   0, 0.1, 0.2, 0.3, 0.4, 0.5 us at 0, -4, -8, -12, -16, -20 dB, the first tap Rice (K = 0.91 / 0.41, los_cos = 0.7), the rest Rayleigh
 *   "sfn2"  0 and 200 samples at 0 and -6 dB, both Rayleigh
 * Any other name: DABGPU_ERR_INVALID_ARG. */
#define DABGPU_FADING_OSC 17
#define DABGPU_FADING_GRID 64
#define DABGPU_FADING_MAX_DOPPLER_CYCLES 0.00048828125       /* 2^-11 */
enum { DABGPU_TAP_STATIC = 0, DABGPU_TAP_FADING = 1 };
typedef struct {
    uint64_t freq_q64[DABGPU_FADING_OSC], phase_q64[DABGPU_FADING_OSC];
    float amp_diffuse, amp_los;
} dabgpu_channel_fading_tap;
typedef struct {
    int32_t kind[DABGPU_CHANNEL_MAX_TAPS];
    dabgpu_channel_fading_tap tap[DABGPU_CHANNEL_MAX_TAPS];
} dabgpu_channel_fading_stream;
typedef struct {
    double doppler_cycles;                       /* maximum Doppler shift f_D over the sample rate */
    uint64_t seed;
    int32_t kind[DABGPU_CHANNEL_MAX_TAPS];
    float rice_k[DABGPU_CHANNEL_MAX_TAPS];       /* linear power ratio line of sight / diffuse, >= 0 */
    float los_cos[DABGPU_CHANNEL_MAX_TAPS];      /* cosine of the line of sight's arrival angle */
} dabgpu_channel_fading_spec;
int dabgpu_channel_fading_plan(const dabgpu_channel_stream *params, const dabgpu_channel_fading_spec *specs, size_t n_streams,
                               dabgpu_channel_fading_stream *out);
int dabgpu_channel_fading_gain_host(const dabgpu_channel_fading_stream *row, int tap, uint64_t m0, size_t count, float *out);
int dabgpu_channel_profile(const char *name, dabgpu_channel_stream *params, dabgpu_channel_fading_spec *spec);

/* A fading bank: dabgpu_channel_bank_create_fading uploads the tables beside the parameters; such a bank always launches the fading
 * kernel (staged; its LDS holds the tile's grid gains, (halo + 1026 + 18 x 8) x 8 bytes), whatever the kinds say -- the geometry is fixed at
 * creation for the reason given above: captured calls.  A table is accepted when every kind below n_taps is STATIC or FADING and the two
 * amplitudes of its fading taps are finite.  dabgpu_channel_bank_set_fading replaces all tables, ordered on `stream` like _set_params,
 * and is refused (DABGPU_ERR_INVALID_ARG) on a bank not created fading.  _apply, _apply_host_sync, _seek and _set_params work on a fading
 * bank unchanged (the kinds are read against the n_taps of the parameters in force); a call stays two launches and capturable.  A fading
 * bank whose kinds are all STATIC returns the plain bank's output bit for bit (tests/test_gpu_channel_fading.py). */
/* dabgpu_channel_plan for a fading bank (host only): the same checks, `staged` = 1 and `lds_bytes` with the grid gains */
int dabgpu_channel_plan_fading(const dabgpu_channel_stream *params, size_t n_streams, dabgpu_channel_geometry *out);
int dabgpu_channel_bank_create_fading(dabgpu_ctx *ctx, size_t n_streams, const dabgpu_channel_stream *h_params,
                                      const dabgpu_channel_fading_stream *h_tables, dabgpu_channel_bank **out);
int dabgpu_channel_bank_set_fading(dabgpu_channel_bank *bank, const dabgpu_channel_fading_stream *h_tables, void *stream);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Interferer: narrowband spurs, a band-limited jammer and impulsive bursts added to n_streams independent streams of complex float
 * samples -- what the noise profile and the banded combiner defend against.  The reference has no interferer; the definition is this
 * library's own, written once in dab-radio_amd/csrc/interferer_core.h for the kernel (interferer.hip) and for the host model the
 * tests build from the same header (tests/cpp/interferer_host_model.cpp), pinned to an independent numpy model (tests/interferer_model.py,
 * tests/test_interferer_model.py) and on the device bit for bit to the host model (tests/test_gpu_interferer.py).  Philox, Box-Muller, the
 * 64-bit oscillator and sine / cosine are the channel model's (channel_core.h), unchanged.  Bounds and measurements: DESIGN.md 4.28.
 *
 * For stream s, absolute sample m (the bank's 64-bit position + the sample's index i in the call), n_sources <= DABGPU_INTERFERER_MAX
 * sources k in list order:
 *   TONE   v = amp * e^(j 2 pi phase), phase = phase0_q64 + m * freq_q64 in unsigned 64-bit arithmetic, its top 24 bits the angle
 *   BAND   band-limited Gaussian noise from shape `shape` of the bank (interp L = 2^l, 16 taps per phase): q = m >> l, r = m & (L - 1),
 *            b = sum over t = 0 .. 15 of taps[r + L t] * g[q - t]
 *          in that order, the first term a plain product, the others fmaf, re and im separately; g[n] = the Box-Muller pair of
 *          Philox4x32-10 with key = seed and counter = (low word of n >> 1, high word of n >> 1, s, 16 + k), words 2 (n & 1) and
 *          2 (n & 1) + 1; n is an unsigned 64-bit number, so q - t wraps below 0.  (Counter word 3 is 0 for the channel's noise and 1 for
 *          the fading tables: one seed serves all three independently.)  Then v = (amp * b) * e^(j 2 pi phase), the rotation to the band's
 *          centre (skipped when freq_q64 = phase0_q64 = 0).
 *          shape = -1: white over the whole sampled band, no filter: b = g[m] * 0.70710678f (the division by sqrt 2 written as a
 *          product with the nearest float, because `/` is not the same operation under every compiler: channel_core.h)
 *   gate   gate_period = 0: always on.  Otherwise on iff ((m - gate_offset) mod gate_period) < gate_on, in exact integer arithmetic with
 *          a non-negative remainder; the edges are abrupt (a burst interferer).  amp is the amplitude while the gate is on.
 *   y[i]   = x[i] + v_0 + v_1 + ... added in list order (plain float additions per component); d_in = NULL: x = 0.  A source of kind OFF
 *          or with amp = 0 runs no generator and adds nothing; a stream with no live source returns its input bit for bit.
 * The value of a sample depends on (parameters, shapes, seed, s, k, m) alone: a call of a + b samples equals a call of a and then one of b
 * on the following input, at any split, and replays of a captured call continue the stream.  E|v|^2 = amp^2 while the gate is on.
 *
 * dabgpu_interferer_design (host only, no device): a flat band of width_cycles (a fraction of the sample rate, two-sided) as a
 * Kaiser-windowed sinc of 16 L taps computed in double and rounded to float.  L is the largest power of two <= 64 for which the passband
 * and the transition stay inside the low rate's Nyquist band.  The cutoff (the -6 dB point of the window method) is the nominal edge
 * width_cycles / 2 and the transition, DABGPU_INTERFERER_TRANSITION / L cycles wide, lies around it; the rule is
 * width_cycles / 2 + transition / (2 L) <= 1 / (2 L), so the images of the interpolation fall into the stopband and the output power is
 * the same at every one of the L phases.  The table is scaled so that the mean over the phases of sum_t taps[r + L t]^2 is 1/2 (g has
 * variance 1 per component, hence E|b|^2 = 1).  The record carries its own figures, from the table's spectrum at the 8193 frequencies
 * 0 .. 1/2 of a 2^14-point transform: width_3db_cycles (two-sided), inband_share (power inside +-width / 2 over the whole),
 * stopband_level (largest |H| from width / 2 + transition / (2 L) on, relative to |H(0)|), phase_ripple (max / min over the phases of
 * sum_t taps[r + L t]^2).  Refused with DABGPU_ERR_INVALID_ARG: NULL out, width_cycles not finite, above 1, or below
 * DABGPU_INTERFERER_MIN_WIDTH (narrower than the transition of L = 64 no flat part is left: that is a tone).
 *
 * dabgpu_interferer_plan (host only): checks a parameter list against n_shapes shapes and returns the launch geometry.  Refused, naming
 * stream, source and field: n_streams outside 1..1048576, n_shapes outside 0..4, NULL params (or shapes with n_shapes > 0), a shape whose
 * interp is no power of two in 1..64 or that has a tap that is not finite, n_sources outside 0..4, a kind that is none of OFF, TONE,
 * BAND, of the sources below n_sources that are not OFF: amp not finite or negative, gate_on > gate_period, |gate_offset| >= 2^62, and of
 * BAND sources a shape index outside -1 .. n_shapes - 1.
 *   block_samples  output samples one workgroup produces (DABGPU_INTERFERER_BLOCK)
 *   band_slots     the largest count of shaped BAND sources (shape >= 0, amp != 0) on one stream
 *   slot_bytes     LDS of one such source: the largest, over the shapes, of 16 L floats + (1024 / L + 18) complex floats
 *   lds_bytes      band_slots x slot_bytes; 0 for a bank of tones and white sources (that kernel variant allocates none) */
#define DABGPU_INTERFERER_MAX 4
#define DABGPU_INTERFERER_MAX_SHAPES 4
#define DABGPU_INTERFERER_TAPS 16
#define DABGPU_INTERFERER_MAX_INTERP 64
#define DABGPU_INTERFERER_BLOCK 1024
#define DABGPU_INTERFERER_TRANSITION 0.25                   /* transition width of a shape, in cycles of its low rate */
#define DABGPU_INTERFERER_MIN_WIDTH 0.00390625              /* 2^-8 = the transition of L = 64; L = 64 serves widths up to 0.75 / 64 */
#define DABGPU_INTERFERER_MAX_POSITION ((int64_t)1 << 62)   /* |gate_offset| and the stream position stay below */
enum { DABGPU_INTERFERER_OFF = 0, DABGPU_INTERFERER_TONE = 1, DABGPU_INTERFERER_BAND = 2 };
typedef struct {
    int32_t kind;                   /* DABGPU_INTERFERER_OFF / _TONE / _BAND */
    int32_t shape;                  /* BAND: index of a shape of the bank, or -1 = white */
    float amp;
    int32_t reserved;
    uint64_t freq_q64, phase0_q64;  /* the tone, or the band's centre (dabgpu_channel_freq_q64) */
    uint64_t gate_period, gate_on;  /* samples; gate_period = 0: always on */
    int64_t gate_offset;
} dabgpu_interferer_source;
typedef struct {
    uint64_t seed;
    int32_t n_sources, reserved;
    dabgpu_interferer_source source[DABGPU_INTERFERER_MAX];
} dabgpu_interferer_stream;
typedef struct {
    int32_t interp, reserved;       /* L */
    double width_cycles, cutoff_cycles, beta;
    double width_3db_cycles, inband_share, stopband_level, phase_ripple;
    float taps[DABGPU_INTERFERER_TAPS * DABGPU_INTERFERER_MAX_INTERP];      /* the first 16 L are used: tap j = r + L t */
} dabgpu_interferer_shape;
typedef struct { uint32_t block_samples, band_slots, slot_bytes, lds_bytes; } dabgpu_interferer_geometry;
int dabgpu_interferer_design(double width_cycles, dabgpu_interferer_shape *out);
int dabgpu_interferer_plan(const dabgpu_interferer_stream *params, size_t n_streams, const dabgpu_interferer_shape *shapes, int n_shapes,
                           dabgpu_interferer_geometry *out);

/* Interferer bank: the parameters of n_streams streams, up to 4 shapes shared by all of them and the common position on the device,
 * built like the channel bank above.
 *   d_in    NULL (the bank generates the interferer alone), or stream s reads n_out complex float from d_in + s * in_stride_samples;
 *           in_stride_samples = 0: every stream reads the same row, otherwise >= n_out and even.  16-byte aligned.
 *   d_out   as dabgpu_channel_bank_apply: complex float or the modulator's u8 pairs with u8_scale, rows out_stride_bytes apart (a multiple
 *           of 16 that holds n_out samples; 0 = the default), 16-byte aligned.  d_out == d_in (complex float, rows equally far apart) is
 *           allowed: the operation is sample-wise in x.
 * A call is the interferer kernel and the one-thread kernel that adds n_out to the position, on `stream`; no host state changes, so a
 * call may be captured and its replays continue the stream.  _seek sets the position (< 2^62), _set_params replaces all parameters within
 * the geometry fixed at creation: more shaped BAND sources on one stream than band_slots of the creation are refused, and so is any in a
 * bank created without (the shapes stay those of the creation).  Arguments are checked in plain C++ (dabgpu_host_logic.cpp) before any
 * device call, and a refusal leaves the output untouched (tests/test_interferer_plan.py, tests/test_gpu_interferer.py). */
typedef struct dabgpu_interferer_bank dabgpu_interferer_bank;
int dabgpu_interferer_bank_create(dabgpu_ctx *ctx, size_t n_streams, const dabgpu_interferer_stream *h_params,
                                  const dabgpu_interferer_shape *h_shapes, int n_shapes, dabgpu_interferer_bank **out);
void dabgpu_interferer_bank_destroy(dabgpu_interferer_bank *bank);
int dabgpu_interferer_bank_set_params(dabgpu_interferer_bank *bank, const dabgpu_interferer_stream *h_params, void *stream);
int dabgpu_interferer_bank_seek(dabgpu_interferer_bank *bank, uint64_t position, void *stream);
int dabgpu_interferer_bank_apply(dabgpu_interferer_bank *bank, const float *d_in, size_t in_stride_samples, size_t n_out, void *d_out,
                                 int out_format, size_t out_stride_bytes, float u8_scale, void *stream);
/* the same from and to host memory on the context's stream (h_in may be NULL; rows of any length >= n_out, no alignment rule), as
 * dabgpu_channel_bank_apply_host_sync */
int dabgpu_interferer_bank_apply_host_sync(dabgpu_interferer_bank *bank, const float *h_in, size_t in_stride_samples, size_t n_out,
                                           void *h_out, int out_format, size_t out_stride_bytes, float u8_scale);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Impulse blanker: zeroes bursts (ignition-like impulsive interference, the interferer's gated white source) in n_streams independent
 * streams of complex float samples ahead of the demodulator.  The reference has no blanker; the definition is this library's own,
 * written once in dab-radio_amd/csrc/blanker_core.h for the kernel (blanker.hip) and for the host model the tests build from the same
 * header (tests/cpp/blanker_host_model.cpp), pinned to an independent numpy model (tests/blanker_model.py, tests/test_blanker_model.py)
 * and on the device bit for bit to the host model (tests/test_gpu_blanker.py).  Derivation and measurements: DESIGN.md 4.29.
 *
 * A greatest-of cell-averaging detector on block powers.  It takes no level from outside and keeps no state: output sample m of stream s
 * depends on (parameters, the input around m) alone, so a call of a + b samples equals a call of a and then one of b on the same d_in and
 * n_in at any split (inside a block too), and replays of a captured call continue the stream.
 *   input   x[i], i = m - start, of the caller's d_in; m is absolute (the bank's 64-bit position + the sample's index in the call) and
 *           signed where blocks before sample 0 are read; samples outside [0, n_in) are 0.  A caller that holds a window from absolute
 *           sample W on passes it as d_in and adds W to `start`.
 *   p[b]    block b = absolute samples [32 b, 32 b + 32): the mean of |x|^2 in float32.  |x|^2 = fmaf(im, im, re * re); the 32 values
 *           are summed as a pairwise tree (neighbours first, 5 levels); the mean is a product with 2^-5.  No division anywhere.
 *   ref[b]  q[b] = p[b] where finite, else 0.  before = sum_{k = 1..window} q[b - gap - k], after = sum_{k = 1..window} q[b + gap + k],
 *           each from 0 in increasing k in float32; ref = the greater of the two (the smaller cannot be trusted at a NULL -> PRS edge,
 *           where "before" holds noise only and would blank the start of every frame).
 *   flag[b] = p[b] not finite, or (ref[b] > 0 and (float)window * p[b] > threshold * ref[b])
 *   blank[b] = the OR of flag[b - guard .. b + guard]
 *   y[m]    = +0 + j(+0) where blank[m >> 5], else x[m - start] bit for bit.  A stream with enabled = 0 copies its input.
 *   mask    (optional) one uint32 per stream and absolute tile of 1024 samples: bit k of tile t's word is blank[32 t + k].  Word j of a
 *           call at position p is tile (p >> 10) + j; a call sets only the bits of blocks whose FIRST sample lies in [p, p + n_out) and
 *           writes all dabgpu_blanker_mask_words(n_out) = n_out / 1024 + 2 words of every stream (the others 0), so the words of split
 *           calls OR together to the words of one call.  A disabled stream's words are 0.
 * dabgpu_blanker_defaults: threshold 3, gap 8, window 16, guard 1, enabled, start 0.  Against one 16-block side a threshold of 3 has a
 * per-block false-alarm probability of 3.9e-13 for complex Gaussian samples (tests/blanker_model.py recomputes it).
 *
 * dabgpu_blanker_plan (host only, no device): refused with DABGPU_ERR_INVALID_ARG, naming stream and field: n_streams outside
 * 1..1048576, NULL params, a threshold that is not finite or outside (1, 1024], window outside 1..32, gap outside 0..32, guard outside
 * 0..4, |start| above 2^62.  (enabled = 0 streams are checked all the same.)
 *   reach_blocks   the largest gap + window + guard of the list: blocks either side of a block that its output depends on
 *   block_samples  output samples one workgroup produces (DABGPU_BLANKER_BLOCK)
 *   lds_bytes      a workgroup's block powers and flags: (block_samples / 32 + 2 reach_blocks) floats + (block_samples / 32 + 8) words
 * dabgpu_blanker_input_needed (host only): the input indices [first, first + count) (first may be negative, count may run past n_in)
 * that a call of n_out samples at `position` reads of a stream with these parameters: whole blocks, gap + window + guard blocks either
 * side; count = 0 for n_out = 0; a disabled stream reads its n_out samples only.  With the defaults the look-ahead is 25 blocks = 800
 * samples, about 0.39 ms at 2.048 MS/s. */
#define DABGPU_BLANKER_POWER_BLOCK 32                       /* samples of one block power */
#define DABGPU_BLANKER_BLOCK 1024                           /* samples of one workgroup's tile = one mask word */
#define DABGPU_BLANKER_MAX_WINDOW 32
#define DABGPU_BLANKER_MAX_GAP 32
#define DABGPU_BLANKER_MAX_GUARD 4
#define DABGPU_BLANKER_MAX_THRESHOLD 1024.0f
#define DABGPU_BLANKER_MAX_POSITION ((int64_t)1 << 62)      /* |start| and the stream position stay below */
typedef struct {
    int64_t start;
    float threshold;
    int32_t gap, window, guard;     /* blocks */
    int32_t enabled, reserved;
} dabgpu_blanker_stream;
typedef struct { uint32_t reach_blocks, block_samples, lds_bytes, reserved; } dabgpu_blanker_geometry;
dabgpu_blanker_stream dabgpu_blanker_defaults(void);
size_t dabgpu_blanker_mask_words(size_t n_out);
int dabgpu_blanker_plan(const dabgpu_blanker_stream *params, size_t n_streams, dabgpu_blanker_geometry *out);
int dabgpu_blanker_input_needed(const dabgpu_blanker_stream *params, uint64_t position, size_t n_out, int64_t *first, uint64_t *count);

/* Impulse blanker bank: the parameters of n_streams streams and their common position on the device, built like the channel bank.
 *   d_in    stream s reads d_in + s * in_stride_samples complex float; in_stride_samples = 0: one shared row, otherwise >= n_in and even.
 *           16-byte aligned.  n_in >= 1.
 *   d_out   stream s writes n_out complex float from d_out + s * out_stride_bytes on (a multiple of 16 that holds n_out samples; 0 = the
 *           default), 16-byte aligned.  d_out == d_in is refused: a workgroup reads its neighbours' tiles, so in place is not defined.
 *   d_mask  NULL, or stream s writes dabgpu_blanker_mask_words(n_out) words from d_mask + s * mask_stride_words on (0 = that count;
 *           otherwise at least that count), 4-byte aligned.
 * A call is two launches on `stream`: the blanker kernel and the one-thread kernel that adds n_out to the position; no host state
 * changes, so a call may be captured and its replays continue the stream.  _seek sets the position (<= 2^62), _set_params replaces all
 * parameters within the geometry fixed at creation: a larger reach_blocks is refused (create the bank with its widest parameters).
 * Arguments are checked in plain C++ (dabgpu_host_logic.cpp) before any device call, and a refusal leaves the output untouched
 * (tests/test_blanker_plan.py, tests/test_gpu_blanker.py). */
typedef struct dabgpu_blanker_bank dabgpu_blanker_bank;
int dabgpu_blanker_bank_create(dabgpu_ctx *ctx, size_t n_streams, const dabgpu_blanker_stream *h_params, dabgpu_blanker_bank **out);
void dabgpu_blanker_bank_destroy(dabgpu_blanker_bank *bank);
int dabgpu_blanker_bank_set_params(dabgpu_blanker_bank *bank, const dabgpu_blanker_stream *h_params, void *stream);
int dabgpu_blanker_bank_seek(dabgpu_blanker_bank *bank, uint64_t position, void *stream);
int dabgpu_blanker_bank_apply(dabgpu_blanker_bank *bank, const float *d_in, size_t in_stride_samples, size_t n_in, size_t n_out, void *d_out,
                              size_t out_stride_bytes, uint32_t *d_mask, size_t mask_stride_words, void *stream);
/* the same from and to host memory on the context's stream (rows of any length >= n_in, no alignment rule; h_mask may be NULL), as
 * dabgpu_channel_bank_apply_host_sync */
int dabgpu_blanker_bank_apply_host_sync(dabgpu_blanker_bank *bank, const float *h_in, size_t in_stride_samples, size_t n_in, size_t n_out,
                                        void *h_out, size_t out_stride_bytes, uint32_t *h_mask, size_t mask_stride_words);

/* ------------------------------------------------------------------------------------------------------------------------------
 * IQ balance: the DC term and the mirror image of a zero-IF front end, in n_streams independent streams of complex float samples --
 * made (the impairment behind the simulator's channel) and removed (blindly, ahead of resampler, channeliser and blanker) by one
 * widely-linear map per sample.  The reference has nothing comparable; the definition is this library's own, written once in
 * dab-radio_amd/csrc/iqbal_core.h for the kernels (iqbal.hip), for dabgpu_iqbal_solve_host and for the host model the tests build from
 * the same header (tests/cpp/iqbal_host_model.cpp), pinned to an independent numpy model (tests/iqbal_model.py,
 * tests/test_iqbal_model.py) and on the device bit for bit to the host model (tests/test_gpu_iqbal.py).  Derivation, bounds and
 * measurements: DESIGN.md 4.32.
 *
 *   map     z = a y + b conj(y) + c, complex float a, b, c per stream; each component starts from c and takes the terms of a, then those
 *           of b, one fmaf each (iqbal_core.h, iqb_map).  A stream of mode OFF copies its input bit for bit.
 *   tile    1024 ABSOLUTE samples (the bank's 64-bit position + the sample's index in the call).  Its five float32 moments, of the RAW
 *           input: sum re, sum im, sum |y|^2 = fmaf(im, im, re re), sum fmaf(-im, im, re re), sum (2 re) im, each a 10-level pairwise
 *           tree over the sample index; the level order (index bits 0, 9, 1 .. 8) is iqbal_core.h's IQB_TREE_BITS.
 *   fold    state N, S[5] per TRACK stream; for each tile of a MEASURE call in increasing order N = fmaf(forget, N, 1024),
 *           S_k = fmaf(forget, S_k, m_k).  A tile with a moment that is not finite is skipped and counted (tiles_skipped).
 *   solve   r = 1 / N, d = (S_0, S_1) r, P = S_2 r - |d|^2, Q = (S_3, S_4) r - d^2, C = Q (1 / P), w_0 = C / 2 and three steps
 *           w = (C / 2)(1 + |w|^2) (the fixed point of C = 2 w / (1 + |w|^2), w = K2 / conj(K1)); a = 1, b = -w, c = -(d - w conj(d)).
 *           Identity (a = 1, b = c = 0, valid = 0) while N < min_weight, or P is not a normal positive float, or |C|^2 >= 1.  The
 *           residual complex gain K1 (1 - |w|^2) stays in the samples: DQPSK does not see it.
 * dabgpu_iqbal_defaults: TRACK, a = 1, b = c = 0, forget = dabgpu_iqbal_forget(16 mode-I frames), min_weight 65536.
 * dabgpu_iqbal_plan (host only): refused with DABGPU_ERR_INVALID_ARG, naming stream and field: n_streams outside 1..1048576, NULL
 * params, a mode outside OFF / FIXED / TRACK, a coefficient that is not finite, forget outside (0, 1], min_weight not finite or below
 * 1024 (one tile), max_samples_per_call not a multiple of 1024 in 1024..2^31.
 *   tile_samples    1024
 *   tiles_per_call  max_samples_per_call / 1024: the tiles a MEASURE call may hold
 *   scratch_bytes   n_streams x tiles_per_call x 32: the bank's tile records
 * dabgpu_iqbal_impairment: a FIXED stream for a front end with gain error gain_db (Q against I) and phase error phase_deg and DC
 * dc_re + j dc_im: a = K1 = (1 + g e^{-j phi}) / 2, b = K2 = (1 - g e^{j phi}) / 2, c = DC, formed in double and rounded once.  Refused:
 * |gain_db| > 20, |phase_deg| > 45, anything not finite.
 * dabgpu_iqbal_forget: forget per tile for a time constant in samples, exp(-1024 / tau) rounded to float (1 for an infinite one); 0
 * for a time constant that is not at least one tile.
 * dabgpu_iqbal_solve_host: the solve above of the state in record->N, record->S with the stream's min_weight; fills the other fields of
 * the record except the counters. */
#define DABGPU_IQBAL_TILE 1024
#define DABGPU_IQBAL_OFF 0
#define DABGPU_IQBAL_FIXED 1
#define DABGPU_IQBAL_TRACK 2
#define DABGPU_IQBAL_MEASURE 1u                             /* flags of _apply */
#define DABGPU_IQBAL_APPLY 2u
#define DABGPU_IQBAL_MAX_POSITION ((uint64_t)1 << 62)
typedef struct {
    int32_t mode, reserved;
    float a_re, a_im, b_re, b_im, c_re, c_im;   /* FIXED: the map's coefficients */
    float forget, min_weight;                   /* TRACK */
} dabgpu_iqbal_stream;
typedef struct { uint32_t tile_samples, tiles_per_call; uint64_t scratch_bytes; } dabgpu_iqbal_geometry;
typedef struct {
    float N, S[5];                              /* the fold's state */
    float d_re, d_im, P, C_re, C_im, w_re, w_im;
    float a_re, a_im, b_re, b_im, c_re, c_im;   /* what the next APPLY maps a TRACK stream with */
    uint32_t valid;                             /* 1: the coefficients are the solve's; 0: identity */
    uint64_t tiles_used, tiles_skipped;
    uint32_t calls_refused, reserved;           /* MEASURE calls that found the position off a tile edge (the device refuses them) */
} dabgpu_iqbal_record;
dabgpu_iqbal_stream dabgpu_iqbal_defaults(void);
int dabgpu_iqbal_plan(const dabgpu_iqbal_stream *params, size_t n_streams, size_t max_samples_per_call, dabgpu_iqbal_geometry *out);
int dabgpu_iqbal_impairment(double gain_db, double phase_deg, double dc_re, double dc_im, dabgpu_iqbal_stream *out);
float dabgpu_iqbal_forget(double time_constant_samples);
int dabgpu_iqbal_solve_host(const dabgpu_iqbal_stream *params, dabgpu_iqbal_record *record);

/* IQ balance bank: the parameters and records of n_streams streams, their common position and the tile scratch on the device.
 *   flags   DABGPU_IQBAL_MEASURE, DABGPU_IQBAL_APPLY or both.  Both is ONE pass: the output is mapped with the coefficients as they stood
 *           before the call, then the call's tiles are folded and solved.  Priming: a MEASURE call, _seek back, an APPLY call.
 *   d_in    stream s reads n complex float from d_in + s * in_stride_samples (0: one shared row; otherwise >= n and even), 16-byte aligned.
 *   d_out   APPLY: stream s writes n samples from d_out + s * out_stride_bytes on (a multiple of 16 that holds n samples; 0 = the
 *           default), 16-byte aligned, complex float or u8 pairs (ch_u8 with u8_scale).  d_out == d_in is allowed for complex float with
 *           equal strides: the map is pointwise.  NULL without APPLY.
 *   MEASURE needs n to be a multiple of 1024 up to the bank's max_samples_per_call (refused on the host) and the position to be a
 *           multiple of 1024.  The position lives on the device, so that refusal is the device's: the call writes nothing, folds
 *           nothing, leaves the position where it was and raises calls_refused of every record; the host form returns
 *           DABGPU_ERR_INVALID_ARG then.  Frames of all four transmission modes are multiples of 1024.
 *   APPLY alone takes any position and any n; partial tiles at either end are stored sample by sample.
 * A call is up to three launches on `stream`: the work kernel (one 256-thread workgroup per stream and tile), with MEASURE the
 * fold-and-solve kernel (one lane per stream, tiles in increasing order, no atomics), and the position advance.  No host state changes,
 * so a call may be captured and its replays continue the stream.  _seek sets the position (<= 2^62), _set_params replaces all
 * parameters and keeps the records, _reset returns the records to their first state (N = 0, identity, counters 0). */
typedef struct dabgpu_iqbal_bank dabgpu_iqbal_bank;
int dabgpu_iqbal_bank_create(dabgpu_ctx *ctx, size_t n_streams, const dabgpu_iqbal_stream *h_params, size_t max_samples_per_call,
                             dabgpu_iqbal_bank **out);
void dabgpu_iqbal_bank_destroy(dabgpu_iqbal_bank *bank);
int dabgpu_iqbal_bank_set_params(dabgpu_iqbal_bank *bank, const dabgpu_iqbal_stream *h_params, void *stream);
int dabgpu_iqbal_bank_seek(dabgpu_iqbal_bank *bank, uint64_t position, void *stream);
int dabgpu_iqbal_bank_reset(dabgpu_iqbal_bank *bank, void *stream);
int dabgpu_iqbal_bank_apply(dabgpu_iqbal_bank *bank, const float *d_in, size_t in_stride_samples, size_t n, void *d_out, int out_format,
                            size_t out_stride_bytes, float u8_scale, uint32_t flags, void *stream);
/* the same from and to host memory on the context's stream (rows of any length >= n, no alignment rule; h_out may be NULL without
 * APPLY), as dabgpu_channel_bank_apply_host_sync */
int dabgpu_iqbal_bank_apply_host_sync(dabgpu_iqbal_bank *bank, const float *h_in, size_t in_stride_samples, size_t n, void *h_out,
                                      int out_format, size_t out_stride_bytes, float u8_scale, uint32_t flags);
/* the n_streams records (waits for the context's stream) */
int dabgpu_iqbal_bank_read_state_host_sync(dabgpu_iqbal_bank *bank, dabgpu_iqbal_record *h_records);
/* the tile records of the last MEASURE call, n_tiles <= tiles_per_call of them per stream: h_moments[(s * n_tiles + j) * 8 + k], k < 5 the
 * sums of the call's tile j, k >= 5 zero (waits for the context's stream) */
int dabgpu_iqbal_bank_read_moments_host_sync(dabgpu_iqbal_bank *bank, size_t n_tiles, float *h_moments);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Resampler: arbitrary-ratio, fractional-delay resampling of n_streams independent streams of complex float samples -- a receiver's
 * sampling-clock error and fractional delay behind the channel model, and captures at 2.4, 2.56, 3.072 or 4.096 MS/s brought to the 2.048 MHz
 * grid in front of the demodulator.  The reference has nothing comparable; the definition is this library's own, written once in
 * dab-radio_amd/csrc/resample_core.h for the kernel (resample.hip) and for the host model the tests build from the same header, pinned to
 * an independent numpy model (tests/resample_model.py, tests/test_resample_model.py) and on the device bit for bit to the host model
 * (tests/test_gpu_resample.py).  Error bounds and measurements: DESIGN.md 4.19.
 *
 * For stream s, absolute output sample m (the bank's 64-bit position + the sample's index in the call) and input x[0 .. n_in):
 *   T(m)   = offset_q62 + m * step_q62 in exact integer arithmetic, in units of 2^-62 input samples; step_q62 is unsigned Q2.62 (input
 *            samples per output sample, 0.5 .. 2), offset_q62 = offset_samples * 2^62 + offset_frac_q62 is signed: offset_samples any
 *            integer up to +-2^62, offset_frac_q62 in [0, 2^62).  The value is 128 bits wide and depends on (parameters, m) alone: a call
 *            with a + b samples equals a call with a and then one with b on the same d_in and n_in, at any split.
 *   n, p, w  n = floor(T / 2^62); the phase row p = the top 8 bits of the fraction (DABGPU_RESAMPLE_PHASES = 256 rows); w = the next 15
 *            bits over 2^15
 *   c_j    = fmaf(w, H[p + 1][j] - H[p][j], H[p][j]), j = 0 .. DABGPU_RESAMPLE_TAPS - 1: H is the design's table of L + 1 rows, row L
 *            being row 0 advanced by one input sample.  The interpolated form IS the definition.
 *   y      = gain * sum_j c_j * x[n - taps / 2 + 1 + j], re and im separate, each one chain in ascending j that starts from the product
 *            c_0 * x and continues with fmaf(c_j, x, sum).  wrap != 0: the index is taken modulo n_in (a transmission that repeats);
 *            wrap = 0: samples outside the input are 0.  The output is complex float or the u8 pairs of the modulator's quantiser.
 *   identity  step_q62 = 2^62 with offset_frac_q62 = 0 takes no filter: y = gain * x[n], the shifted input bit for bit at gain 1.
 *
 * dabgpu_resample_design (host only): the (L + 1) x taps float table of a Kaiser-windowed sinc (beta = 9.25, I0 by its series, everything
 * in double) for steps up to max_step (0.5 .. 2).  With M = max(max_step, 1): h(t) = sinc(t / M) / M * kaiser(t), zero for |t| >= taps / 2,
 * H[p][j] = h(p / L + taps / 2 - 1 - j), every row p < L divided by its sum (DC gain 1 per phase), H[L][j] = H[0][j - 1], H[L][0] = 0.
 * passband_cycles (0 = the default 0.375, the +-768 kHz of a DAB block at 2.048 MHz; accepted: (0, 0.45]) is the passband edge in cycles
 * per sample of the SLOWER of the two rates: per output sample for max_step >= 1, per input sample below (where 0.375 cycles per output
 * sample would lie above the input's own Nyquist frequency).  In cycles per input sample the passband ends at passband / M, the first alias
 * of it begins at (1 - passband) / M and the cutoff 0.5 / M lies half way.  The function RETURNS the table's own error, evaluated in double
 * over frequencies x all phases x w in {0, 1/2, 1 - 2^-15}:
 *   passband_error   worst |sum_j c_j e^(2 pi i f (j - taps / 2 + 1 - frac)) - 1| over 65 frequencies f in [0, passband / M]
 *   alias_leakage    worst |the same sum| over 65 frequencies in [(1 - passband) / M, 0.5] (0 where that interval is empty: M <= 1.25)
 *   error            their sum; 1e-4 (-80 dB) or better for every max_step in [0.5, 2] at the default passband
 * A bank has one table; a stream may use it when its step does not exceed the design's max_step (a smaller step keeps the passband in
 * input cycles, which is narrower in its own output cycles).
 *
 * dabgpu_resample_plan (host only): checks a parameter list against a design and returns the launch geometry.  Refused with
 * DABGPU_ERR_INVALID_ARG: a null pointer, n_streams outside 1..1048576, a step outside [0.5, 2] or above the design's max_step (rounded up
 * to Q2.62), gain not finite, |offset_samples| above DABGPU_CHANNEL_MAX_POSITION, offset_frac_q62 >= 2^62.
 *   block_samples   output samples one workgroup produces (DABGPU_RESAMPLE_BLOCK)
 *   window_samples  input window of a workgroup: ceil(block_samples * largest step) + taps + 2
 *   table_rows      table rows a workgroup stages: what a block of the fastest-drifting stream can touch, at most L + 1 (the whole table);
 *                   a step within a few hundred ppm of 1 needs a handful
 *   lds_bytes       (window_samples rounded up to even) * 8 + table_rows * (taps + 1) * 4
 * dabgpu_resample_step_q62(in_rate_hz, out_rate_hz, ppm): in / out * (1 + ppm * 1e-6) rounded to the nearest Q2.62 value (0 for NaN,
 * rates that are not positive, or a result outside (0, 4)); dabgpu_resample_step is its inverse as a double.
 * dabgpu_resample_input_needed: the span [*first, *first + *count) of input indices that a call of n_out samples at `position` reads for
 * ONE stream (before wrap or zero-fill; *first may be negative), so that callers can size windows; *count = 0 for n_out = 0. */
#define DABGPU_RESAMPLE_PHASES 256
#define DABGPU_RESAMPLE_PHASE_BITS 8
#define DABGPU_RESAMPLE_TAPS 48
#define DABGPU_RESAMPLE_BLOCK 1024
#define DABGPU_RESAMPLE_DEFAULT_PASSBAND 0.375
typedef struct {
    uint64_t step_q62;
    int64_t offset_samples;
    uint64_t offset_frac_q62;
    float gain;
    int32_t reserved;
} dabgpu_resample_stream;
typedef struct {
    double max_step, passband_cycles, beta;
    double passband_error, alias_leakage, error;
    float table[(DABGPU_RESAMPLE_PHASES + 1) * DABGPU_RESAMPLE_TAPS];
} dabgpu_resample_filter;
typedef struct { uint32_t block_samples, window_samples, table_rows, lds_bytes; } dabgpu_resample_geometry;
int dabgpu_resample_design(double max_step, double passband_cycles, dabgpu_resample_filter *out);
int dabgpu_resample_plan(const dabgpu_resample_stream *params, size_t n_streams, const dabgpu_resample_filter *design,
                         dabgpu_resample_geometry *out);
uint64_t dabgpu_resample_step_q62(double in_rate_hz, double out_rate_hz, double ppm);
double dabgpu_resample_step(uint64_t step_q62);
int dabgpu_resample_input_needed(const dabgpu_resample_stream *params, uint64_t position, size_t n_out, int64_t *first, uint64_t *count);

/* Resampler bank: the parameters of n_streams streams, the design's table and the streams' common position on the device.  The contract
 * is the channel bank's, point for point: d_in with a stride (even, >= n_in) or shared (0), d_in and d_out 16-byte aligned, out_stride_bytes
 * 0 or a multiple of 16 that holds n_out samples, complex float (DABGPU_IQ_RAW_F32L) or u8 pairs with u8_scale (DABGPU_IQ_RAW_U8); nothing
 * else is written.  A call is two launches on `stream` -- the resampling kernel, then a one-thread kernel that adds n_out to the position
 * -- and changes no host state, so it may be captured in a HIP graph; replays continue the stream.  _seek sets the position (0 at
 * creation, at most DABGPU_CHANNEL_MAX_POSITION), _set_params replaces all parameters; both are ordered on `stream`.  The geometry is
 * fixed when the bank is created: _set_params refuses (DABGPU_ERR_INVALID_ARG) parameters that need a larger window or more table rows, or
 * a step above the design's max_step.  Streams of one launch may have different steps.  Arguments are checked before any device call
 * (dabgpu_host_logic.cpp; tests/test_resample_plan.py, tests/cpp/resample_plan_fuzz.cpp, tests/test_gpu_resample.py). */
typedef struct dabgpu_resample_bank dabgpu_resample_bank;
int dabgpu_resample_bank_create(dabgpu_ctx *ctx, size_t n_streams, const dabgpu_resample_stream *h_params,
                                const dabgpu_resample_filter *design, dabgpu_resample_bank **out);
void dabgpu_resample_bank_destroy(dabgpu_resample_bank *bank);
int dabgpu_resample_bank_set_params(dabgpu_resample_bank *bank, const dabgpu_resample_stream *h_params, void *stream);
int dabgpu_resample_bank_seek(dabgpu_resample_bank *bank, uint64_t position, void *stream);
int dabgpu_resample_bank_apply(dabgpu_resample_bank *bank, const float *d_in, size_t in_stride_samples, size_t n_in, int wrap, size_t n_out,
                               void *d_out, int out_format, size_t out_stride_bytes, float u8_scale, void *stream);
/* the same from and to host memory on the context's stream, with the rules of dabgpu_channel_bank_apply_host_sync */
int dabgpu_resample_bank_apply_host_sync(dabgpu_resample_bank *bank, const float *h_in, size_t in_stride_samples, size_t n_in, int wrap,
                                         size_t n_out, void *h_out, int out_format, size_t out_stride_bytes, float u8_scale);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Channeliser: wideband captures to DAB blocks and back.  A wideband tuner writes several Band III blocks, 1.712 MHz apart, into one
 * 8.192 / 10.24 / 16.384 MS/s capture; SPLIT is a frequency-translating, integer-decimating bank that turns one such stream into up to
 * DABGPU_CHANNELISER_MAX_CHANNELS block streams, COMBINE is its transpose (block streams at their offsets and levels onto one wideband
 * stream, for the simulator).  A rate that is no integer multiple of the block rate is left to the resampler behind the channeliser
 * (10 MS/s -> split by 4 -> 2.5 MS/s -> resampler -> 2.048 MS/s).  The reference has nothing comparable; the definition is this library's
 * own, written once in dab-radio_amd/csrc/channelise_core.h for the kernels (channelise.hip) and for the host model of the tests
 * (tests/cpp/channelise_host_model.cpp), pinned to an independent numpy model (tests/channelise_model.py) and on the device bit for bit to
 * the host model (tests/test_gpu_channelise.py).  Design table, error bound and measurements: DESIGN.md 4.20.
 *
 * Table.  dabgpu_channeliser_design(decim, passband_cycles, stopband_cycles, *out), host only, double throughout: D = decim in 1..8,
 * K = DABGPU_CHANNELISER_TAPS_PER_PHASE * D taps.  h[j] = 2 f_c / D * sinc(2 f_c t / D) * kaiser(t), t = j - P in wideband samples, under the
 * resampler's Kaiser window (beta = 9.25, I0 by its series, argument 2 t / K, zero from |2 t / K| = 1 on); f_c lies half way between the
 * two edges, which are given in cycles per sample of the BLOCK rate (0 = the defaults 0.375, the 768 kHz edge of a block at 2.048 MS/s,
 * and 0.4609375, the 944 kHz edge of the next block); the table is divided by its sum (DC gain 1).  The peak sits on tap P = K / 2 - 1 as in
 * the resampler: block sample m is time-aligned with wideband sample m * D, so frame positions divide exactly.  D = 1: K = 1, h = {1}, P = 0:
 * mixing only.  The function returns the table's own error on a grid of 16 K + 1 frequencies per band, in cycles per wideband sample:
 *   passband_error   worst |H(f) - 1| over [0, passband / D],  H(f) = sum_j h[j] e^(-2 pi i f (j - P))
 *   stopband_level   worst |H(f)| over [stopband / D, 0.5]
 *   error            their sum: 5.3e-5 for D = 2..8 at the default edges, inside the resampler's 1e-4 (-80 dB) target; 0 for D = 1
 * Refused with DABGPU_ERR_INVALID_ARG: a null result, D outside 1..8, an edge that is NaN or negative, passband >= stopband (no
 * transition), stopband above 0.5 * D (beyond what the wideband stream can hold).
 *
 * Split.  Channel c of input stream s has freq_q64 (cycles per WIDEBAND sample, two's complement), phase0_q64 and gain.  With the bank's
 * 64-bit output position pos, the bank's `start` and wideband input x_s[0 .. n_in):
 *   v_c[n] = x_s[n] rotated by (cos, sin)(-(phase0 + n * freq)): the 64-bit phase is exact, its angle the top 24 bits (ch_osc_cycles,
 *            ch_cos_sin of the channel model), the product order the channel model's; both words 0 skip the rotation
 *   y_c[m] = gain * sum_{j < K} h[j] * v_c[(pos + m) * D + start - P + j], re and im one chain each in ascending j, the first term the plain
 *            product and every later one fmaf, the gain last
 * Samples outside the input are zero, or (wrap) the index is taken modulo n_in; the oscillator always sees the absolute index n, so a + b
 * outputs equal a and then b at any split and replays of a captured call continue the stream.  D = 1 with both words 0 and gain 1 returns
 * the input shifted by `start`, bit for bit.  Mix-then-filter is the definition on purpose: the table stays real and bank-wide, and a
 * channel is three words that _set_params can replace under a captured graph.
 *
 * Combine, the transpose over the same table: block streams x_c[0 .. n_in), wideband output sample n = pos + i:
 *   u_c[n] = D * sum_m h[n - start - m * D + P] * x_c[m] over the m whose tap index lies in [0, K): K / D taps, ascending m, chained as above
 *   y[n]   = sum_c rot(gain_c * u_c[n], +(phase0_c + n * freq_c)), channels in list order, the first term starts the sum, every later one
 *            is added (re and im each one plain addition)
 * as complex float or the u8 pairs of the modulator's quantiser.  Position, splitting and wrap rules are those of the split.
 *
 * dabgpu_channeliser_plan (host only): a channel list against a design.  Refused with DABGPU_ERR_INVALID_ARG: a null pointer, n_streams
 * outside 1..1048576, n_channels outside 1..8 n_streams, a channel whose `stream` is >= n_streams or below its predecessor's (the list is
 * sorted by stream), more than 8 channels on one stream, a gain that is not finite, |start| above DABGPU_CHANNELISER_MAX_START.  Geometry:
 *   split_tile / combine_tile       output samples one workgroup produces (combine: DABGPU_CHANNELISER_COMBINE_ROWS * D)
 *   split_window / combine_window   input samples it stages per stream / per channel
 *   split_lds_bytes / combine_lds_bytes
 * dabgpu_channeliser_freq_q64(offset_hz, rate_hz): offset / rate as the nearest Q64 word; 0 for NaN, a rate that is not positive, or an
 * offset outside +- half the rate (+- half itself is accepted: both are the word 2^63).
 * dabgpu_channeliser_input_needed(decim, position, start, n_out, *first, *count): the span of wideband indices that a split of n_out
 * samples at `position` reads (before wrap or zero-fill; *first may be negative; *count = 0 for n_out = 0).
 * dabgpu_channeliser_decim_for(rate_hz): the largest D <= 8 with rate / D >= 2.048 MHz; 0 when there is none (NaN, below 2.048 MHz). */
#define DABGPU_CHANNELISER_TAPS_PER_PHASE 72
#define DABGPU_CHANNELISER_MAX_DECIM 8
#define DABGPU_CHANNELISER_MAX_CHANNELS 8                     /* per stream */
#define DABGPU_CHANNELISER_SPLIT_TILE 512
#define DABGPU_CHANNELISER_COMBINE_ROWS 128                   /* block-rate positions per workgroup: a tile is 128 D wideband samples */
#define DABGPU_CHANNELISER_DEFAULT_PASSBAND 0.375
#define DABGPU_CHANNELISER_DEFAULT_STOPBAND 0.4609375
#define DABGPU_CHANNELISER_MAX_POSITION ((int64_t)1 << 58)    /* outputs; (position + n_out) * 8 + start stays a signed 64-bit number */
#define DABGPU_CHANNELISER_MAX_START ((int64_t)1 << 61)
typedef struct {
    uint64_t freq_q64, phase0_q64;
    float gain;
    uint32_t stream;                                          /* split: the input stream it reads; combine: the output stream it joins */
} dabgpu_channeliser_channel;
typedef struct {
    int32_t decim, taps;
    double passband_cycles, stopband_cycles, cutoff_cycles, beta;
    double passband_error, stopband_level, error;
    float table[DABGPU_CHANNELISER_TAPS_PER_PHASE * DABGPU_CHANNELISER_MAX_DECIM];
} dabgpu_channeliser_filter;
typedef struct {
    uint32_t decim, taps, split_tile, split_window, split_lds_bytes, combine_tile, combine_window, combine_lds_bytes;
} dabgpu_channeliser_geometry;
int dabgpu_channeliser_design(int decim, double passband_cycles, double stopband_cycles, dabgpu_channeliser_filter *out);
int dabgpu_channeliser_plan(const dabgpu_channeliser_channel *channels, size_t n_channels, size_t n_streams, int64_t start,
                            const dabgpu_channeliser_filter *design, dabgpu_channeliser_geometry *out);
uint64_t dabgpu_channeliser_freq_q64(double offset_hz, double rate_hz);
int dabgpu_channeliser_input_needed(int decim, uint64_t position, int64_t start, size_t n_out, int64_t *first, uint64_t *count);
int dabgpu_channeliser_decim_for(double rate_hz);

/* Channeliser bank: the design's table, n_channels channels on n_streams wideband streams, `start` and the position on the device.  The
 * buffer rules are the channel bank's.  Split: d_in holds n_streams wideband rows (in_stride_samples even and >= n_in, or 0 = one shared
 * row), d_out n_channels rows of n_out complex float, row c = channel c of the list.  Combine: d_in holds n_channels block rows, d_out
 * n_streams rows of n_out wideband samples, complex float or u8 pairs; a stream with no channel is written as zeros.  d_in and d_out
 * 16-byte aligned, out_stride_bytes 0 or a multiple of 16 that holds n_out samples; nothing else is written.  A call is two launches on
 * `stream` -- the kernel, then a one-thread kernel that adds n_out to the position -- and changes no host state: it may be captured in a
 * HIP graph and replays continue the stream.  The position counts output samples of the calls made (block samples for a split, wideband
 * samples for a combine; one bank serves one direction at a time), 0 at creation; _seek sets it (at most
 * DABGPU_CHANNELISER_MAX_POSITION).  _set_params replaces every channel and `start`, ordered on `stream`; the tile, window and LDS bytes
 * and the room for the list are fixed at creation, so it refuses (DABGPU_ERR_INVALID_ARG) a list with more channels than the bank was
 * created with (fewer are accepted: the rows of the channels left out are not written) and whatever dabgpu_channeliser_plan refuses.
 * The decimation is the design's and cannot change in a bank: tile, window and LDS bytes depend on it alone, so the channel count is
 * all of the plan that a new list can exceed.
 * Above 48 KB of LDS (split, D >= 6) the kernel's limit is raised once at creation. */
typedef struct dabgpu_channeliser_bank dabgpu_channeliser_bank;
int dabgpu_channeliser_bank_create(dabgpu_ctx *ctx, const dabgpu_channeliser_channel *h_channels, size_t n_channels, size_t n_streams,
                                   int64_t start, const dabgpu_channeliser_filter *design, dabgpu_channeliser_bank **out);
void dabgpu_channeliser_bank_destroy(dabgpu_channeliser_bank *bank);
int dabgpu_channeliser_bank_set_params(dabgpu_channeliser_bank *bank, const dabgpu_channeliser_channel *h_channels, size_t n_channels,
                                       int64_t start, void *stream);
int dabgpu_channeliser_bank_seek(dabgpu_channeliser_bank *bank, uint64_t position, void *stream);
int dabgpu_channeliser_bank_split(dabgpu_channeliser_bank *bank, const float *d_in, size_t in_stride_samples, size_t n_in, int wrap,
                                  size_t n_out, float *d_out, size_t out_stride_bytes, void *stream);
int dabgpu_channeliser_bank_split_host_sync(dabgpu_channeliser_bank *bank, const float *h_in, size_t in_stride_samples, size_t n_in, int wrap,
                                            size_t n_out, float *h_out, size_t out_stride_bytes);
int dabgpu_channeliser_bank_combine(dabgpu_channeliser_bank *bank, const float *d_in, size_t in_stride_samples, size_t n_in, int wrap,
                                    size_t n_out, void *d_out, int out_format, size_t out_stride_bytes, float u8_scale, void *stream);
int dabgpu_channeliser_bank_combine_host_sync(dabgpu_channeliser_bank *bank, const float *h_in, size_t in_stride_samples, size_t n_in,
                                              int wrap, size_t n_out, void *h_out, int out_format, size_t out_stride_bytes, float u8_scale);

/* ------------------------------------------------------------------------------------------------------------------------------
 * TII: transmitter identification information in the NULL symbol of mode I, both directions (every other mode returns
 * DABGPU_ERR_INVALID_ARG).  The reference has no TII code; this section is the definition.  It is EN 300 401 clause 14.8.1 as recalled:
 * THE NUMBERING OF p FOLLOWS THE TABLE BELOW AND HAS NOT BEEN CHECKED AGAINST TABLE 38 of the standard.
 *
 * Pattern table: T[0 .. 69] = the 70 bytes with exactly four bits set in ascending numeric order (T[0] = 0x0F, T[1] = 0x17, T[2] = 0x1B,
 * ..., T[69] = 0xF0); a_b(p) = bit 7 - b of T[p], b = 0 .. 7.  dabgpu_tii_pattern(p) = T[p], -1 outside [0, 70).
 * Carriers of the transmitter with main id p in [0, 70) and sub id c in [0, 24): for every b with a_b(p) = 1 and every block start
 * B in {-768, -384, +1, +385} the pair k0 = B + 2 c + 48 b and k0 + 1: 32 carriers in [-768, 768], none of them 0; carrier k sits in
 * bin k mod 2048.  dabgpu_tii_carriers writes them (b ascending, B ascending, k0 then k0 + 1).
 *
 * Transmit: the NULL spectrum is z[k0] += amp * PRS[k0], z[k0 + 1] += amp * PRS[k0] (both carriers of a pair carry the phase of k0; PRS =
 * the modulator's PRS spectrum, amp a real float, amp = 1 the power of a data carrier) for up to DABGPU_TII_MAX_TX transmitters, whose
 * spectra add in list order.  The NULL period is the inverse transform of z behind its last 608 samples, through the inverse transform,
 * frequency shift and quantiser of a data symbol.  A frame with no transmitter keeps its zeros: TII is sent in alternate frames, the
 * caller says per frame.
 *   dabgpu_ofdm_modulate_frames_tii: dabgpu_ofdm_modulate_frames plus d_tii [n_frames][DABGPU_TII_MAX_TX] and d_tii_count [n_frames] on
 *   the device (either NULL, or every count 0: the output of dabgpu_ofdm_modulate_frames bit for bit).  The lists are device memory, so
 *   the call cannot refuse their content: the kernel reads min(count, 4) entries and passes over an entry that dabgpu_tii_validate
 *   would refuse.  The _host_sync form validates its lists (main_id >= 70, sub_id >= 24, a count above 4, an amp that is not finite)
 *   and, like a mode other than I, refuses before any device call.
 *
 * Detect, per receiver and frame (dabgpu_tii_bank_process; one 256-thread workgroup per receiver, kernel launches only: asynchronous,
 * no host state changes, so a call may be captured in a HIP graph and replayed on the next frame's samples):
 *   1 window      the 2048 samples that begin 608 samples after the NULL's first sample; the NULL begins at null_offset_samples +
 *                 fine_time_offset of the receiver's dabgpu_sync_state (0 without records).  A record with sync_valid = 0 (or a
 *                 fine_time_offset outside [-504, 1543]) skips the receiver: accumulator, frame count and results untouched.
 *   2 offset      apply_pll with the record's freq_coarse + freq_fine (or d_freq_offset[k]; neither: 0), phase 0 at the window's first sample
 *   3 transform   forward, 2048 points, the demodulator's butterflies
 *   4 power       P[k] = fma(re, re, im * im)
 *   5 fold        for c < 24, b < 8, q_B = P[B + 2 c + 48 b] + P[B + 2 c + 48 b + 1]:  E[c][b] = (q_-768 + q_-384) + (q_+1 + q_+385)
 *   6 accumulate  acc[c][b] += E[c][b] (192 floats per receiver on the device), frames += 1
 *   7 decision    (decide != 0) every comb's eight values sorted; N = the mean over the 24 combs, in order of c, of the mean of each
 *                 comb's four smallest -- any transmitter leaves four of its comb's eight groups empty, so N is a noise floor whatever is
 *                 on the air.  A comb is active when its fourth largest value is >= threshold * N; its mask (bit 7 - b for group b) holds
 *                 the groups >= threshold * N.  A mask of four bits gives main_id by the table, any other main_id = -1 with the mask (two
 *                 main ids on one comb).  strength = mean of the masked groups / N.  N = 0 (no energy at all): no record.
 *                 d_results [n][24] records in ascending sub_id, d_counts [n].
 * Default threshold 2.16: under noise alone an accumulated group is a sum of 8 * frames unit exponentials, a Gamma(8 * frames, 1)
 * variable.  Splitting a comb's event by which four groups are its smallest gives P(comb active) = 70 E[S(max(t, max a))^4] with
 * t = threshold * (23 N' + mean a) / 24, a = four independent Gamma draws, N' the floor of the other 23 combs, S the Gamma survival
 * function; P(any of 24 combs) = 24 P to within 1e-12.  At frames = 2 this is 1.20e-6 at 2.15 and 0.93e-6 at 2.16 (root 2.157): 2.16 is
 * the smallest threshold, in steps of 0.01, with fewer than 1e-6 false decisions (tests/tii_model.py, asserted by tests/test_tii_model.py).
 * More frames only lower the probability.
 * The decision needs a noise floor: on a signal without noise N is the float32 rounding of the transforms, which is not flat, and what
 * is reported beside the transmitters is then undefined.
 * Records of a synchroniser: the record of the first frame after an acquisition is up to half a carrier spacing off (the coarse estimate
 * is a weighted mean of three bins and freq_fine takes its remainder through fmodf(., 0.505 spacings), the reference's arithmetic); half
 * a spacing off, a third of every pair's power falls into the combs c - 1 and c + 1.  The fine-frequency update has the record within
 * 0.05 spacings after that frame.  So do not feed the detector a receiver's first DABGPU_TII_SETTLE_FRAMES frames after sync_valid
 * turned 1 (or reset the bank after them); tests/test_tii_closed_loop.py pins both the exact settled loop and the unsettled frame.
 * Beyond the issue's list, kept deliberately: dabgpu_tii_main_id (the table look-up of step 7, shared with the kernel),
 * dabgpu_tii_validate (the refusal of the _host_sync modulator, callable before a device list is uploaded) and dabgpu_tii_bank_read
 * (a synchronous read-back of accumulators and frame counts for tests and diagnosis; no call on the hot path). */
#define DABGPU_TII_MAX_TX 4
#define DABGPU_TII_SETTLE_FRAMES 1
#define DABGPU_TII_NB_MAIN 70
#define DABGPU_TII_COMBS 24
#define DABGPU_TII_GROUPS 8
#define DABGPU_TII_DEFAULT_THRESHOLD 2.16f
typedef struct { uint8_t main_id, sub_id; float amp; } dabgpu_tii_tx;
typedef struct { float threshold; int32_t reserved; } dabgpu_tii_cfg;
typedef struct { int32_t sub_id, main_id; uint32_t mask; float strength; } dabgpu_tii_record;
void dabgpu_tii_cfg_default(dabgpu_tii_cfg *cfg);
int dabgpu_tii_pattern(int main_id);
int dabgpu_tii_main_id(uint32_t mask);                        /* inverse of dabgpu_tii_pattern, -1 for a mask that is no pattern */
int dabgpu_tii_carriers(int main_id, int sub_id, int out[32]);
/* n_frames lists of DABGPU_TII_MAX_TX entries and their counts, in host memory (counts NULL: no list is read) */
int dabgpu_tii_validate(const dabgpu_tii_tx *tii, const uint8_t *tii_count, size_t n_frames);
int dabgpu_ofdm_modulate_frames_tii(dabgpu_ctx *ctx, int transmission_mode, const uint8_t *d_payload, int payload_layout, size_t n_frames,
                                    const float *d_prs_fft_ref, float freq_norm, void *d_out, int out_format, void *stream,
                                    const dabgpu_tii_tx *d_tii, const uint8_t *d_tii_count);
int dabgpu_ofdm_modulate_frames_tii_host_sync(dabgpu_ctx *ctx, int transmission_mode, const uint8_t *h_payload, int payload_layout,
                                              size_t n_frames, const float *h_prs_fft_ref, float freq_norm, void *h_out, int out_format,
                                              const dabgpu_tii_tx *h_tii, const uint8_t *h_tii_count);
/* Detector bank: accumulators and frame counts of n_receivers receivers on the device (cfg NULL = the default).
 *   d_iq      receiver k's samples: complex float at d_iq + 2 * k * stream_stride_samples, 8-byte aligned (16-byte aligned windows are
 *             read with 16-byte loads); stream_stride_samples >= null_offset_samples + 2656, + 1543 more when d_states is given
 *   d_states  [n] the records dabgpu_ofdm_sync / dabgpu_ofdm_sync_demod_frames left (read only), or NULL
 *   d_freq_offset  [n] cycles per sample, or NULL: receiver k is rotated by d_freq_offset[k] instead of its record's sum unless that
 *             value is NaN (position and validity stay the record's); without records it is the only offset
 *   d_results, d_counts  required when decide != 0
 * _reset clears accumulators and frame counts on `stream`; _read copies them to host memory behind everything queued on `stream` and
 * waits (h_acc [n][192], h_frames [n], either may be NULL).  The _host_sync form serves a bank of one receiver from host memory:
 * h_iq holds n_samples samples, the NULL begins at null_offset_samples + fine_time_offset, which must leave the window inside them. */
typedef struct dabgpu_tii_bank dabgpu_tii_bank;
int dabgpu_tii_bank_create(dabgpu_ctx *ctx, size_t n_receivers, const dabgpu_tii_cfg *cfg, dabgpu_tii_bank **out);
void dabgpu_tii_bank_destroy(dabgpu_tii_bank *bank);
int dabgpu_tii_bank_reset(dabgpu_tii_bank *bank, void *stream);
int dabgpu_tii_bank_process(dabgpu_tii_bank *bank, const float *d_iq, size_t stream_stride_samples, size_t null_offset_samples,
                            const dabgpu_sync_state *d_states, const float *d_freq_offset, int decide, dabgpu_tii_record *d_results,
                            uint32_t *d_counts, void *stream);
int dabgpu_tii_bank_process_host_sync(dabgpu_tii_bank *bank, const float *h_iq, size_t n_samples, size_t null_offset_samples,
                                      float freq_offset, int fine_time_offset, int decide, dabgpu_tii_record *h_results, uint32_t *h_count);
int dabgpu_tii_bank_read(dabgpu_tii_bank *bank, float *h_acc, uint32_t *h_frames, void *stream);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Ingest pipe: the host -> device hand-over of capture bytes.  Replaces the reader thread -> OFDM_Demod::Process hand-over
 * of examples/app_helpers/app_ofdm_blocks.h:45-58 and the memcpy of OFDM_Demod::ReadSymbols (src/ofdm/ofdm_demodulator.cpp:550-577).
 * A ring of `depth` PINNED host buffers with device twins and a copy stream of its own:
 *     dabgpu_ingest_acquire(pipe, &h)            fill h (e.g. fread straight into it; capture format, 2 B per sample for raw_u8)
 *     dabgpu_ingest_submit(pipe, bytes, &d)      asynchronous copy on the pipe's copy stream; d = device twin
 *     dabgpu_ingest_wait(pipe, d, s)             stream s waits for the copy into d (right before the kernels that read it: a batch may be copied ahead)
 *     ... enqueue kernels reading d on s (dabgpu_ofdm_demod_frames_raw, dabgpu_stream_bank_process_raw, ...)
 *     dabgpu_ingest_consumed(pipe, d, s)         d may be overwritten once those kernels have run
 * With depth >= 2 the copy of batch k + 1 overlaps the demodulation of batch k; acquire blocks only while the ring is full.
 * One pipe = one producer thread. */
typedef struct dabgpu_ingest dabgpu_ingest;
int dabgpu_ingest_create(dabgpu_ctx *ctx, size_t buffer_bytes, int depth, dabgpu_ingest **out);
void dabgpu_ingest_destroy(dabgpu_ingest *pipe);
int dabgpu_ingest_acquire(dabgpu_ingest *pipe, void **h_buffer);
int dabgpu_ingest_submit(dabgpu_ingest *pipe, size_t bytes, void **d_buffer);
int dabgpu_ingest_wait(dabgpu_ingest *pipe, const void *d_buffer, void *compute_stream);
int dabgpu_ingest_consumed(dabgpu_ingest *pipe, const void *d_buffer, void *compute_stream);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Channel BER: the channel ("pre-Viterbi") bit error rate of every code word a decode call has decoded, without knowing what was sent.
 * The decoded bytes are encoded again and compared with the hard decisions of the soft bits the decoder consumed.  For one code word of
 * K = kept_bits of its dabgpu_tx_encode_plan entry (a FIB group: 2304):
 *   s_i   the soft bit the decoder consumed at position i < K: FIC, soft bit i of the FIB group; MSC, what CIF_Deinterleaver delivers
 *         for that CIF (bit i of the sub-channel comes from the CIF that is 15 - bitrev4(i mod 16) CIFs older, read from the same ring
 *         and in the same layout as dabgpu_msc_decode_frames_layout reads it)
 *   e_i   bit i of the code word the channel encoder makes of the decoder's output bytes AS THEY STAND (the 96 bytes of a FIB group with
 *         the received CRC bytes, or the sub-channel's bytes of that CIF): energy dispersal, K = 7 rate-1/4 code with zero tail,
 *         puncturing -- the schedule of dabgpu_tx_encode_plan; nothing is corrected or recomputed
 *   h_i   = (s_i >= 0), as dabgpu_soft_bits_to_hard_bytes decides; |s_i| in integer arithmetic, |-128| = 128
 * Soft bits of the capacity units beyond K are not read.  Every field is an integer: the results have no tolerance. */
typedef struct {
    uint32_t n_bits;        /* positions i < K with s_i != 0 (a 0 is an erasure: not compared) */
    uint32_t n_errors;      /* of those, h_i != e_i */
    uint32_t error_weight;  /* sum of |s_i| over the error positions */
    uint32_t total_weight;  /* sum of |s_i| over all i < K */
} dabgpu_ber_result;

/* dabgpu_ber_plan (host only, no device): the launch a dabgpu_ber_frames_layout call with these arguments makes, FIC and MSC both.
 * Refuses with DABGPU_ERR_INVALID_ARG and the reason in dabgpu_last_error(), in this order: a sub-channel count outside 0..64 (or a null
 * list); a descriptor dabgpu_subchannel_validate refuses, in list order; a multiplex dabgpu_tx_encode_plan refuses (two sub-channels that
 * overlap); n_ensembles outside 1..1048576; an unknown bits_layout; history_frames < 5; ensemble_stride < history_frames x 230400 or not
 * a multiple of 16; out_ensemble_stride < 4 x the CIF's decoded bytes or not a multiple of 4 (n_sub > 0 only).  n_sub = 0 is legal: FIC
 * only. */
typedef struct {
    uint32_t n_sub;
    uint32_t codewords_per_ensemble;    /* 4 x n_sub sub-channel code words + 4 FIB groups: one wavefront each */
    uint32_t cif_bytes;                 /* decoded bytes of one CIF of all sub-channels (dabgpu_tx_encode_plan's cif_in_bytes) */
    uint32_t n_sched;                   /* entries of the multiplex's kept-bit schedules */
    uint32_t sched_offset[65];          /* first schedule entry of sub-channel s; [n_sub] = the FIB group's */
    uint32_t max_kept_bits;             /* K of the longest code word */
    uint32_t lds_bytes;                 /* LDS one wavefront holds its code word in: whole blocks of 512 bits */
    uint32_t waves_per_block, block_threads;
    uint32_t grid;                      /* workgroups */
} dabgpu_ber_geometry;
int dabgpu_ber_plan(const dabgpu_subchannel *subs, int n_sub, size_t n_ensembles, int history_frames, size_t ensemble_stride,
                    size_t out_ensemble_stride, int bits_layout, dabgpu_ber_geometry *out);

/* The batch forms.  The arguments are those of dabgpu_decode_frames_layout / dabgpu_decode_ring_layout, whose outputs d_fib_bytes
 * [n_ensembles][4][96] and d_msc_out are inputs here; d_fic_ber [n_ensembles][4], d_msc_ber [n_ensembles][4][n_sub].  A half whose bytes
 * or records are NULL is skipped (and the MSC half when n_subchannels = 0).  d_bits_history 16-byte aligned, the byte and record
 * pointers 4- and 16-byte aligned.  Ring form: an ensemble with a negative slot gets all-zero records.  One launch, one pass over the
 * soft bits, nothing intermediate in device memory; a steady-state call enqueues that kernel only and may be captured in a HIP graph
 * (the first call with a multiplex uploads its tables, as the decoders do: run once before capturing). */
int dabgpu_ber_frames_layout(dabgpu_ctx *ctx, const int8_t *d_bits_history, size_t n_ensembles, size_t ensemble_stride, int history_frames,
                             int newest_frame_slot, const dabgpu_subchannel *h_subchannels, int n_subchannels, const uint8_t *d_fib_bytes,
                             const uint8_t *d_msc_out, size_t out_ensemble_stride, dabgpu_ber_result *d_fic_ber,
                             dabgpu_ber_result *d_msc_ber, int bits_layout, void *stream);
int dabgpu_ber_ring_layout(dabgpu_ctx *ctx, const int8_t *d_hist, size_t n_ensembles, size_t ensemble_stride, int history_frames,
                           const int32_t *d_newest_slot, const dabgpu_subchannel *h_subchannels, int n_subchannels,
                           const uint8_t *d_fib_bytes, const uint8_t *d_msc_out, size_t out_ensemble_stride, dabgpu_ber_result *d_fic_ber,
                           dabgpu_ber_result *d_msc_ber, int bits_layout, void *stream);
/* One code word from and to host memory, synchronous, on the context's stream (the mirror layer's forms): a FIB group's 2304 soft bits
 * and 96 decoded bytes; a sub-channel's de-interleaved CIF (length x 64 soft bits, of which the first K are read) and its decoded bytes */
int dabgpu_ber_fib_group_host_sync(dabgpu_ctx *ctx, const int8_t *h_bits /*[2304]*/, const uint8_t *h_bytes /*[96]*/, dabgpu_ber_result *result);
int dabgpu_ber_codeword_host_sync(dabgpu_ctx *ctx, const dabgpu_subchannel *sc, const int8_t *h_deinterleaved_bits, const uint8_t *h_bytes,
                                  dabgpu_ber_result *result);

/* ------------------------------------------------------------------------------------------------
 * Receive diversity: the DQPSK products of several receivers of one ensemble (antennas, tuners, sites) combined into one frame of soft
 * bits.  A differential product carries no channel phase, so the products of K branches add coherently carrier by carrier, each
 * weighted by the channel amplitude it keeps (the amplitude DABGPU_SOFT_CSI keeps: every branch is demodulated under that policy with
 * one level L, its products are the demodulator's d_dqpsk view, its scale k_b the demodulator's d_soft_scale word).
 *   live branch   its sync record, if given, has sync_valid != 0; its scale k_b is finite and > 0; its weight w_b (1 without a weight
 *                 pointer) is finite and > 0.  The products of a branch that is not live are never read.
 *   sum           over the live branches in branch order: the first contributes w_b * c, the next ones fmaf(w_b, c_b, sum), c = re d
 *                 and im d.  w_b = 1 / (noise power of branch b) is the maximal-ratio weight; receivers of equal noise take 1.
 *   scale         k = 1 / sum_live (w_b / k_b) = L 1536 / (2048 sum w_b P_b); 0 -- every soft bit of the frame 0 -- without a live
 *                 branch, or where that sum is not a normal number.  One live branch of weight exactly 1: k = k_b, so that K = 1
 *                 reproduces the demodulator's weighted soft bits bit for bit.
 *   soft bits     -(c k) of the sum, c = re and -im, NaN -> 0, clamped to [-127, 127], truncated; frequency de-interleave and both
 *                 layouts (DABGPU_BITS_NATURAL / DABGPU_BITS_MSC_CLASSED) exactly as the demodulator's.
 * Arithmetic: csrc/diversity_core.h; the device equals dabgpu_diversity_scale_host and the tests' host model bit for bit.
 */
#define DABGPU_DIVERSITY_MAX_BRANCHES 8
typedef struct {
    const float *d_dqpsk;                 /* [n_frames][75][1536] complex float, 16-byte aligned */
    const float *d_scale;                 /* [n_frames] k_b */
    const float *d_weight;                /* [n_frames] w_b, may be NULL: weight 1 */
    const dabgpu_sync_state *d_sync;      /* [n_frames], may be NULL: every frame of the branch was demodulated */
} dabgpu_diversity_branch;
typedef struct { uint32_t symbols_per_block, runs_per_frame, grid, threads, lds_bytes; } dabgpu_diversity_geometry;
/* What a dabgpu_diversity_combine_frames call with these arguments launches; needs no device (no address is dereferenced, h_branches is
 * a table in host memory).  DABGPU_ERR_INVALID_ARG, with the reason in dabgpu_last_error, for: a null table or result; n_branches
 * outside 1 .. DABGPU_DIVERSITY_MAX_BRANCHES; n_frames above 2^24; an unknown bits_layout; symbols_per_block outside 0 .. 75;
 * bits_frame_stride neither 0 nor a multiple of 16 >= 230400; d_bits null or not 16-byte aligned; a branch without products or scales,
 * products that are not 16-byte aligned, scales / weights / records that are not 4-byte aligned.  symbols_per_block = 0: the planner
 * chooses (short runs for small batches, so that the launch still spreads over the chip); the result never depends on it. */
int dabgpu_diversity_plan(const dabgpu_diversity_branch *h_branches, int n_branches, size_t n_frames, const int8_t *d_bits,
                          size_t bits_frame_stride, int bits_layout, int symbols_per_block, dabgpu_diversity_geometry *out);
/* n_frames frames of n_branches branches -> d_bits + frame * bits_frame_stride (0 = 230400, packed; a larger stride writes into a
 * history ring and leaves the bytes between the slots alone).  d_soft_scale [n_frames] (may be NULL): k as used; d_live_mask [n_frames]
 * (may be NULL): bit b = branch b was live.  The table travels as a kernel argument: the call is ONE kernel launch, no copy, and may be
 * captured in a HIP graph. */
int dabgpu_diversity_combine_frames(dabgpu_ctx *ctx, const dabgpu_diversity_branch *h_branches, int n_branches, size_t n_frames,
                                    int8_t *d_bits, size_t bits_frame_stride, int bits_layout, int symbols_per_block,
                                    float *d_soft_scale, uint32_t *d_live_mask, void *stream);
/* One frame from and to host memory, synchronous, on the context's stream (the mirror layer's form): h_dqpsk[b] -> [75][1536] complex
 * float of branch b (not read where the branch is not live; may then be NULL), h_scale [n_branches], h_weight [n_branches] or NULL,
 * h_valid [n_branches] or NULL (0 = the branch's synchroniser refused the frame); h_bits [230400]; *h_soft_scale, *h_live_mask may be NULL */
int dabgpu_diversity_combine_host_sync(dabgpu_ctx *ctx, const float *const *h_dqpsk, const float *h_scale, const float *h_weight,
                                       const int *h_valid, int n_branches, int bits_layout, int8_t *h_bits, float *h_soft_scale,
                                       uint32_t *h_live_mask);
/* k of one frame on the host (w, valid may be NULL; *live_mask may be NULL); 0 for n_branches outside 1 .. 8 or a null k */
float dabgpu_diversity_scale_host(const float *k, const float *w, const int *valid, int n_branches, uint32_t *live_mask);
/* A synchronised diversity branch: dabgpu_ofdm_sync_demod_frames_soft in the natural layout that also writes the receivers' DQPSK
 * products, d_dqpsk [n_streams][75][1536] complex float (required, 16-byte aligned).  Bits, records, scales, total phases and
 * correlations are those of dabgpu_ofdm_sync_demod_frames_soft, bit for bit; the products those of dabgpu_ofdm_demod_frames_soft on the
 * shifted frames.  A receiver with sync_valid = 0 leaves its products untouched as well: its branch is dead through d_sync. */
int dabgpu_ofdm_sync_demod_frames_branch(dabgpu_ctx *ctx, const float *d_iq, size_t n_streams, size_t stream_stride_samples,
                                         size_t prs_offset_samples, const dabgpu_sync_cfg *cfg, dabgpu_sync_state *d_states,
                                         int8_t *d_bits, float *d_cp_corr, int symbols_per_block, size_t bits_frame_stride,
                                         float *d_total_phase, const dabgpu_soft_cfg *soft, float *d_soft_scale, float *d_dqpsk,
                                         void *stream);

/* ------------------------------------------------------------------------------------------------
 * Noise estimate: one frame's NULL symbol turned into a calibrated noise power, the frame's signal power and the maximal-ratio weight
 * w_b = 1 / (noise power) that "Receive diversity" takes, as arrays on the device (mode I; stateless, batched, one kernel launch per
 * call, no host state: a call may be captured in a HIP graph).  The reference has no such code; this section is the definition.
 * Per frame:
 *   1 energies    steps 1 to 5 of the TII detector, statement for statement: the 2048 samples that begin 608 samples after the NULL's
 *                 first sample (the NULL begins at null_offset_samples + fine_time_offset of the frame's dabgpu_sync_state, 0 without
 *                 records), apply_pll with the record's freq_coarse + freq_fine (d_freq_offset[k] instead unless it is NaN; neither:
 *                 0), the demodulator's 2048-point transform, P[k] = fma(re, re, im * im), the fold into E[24][8].  The 192 values
 *                 equal, bit for bit, the accumulator of a freshly reset dabgpu_tii_bank after one _process of the same samples.
 *   2 floor       F = the mean over the 24 combs, in order of c, of the mean of each comb's four smallest groups: the detector's own
 *                 statistic at one frame.  Any transmitter leaves four of its comb's eight groups empty.
 *   3 calibration noise_power N = F * dabgpu_noise_unbias().  Under white noise of power s2 per complex sample a group is 2048 s2 times
 *                 a Gamma(8, 1) draw; with mu = E[mean of the four smallest of eight independent such draws] = 5.982762381925 the
 *                 constant is 8 / (mu * 8 * 2048) = 8.161468e-05 as one float, and E[N] = s2.  One frame's N has a relative standard
 *                 deviation of 0.0319 (0.14 dB).  Derivation and variance: tests/noise_model.py.
 *   4 signal      signal_power P = the sum of |x|^2 over the useful part of the phase reference symbol, samples 504 .. 2551 behind the
 *                 NULL's 2656, not rotated, in the demodulator's summation tree: the weighted soft bits' scale of (level, P) is the
 *                 demodulator's d_soft_scale word of that frame bit for bit.  P is a sum over 2048 samples of signal plus noise, N a
 *                 power per sample: the mean signal-to-noise ratio per sample is (P / 2048 - N) / N.
 *   5 outputs     weight = 1 / max(N, P * 2^-40): the cap holds P * weight at 2^40 (120 dB), so a branch without noise (a synthetic
 *                 one) is live with a finite weight, not dead.  The reciprocal is Newton's in fmaf on the mantissa, the exponent
 *                 mirrored exactly: at most 1 ulp from the correctly rounded quotient.  snr = max(P - N, 0) * weight, a plain ratio
 *                 of the two outputs (decibels, and the 2048 of step 4, are the caller's).
 *   skipped       a record with sync_valid = 0, a fine_time_offset outside [-504, 1543] or one that puts the NULL's first sample in
 *                 front of the frame's slice (null_offset_samples + fine_time_offset < 0): none of the frame's samples is read.  P or
 *                 N not finite, P not above 0, or max(N, P * 2^-40) below the normal range (no finite weight).  A skipped frame
 *                 writes 0 to EVERY output, group energies included, and clears d_valid[k] -- a stale weight can never be applied,
 *                 and weight 0 is a dead branch for the combiner.
 * Limits: T strong TII transmitters on distinct combs raise E[N] by (24 + T (8 / mu - 1)) / 24 -- such a comb's four smallest groups
 * are its four empty ones, plain draws of mean 8 -- which is 1.0140 at T = 1 and 1.0562 (0.24 dB) at T = 4.  Two main ids on ONE comb
 * may leave that comb no empty group; its share is then signal, and the bias is not bounded (stated, not fixed).  A carrier offset of
 * up to half a spacing moves power into the combs c - 1 and c + 1 at the same group index, so every comb keeps four empty groups.
 * Echoes of the previous frame up to 608 samples long stay in front of the window.  As for TII, the record of the first frame after
 * an acquisition may be half a spacing off; that only matters with TII on the air.  No smoothing across frames: average noise_power.
 * Arithmetic: csrc/noise_core.h; the device equals dabgpu_noise_floor_host and the tests' host model bit for bit.
 */
typedef struct { float noise_power, signal_power, weight, snr; uint32_t valid; } dabgpu_noise_record;
typedef struct { uint32_t grid, threads, lds_bytes; } dabgpu_noise_geometry;
/* What a dabgpu_noise_estimate_frames call with these arguments launches; needs no device (no address is dereferenced).
 * DABGPU_ERR_INVALID_ARG, with the reason in dabgpu_last_error, for: a null result; a transmission_mode other than 1; n_frames of 0 or
 * above 2^24; d_iq null or not 8-byte aligned; records, offsets or outputs that are not 4-byte aligned; stream_stride_samples below
 * null_offset_samples + 2656 + 2552, + 1543 more when d_states is given (either above 2^40); no output at all (d_valid counts as one). */
int dabgpu_noise_plan(int transmission_mode, const float *d_iq, size_t n_frames, size_t stream_stride_samples, size_t null_offset_samples,
                      const dabgpu_sync_state *d_states, const float *d_freq_offset, const float *d_noise_power,
                      const float *d_signal_power, const float *d_weight, const float *d_snr, const float *d_group_energy,
                      const uint32_t *d_valid, dabgpu_noise_geometry *out);
/* d_iq, stream_stride_samples and null_offset_samples = prs_offset_samples - 2656 are those of dabgpu_ofdm_sync_demod_frames_branch and
 * d_states the records it left, so the call sits behind a branch's demodulation with no copy (16-byte aligned windows are read with
 * 16-byte loads, others with 8-byte loads).  Every output is optional: d_noise_power, d_signal_power, d_weight, d_snr [n_frames]
 * float (d_weight can be a dabgpu_diversity_branch's d_weight as it is), d_group_energy [n_frames][192], d_valid [n_frames] (1 or 0). */
int dabgpu_noise_estimate_frames(dabgpu_ctx *ctx, const float *d_iq, size_t n_frames, size_t stream_stride_samples,
                                 size_t null_offset_samples, const dabgpu_sync_state *d_states, const float *d_freq_offset,
                                 float *d_noise_power, float *d_signal_power, float *d_weight, float *d_snr, float *d_group_energy,
                                 uint32_t *d_valid, void *stream);
/* One frame from host memory, synchronous, on the context's stream: h_iq holds n_samples samples, the NULL begins at
 * null_offset_samples + fine_time_offset, and NULL and phase reference symbol (2656 + 2552 samples) must lie inside them.  A
 * fine_time_offset outside [-504, 1543], which the batched form skips, is refused here (DABGPU_ERR_INVALID_ARG), as is a frame that
 * leaves the samples; *out is then all zero */
int dabgpu_noise_estimate_host_sync(dabgpu_ctx *ctx, const float *h_iq, size_t n_samples, size_t null_offset_samples, float freq_offset,
                                    int fine_time_offset, dabgpu_noise_record *out);
float dabgpu_noise_unbias(void);
/* steps 2 .. 5 on the host (no device): 1 and the record, or 0 and a record of zeros for a skipped frame (or a null argument) */
int dabgpu_noise_floor_host(const float group_energy[192], float signal_power, dabgpu_noise_record *out);

/* ------------------------------------------------------------------------------------------------
 * Noise profile: one frame's NULL symbol turned into a noise power per frequency band and the maximal-ratio weights of the bands, for
 * a combiner that applies them carrier by carrier (mode I; batched, one kernel launch per call, no host state: a call may be captured
 * in a HIP graph; the smoothing state is the caller's array).  "Noise estimate" holds the noise of a branch to be white and gives it
 * one weight per frame; a narrowband interferer (a spur cluster, a co-channel carrier, a neighbour's shoulder) makes the carriers
 * under it the largest products of the frame, and under DABGPU_SOFT_CSI the most confident soft bits.  The reference has no such code;
 * this section is the definition.  Per frame:
 *   1 powers      steps 1 to 4 of the TII detector, statement for statement (window, rotation, transform, P[k] = fma(re, re, im * im):
 *                 the window, the records and d_freq_offset as "Noise estimate" step 1 reads them).  In the carrier order of d_dqpsk,
 *                 C[c] = P[1280 + c] for c < 768 (carriers -768 .. -1) and P[c - 767] for c >= 768 (carriers 1 .. 768); DC is left out.
 *                 d_carrier_power [n_frames][1536] (optional).
 *   2 bands       128 bands of 12 adjacent carriers, band b = carriers 12 b .. 12 b + 11: 64 bands on either side of DC, none
 *                 straddles it, and a pair of carriers 2 i, 2 i + 1 never straddles a band.  sum = the included carriers of the band
 *                 added one after the other in carrier order (the first included one starts the chain), count = how many were
 *                 included.  m_b = (sum * R[count]) * 2^-11, R[n] the float nearest 1 / n.  The transform is not normalised, so under
 *                 white noise of power s2 per complex sample E[C[c]] = 2048 s2 and E[m_b] = s2: no calibration constant.  One
 *                 frame's m_b is a mean of 12 unit exponentials: relative standard deviation 1 / sqrt(12).
 *   3 exclusion   d_exclude (optional): 48 words, bit c mod 32 of word c / 32 set = carrier c is left out of its band (the TII carriers
 *                 that are on the air: dabgpu_tii_carriers; carrier k of -768 .. 768 is c = k + 768 below DC and k + 767 above).  One
 *                 table serves all frames of the call.  A band whose 12 carriers are ALL excluded ignores the mask: it is measured from
 *                 all 12, since a band without a measurement would have no weight.
 *   4 smoothing   d_profile_in [n_frames][128] (optional: the previous n_b of each frame's receiver) and alpha in (0, 1]:
 *                 n_b = fmaf(alpha, m_b - p_b, p_b) where p_b is finite and > 0, n_b = m_b otherwise, so a zeroed buffer starts
 *                 cleanly.  Without d_profile_in n_b = m_b.  With independent frames the relative deviation settles at
 *                 sqrt(alpha / (2 - alpha)) / sqrt(12).  d_profile_out [n_frames][128] (optional) takes n_b; it may be d_profile_in
 *                 itself (in place); any other overlap is the caller's error.
 *   5 weights     M = the mean of the 128 n_b in a fixed tree: 64 + 64 values, each half folded pairwise with partner distance 32, 16,
 *                 8, 4, 2, 1 (the demodulator's wavefront tree), the two results added, times 2^-7.  w_b = 1 / max(n_b, M * 2^-20)
 *                 by the combiner's reciprocal (csrc/diversity_core.h, dv_reciprocal): a band is never weighted more than 60 dB
 *                 above the mean, and a band without noise (a synthetic signal) has a finite weight.  Where M * 2^-20 is below the
 *                 normal range and n_b below it as well, w_b is +infinity, which the combiner counts as 0.
 *                 d_band_weight [n_frames][128], d_mean_noise [n_frames] (= M), d_valid [n_frames] (1 or 0).
 *   skipped       a frame "Noise estimate" skips by its record (none of its samples is read), or whose M is not a normal positive
 *                 finite number (NaN, infinity, all zero).  It writes 0 to every band weight, to d_mean_noise and to d_carrier_power
 *                 and clears d_valid; d_profile_out takes d_profile_in unchanged, or 0 without one: a stale weight is never
 *                 applied, and the state survives.
 * Arithmetic: csrc/noise_profile_core.h; the device equals dabgpu_noise_profile_bands_host and the tests' host model bit for bit. */
#define DABGPU_NOISE_PROFILE_BANDS 128
#define DABGPU_NOISE_PROFILE_BAND_CARRIERS 12
#define DABGPU_NOISE_PROFILE_EXCLUDE_WORDS 48
/* What a dabgpu_noise_profile_frames call with these arguments launches; needs no device (no address is dereferenced).
 * DABGPU_ERR_INVALID_ARG, with the reason in dabgpu_last_error, for: a null result; a transmission_mode other than 1; n_frames of 0 or
 * above 2^24; d_iq null or not 8-byte aligned; records, offsets, tables or outputs that are not 4-byte aligned; stream_stride_samples
 * below null_offset_samples + 2656, + 1543 more when d_states is given (either above 2^40); alpha outside (0, 1] (NaN included);
 * d_profile_in and d_profile_out that overlap without being equal; no output at all (d_valid and d_profile_out count as outputs). */
int dabgpu_noise_profile_plan(int transmission_mode, const float *d_iq, size_t n_frames, size_t stream_stride_samples,
                              size_t null_offset_samples, const dabgpu_sync_state *d_states, const float *d_freq_offset,
                              const uint32_t *d_exclude, const float *d_profile_in, float alpha, const float *d_profile_out,
                              const float *d_band_weight, const float *d_mean_noise, const float *d_carrier_power,
                              const uint32_t *d_valid, dabgpu_noise_geometry *out);
/* d_iq, stream_stride_samples, null_offset_samples, d_states and d_freq_offset are those of dabgpu_noise_estimate_frames: the call sits
 * behind a branch's demodulation with no copy.  Every output is optional; d_band_weight can be an entry of
 * dabgpu_diversity_combine_frames_banded's h_band_weight as it is. */
int dabgpu_noise_profile_frames(dabgpu_ctx *ctx, const float *d_iq, size_t n_frames, size_t stream_stride_samples,
                                size_t null_offset_samples, const dabgpu_sync_state *d_states, const float *d_freq_offset,
                                const uint32_t *d_exclude, const float *d_profile_in, float alpha, float *d_profile_out,
                                float *d_band_weight, float *d_mean_noise, float *d_carrier_power, uint32_t *d_valid, void *stream);
/* One frame from host memory, synchronous, on the context's stream: h_iq holds n_samples samples, the NULL (2656 samples) begins at
 * null_offset_samples + fine_time_offset and must lie inside them; a fine_time_offset outside [-504, 1543] is refused.  h_exclude [48]
 * or NULL; h_profile [128] or NULL: the state, read and written in place; h_band_weight [128], h_mean_noise, h_carrier_power [1536]
 * may be NULL.  Returns DABGPU_OK with *h_valid (may be NULL) 1 or 0. */
int dabgpu_noise_profile_host_sync(dabgpu_ctx *ctx, const float *h_iq, size_t n_samples, size_t null_offset_samples, float freq_offset,
                                   int fine_time_offset, const uint32_t *h_exclude, float *h_profile, float alpha, float *h_band_weight,
                                   float *h_mean_noise, float *h_carrier_power, uint32_t *h_valid);
/* steps 2 to 5 on the host (no device) from the 1536 carrier powers of step 1: exclude [48] or NULL, profile_in [128] or NULL,
 * profile_out / band_weight [128] and mean_noise may be NULL (profile_out may be profile_in).  1 for a valid frame, 0 for a skipped
 * one (whose outputs are those of "skipped" above), -1 for a null carrier_power or an alpha outside (0, 1]. */
int dabgpu_noise_profile_bands_host(const float carrier_power[1536], const uint32_t *exclude, const float *profile_in, float alpha,
                                    float *profile_out, float *band_weight, float *mean_noise);
/* The exclusion words of step 3 from n transmitters' (main_id, sub_id): every carrier of dabgpu_tii_carriers set in out[48] (cleared
 * first).  DABGPU_ERR_INVALID_ARG for an id out of range or a null argument (n = 0: all clear). */
int dabgpu_noise_profile_exclude_tii(const uint8_t *main_ids, const uint8_t *sub_ids, int n, uint32_t out[48]);

/* Banded receive diversity: dabgpu_diversity_combine_frames with a noise profile per branch.  h_band_weight [n_branches] (host memory,
 * travels by value in the kernel argument like the branch table): entry b = a device pointer to [n_frames][128] band weights of
 * branch b, or NULL for a branch without one.  h_band_weight NULL, or every entry NULL: exactly dabgpu_diversity_combine_frames.  For
 * a branch with a table:
 *   d_weight      must be NULL (the planner refuses both)
 *   branch weight the mean of the frame's 128 band weights in the tree of "Noise profile" step 5, a band weight that is not positive
 *                 and finite counting as 0.  It takes the place of w_b in the live rule and in the scale, the exception for one live
 *                 branch of weight exactly 1 included.  The table of a frame is read whatever the branch's record says.
 *   sum           carrier c of the branch enters with the weight of band c / 12 (0 where that is not positive and finite) in place of w_b
 * A table that holds one normal value w in all 128 bands has the mean w exactly (for w < 2^121: above, the tree's sum overflows and the
 * branch is dead), and the call then equals the scalar call with d_weight = w bit for bit; a table of ones on a single branch
 * reproduces the demodulator's weighted soft bits.  With one branch the call gives interference-aware soft bits, with several
 * maximal-ratio combining per band: a branch that is jammed in one part of the block still contributes everywhere else.
 * Limit: the frame scale still rests on the power of the phase reference symbol, which includes the interferer: under an interferer
 * of power I beside the signal power S every soft bit shrinks by (S + I) / S.
 * _plan_banded: what dabgpu_diversity_plan refuses, then a table entry that is not 4-byte aligned and a branch with both a table and
 * d_weight.  The host form takes h_band_weight[b] -> [128] floats in host memory (or NULL; NULL array: the scalar form). */
int dabgpu_diversity_plan_banded(const dabgpu_diversity_branch *h_branches, int n_branches, size_t n_frames, const int8_t *d_bits,
                                 size_t bits_frame_stride, int bits_layout, int symbols_per_block, const float *const *h_band_weight,
                                 dabgpu_diversity_geometry *out);
int dabgpu_diversity_combine_frames_banded(dabgpu_ctx *ctx, const dabgpu_diversity_branch *h_branches, int n_branches, size_t n_frames,
                                           int8_t *d_bits, size_t bits_frame_stride, int bits_layout, int symbols_per_block,
                                           float *d_soft_scale, uint32_t *d_live_mask, const float *const *h_band_weight, void *stream);
int dabgpu_diversity_combine_banded_host_sync(dabgpu_ctx *ctx, const float *const *h_dqpsk, const float *h_scale, const float *h_weight,
                                              const int *h_valid, int n_branches, int bits_layout, int8_t *h_bits, float *h_soft_scale,
                                              uint32_t *h_live_mask, const float *const *h_band_weight);
/* the branch weight of a band table on the host: the tree mean above of 128 band weights */
float dabgpu_diversity_band_mean_host(const float band_weight[128]);

/* ------------------------------------------------------------------------------------------------
 * Decision-directed noise profile: "Noise profile" with the frame's own DQPSK products in the NULL symbol's place (mode I; batched, one
 * kernel launch per call, no host state: a call may be captured in a HIP graph; the smoothing state is the caller's array).  The NULL
 * symbol shows what is on the air for 1.3 ms of a frame's 96 ms; an interferer that is silent then (a TDMA neighbour, a gated source)
 * leaves a flat profile and unweighted bands.  The products behind dabgpu_ofdm_sync_demod_frames_branch carry the noise of the 75 data
 * symbols themselves: for a carrier with channel power a = |H|^2 and noise power q per bin of the unnormalised transform,
 * E|d|^2 = (a + q)^2, and while decisions are right the mean of (|re d| + |im d|) / sqrt(2) is a.  The reference has no such code;
 * this section is the definition.  Per frame, from d_dqpsk [n_frames][75][1536] complex float in carrier order c:
 *   1 sums        S2[c] = the sum over the 75 products of fma(re, re, im * im), S1[c] = the sum of |re| + |im|: each a sequential chain
 *                 in symbol order begun at +0, whatever the launch geometry.
 *   2 carriers    A[c] = S1[c] * k1, k1 the float nearest 1 / (75 sqrt(2)); Q[c] = max(sqrt(S2[c] * k75) - A[c], 0), k75 the float
 *                 nearest 1 / 75, the root correctly rounded; a NaN gives Q[c] = 0.  Q is in the units of "Noise profile" step 1
 *                 (white noise of power s2 per sample: E[Q] = 2048 s2).  d_carrier_noise [n_frames][1536] takes Q,
 *                 d_carrier_amplitude [n_frames][1536] takes A (both optional).
 *   3 bands       steps 2 to 5 of "Noise profile" with Q in the place of C: d_exclude, d_profile_in, alpha, d_profile_out (may be
 *                 d_profile_in itself), M, w_b = 1 / max(n_b, M * 2^-20); d_band_weight [n_frames][128], d_mean_noise, d_valid.
 *   skipped       a frame whose record in d_sync (optional) has sync_valid = 0: its products are stale and none is read; or a frame
 *                 whose M is not a normal positive finite number.  Outputs are those of "Noise profile: skipped": 0 to every band
 *                 weight, to d_mean_noise, d_carrier_noise and d_carrier_amplitude, d_valid cleared, d_profile_out = d_profile_in (0
 *                 without one).
 * One frame's band value is far steadier than the NULL's (12 carriers x 75 products: relative deviation about 0.04 against 0.29),
 * and TII carriers do not bias it; the exclusion table remains for carriers known to be bad.  Limits: the estimate under-reads where
 * decisions fail (q^ / q about 0.98 from 12 dB carrier SNR up, 0.8 at 6 dB, 0.5 at 0 dB, 0.3 at -10 dB) but stays monotone, so a jammed
 * band still reads far above its neighbours; amplitude that changes within the frame (fast fading) reads as noise; the frame scale
 * still rests on the power of the phase reference symbol, and under a jammed band A is inflated, so A is no cure for that.
 * Arithmetic: csrc/dd_profile_core.h; the device equals dabgpu_dd_profile_carriers_host followed by dabgpu_noise_profile_bands_host
 * and the tests' host model bit for bit. */
/* What a dabgpu_dd_profile_frames call with these arguments launches; needs no device (no address is dereferenced).
 * DABGPU_ERR_INVALID_ARG, with the reason in dabgpu_last_error, for: a null result; a transmission_mode other than 1; n_frames of 0 or
 * above 2^24; d_dqpsk null or not 16-byte aligned; records, tables or outputs that are not 4-byte aligned, d_carrier_noise or
 * d_carrier_amplitude not 8-byte aligned; alpha outside (0, 1] (NaN included); d_profile_in and d_profile_out that overlap without
 * being equal; no output at all (d_valid and d_profile_out count as outputs). */
int dabgpu_dd_profile_plan(int transmission_mode, const float *d_dqpsk, size_t n_frames, const dabgpu_sync_state *d_sync,
                           const uint32_t *d_exclude, const float *d_profile_in, float alpha, const float *d_profile_out,
                           const float *d_band_weight, const float *d_mean_noise, const float *d_carrier_noise,
                           const float *d_carrier_amplitude, const uint32_t *d_valid, dabgpu_noise_geometry *out);
/* d_dqpsk and d_sync are dabgpu_ofdm_sync_demod_frames_branch's d_dqpsk and records: the call sits behind a branch's demodulation with
 * no copy.  Every output is optional; d_band_weight can be an entry of dabgpu_diversity_combine_frames_banded's h_band_weight as it is. */
int dabgpu_dd_profile_frames(dabgpu_ctx *ctx, const float *d_dqpsk, size_t n_frames, const dabgpu_sync_state *d_sync,
                             const uint32_t *d_exclude, const float *d_profile_in, float alpha, float *d_profile_out,
                             float *d_band_weight, float *d_mean_noise, float *d_carrier_noise, float *d_carrier_amplitude,
                             uint32_t *d_valid, void *stream);
/* One frame from host memory, synchronous, on the context's stream: h_dqpsk [75][1536] complex float.  h_exclude [48] or NULL;
 * h_profile [128] or NULL: the state, read and written in place; h_band_weight [128], h_mean_noise, h_carrier_noise [1536],
 * h_carrier_amplitude [1536] may be NULL.  Returns DABGPU_OK with *h_valid (may be NULL) 1 or 0. */
int dabgpu_dd_profile_host_sync(dabgpu_ctx *ctx, const float *h_dqpsk, const uint32_t *h_exclude, float *h_profile, float alpha,
                                float *h_band_weight, float *h_mean_noise, float *h_carrier_noise, float *h_carrier_amplitude,
                                uint32_t *h_valid);
/* steps 1 and 2 on the host (no device): one frame's products [75][1536] complex float -> carrier_noise [1536] and
 * carrier_amplitude [1536] (either may be NULL).  Followed by dabgpu_noise_profile_bands_host it is the whole definition.
 * 0, or -1 for null products. */
int dabgpu_dd_profile_carriers_host(const float *dqpsk, float *carrier_noise, float *carrier_amplitude);

/* ------------------------------------------------------------------------------------------------
 * Symbol noise profile: one noise figure and one relative weight per DQPSK product row of a frame (mode I; batched, one kernel launch
 * per call, no host state and no smoothing: a call may be captured in a HIP graph).  A wideband burst that lasts an OFDM symbol or
 * longer escapes the other defences: the blanker's neighbourhood rises with it, the NULL profile hears it only on the NULL, and the
 * decision-directed profile averages every carrier over the frame, so all bands rise alike.  Here the sums run over the 1536 carriers
 * of one row.  The reference has no such code; this section is the definition.  Per frame, from d_dqpsk [n_frames][75][1536] complex
 * float in carrier order, per row s = 0 .. 74:
 *   1 sums        S1 = sum of |re| + |im|, SD = sum of (|re| - |im|)^2, S2 = sum of fma(re, re, im * im) over the row's carriers.
 *                 Order: owner t = 0 .. 255 chains the carriers 2 p, 2 p + 1 of p = t, t + 256, t + 512 from +0; owners
 *                 64 w .. 64 w + 63 meet in the wavefront tree of "Noise profile" step 5; the four sums join as (p0 + p1) + (p2 + p3).
 *   2 quadrature  folded into the first quadrant, the component of a product across the decision diagonal has variance a q + q^2 / 2
 *                 (a channel power, q noise power per bin).  P = S1 * r2 (r2 the float nearest 1 / sqrt 2) stands for the sum of a:
 *                 768 q^2 + P q - SD / 2 = 0, qa = max((sqrt(fma(1536, SD, P * P)) - P) * k1536, 0), k1536 the float nearest
 *                 1 / 1536, the root correctly rounded.  Units of "Noise profile" step 1: white noise of power s2 per sample reads
 *                 as 2048 s2.
 *   3 power       qa saturates where decisions fail; R = sqrt(S2 * k1536) = a + q does not.
 *                 q_s = max(qa_s, med(qa) + (R_s - med(R))), med the 38th smallest of the 75 values (rank counting, ties by row index).
 *   4 weights     q_ref = med(q); v_s = 1 where q_s <= q_ref, else min(1, q_ref * (1 / max(q_s, q_ref * 2^-20))), the reciprocal that
 *                 of "Receive diversity".  Relative weights: exactly 1 for at least 38 rows of a valid frame.
 *   bad rows      a row whose S2 * k1536 or discriminant is not finite (a NaN or an infinity among its products, an overflow) has
 *                 qa = R = q = +infinity: it ranks last in every median, v_s = 0, and d_symbol_noise shows the infinity.
 *   skipped       a frame whose record in d_sync (optional) has sync_valid = 0: its products are stale and none is read; or a frame
 *                 whose q_ref is not a normal positive finite number (all zeros; 38 bad rows).  0 to all of d_symbol_weight,
 *                 d_symbol_noise and d_ref_noise, d_valid cleared.
 * Limits: product s mixes symbols s and s + 1, so a burst's edge weighs on one neighbour row; a frame of which more than half is burst
 * has a jammed q_ref and weights near 1; qa / q is about 0.98 from 12 dB carrier SNR up, 0.8 at 6 dB, 0.45 at 0 dB.
 * Arithmetic: csrc/sym_profile_core.h; the device equals dabgpu_sym_profile_rows_host and the tests' host model bit for bit. */
#define DABGPU_SYM_PROFILE_SYMBOLS 75
/* What a dabgpu_sym_profile_frames call with these arguments launches; needs no device (no address is dereferenced).
 * DABGPU_ERR_INVALID_ARG, with the reason in dabgpu_last_error, for: a null result; a transmission_mode other than 1; n_frames of 0 or
 * above 2^24; d_dqpsk null or not 16-byte aligned; records or outputs that are not 4-byte aligned; no output at all (d_valid counts
 * as one). */
int dabgpu_sym_profile_plan(int transmission_mode, const float *d_dqpsk, size_t n_frames, const dabgpu_sync_state *d_sync,
                            const float *d_symbol_weight, const float *d_symbol_noise, const float *d_ref_noise,
                            const uint32_t *d_valid, dabgpu_noise_geometry *out);
/* d_dqpsk and d_sync are dabgpu_ofdm_sync_demod_frames_branch's d_dqpsk and records: the call sits behind a branch's demodulation with
 * no copy.  d_symbol_weight, d_symbol_noise [n_frames][75], d_ref_noise, d_valid [n_frames]: every output is optional;
 * d_symbol_weight can be an entry of dabgpu_diversity_combine_frames_symbols' h_symbol_weight as it is. */
int dabgpu_sym_profile_frames(dabgpu_ctx *ctx, const float *d_dqpsk, size_t n_frames, const dabgpu_sync_state *d_sync,
                              float *d_symbol_weight, float *d_symbol_noise, float *d_ref_noise, uint32_t *d_valid, void *stream);
/* One frame from host memory, synchronous, on the context's stream: h_dqpsk [75][1536] complex float; h_symbol_weight [75],
 * h_symbol_noise [75], h_ref_noise may be NULL.  Returns DABGPU_OK with *h_valid (may be NULL) 1 or 0. */
int dabgpu_sym_profile_host_sync(dabgpu_ctx *ctx, const float *h_dqpsk, float *h_symbol_weight, float *h_symbol_noise,
                                 float *h_ref_noise, uint32_t *h_valid);
/* the whole definition on the host (no device): one frame's products [75][1536] complex float -> symbol_weight [75],
 * symbol_noise [75], ref_noise (each may be NULL).  1 for a valid frame, 0 for a skipped one, -1 for null products. */
int dabgpu_sym_profile_rows_host(const float *dqpsk, float *symbol_weight, float *symbol_noise, float *ref_noise);

/* Symbol-weighted receive diversity: dabgpu_diversity_combine_frames_banded with a symbol noise profile per branch.  h_symbol_weight
 * [n_branches] (host memory, travels by value in the kernel argument): entry b = a device pointer to [n_frames][75] symbol weights of
 * branch b, or NULL.  h_symbol_weight NULL, or every entry NULL: exactly dabgpu_diversity_combine_frames_banded (which itself falls
 * through to the scalar call without band tables).  For a branch with a symbol table, carrier c of product row s enters the sum with
 *     wband * clean(v[s])
 * where wband is what the banded call uses (the band weight of c / 12, or the branch's scalar weight without a band table) and
 * clean(v) is v where v is positive and finite, else 0; the product is rounded once and takes the place of the weight in the sum.
 * Symbol weights enter neither the live rule nor the frame scale: they are relative weights with median 1, and time interleaving
 * spreads a down-weighted row over 16 CIFs.  A table of ones reproduces the banded call bit for bit.
 * Limits: the FIC is not time-interleaved, so FIC symbols under a burst are lost whatever their weight; the frame scale still rests on
 * the power of the phase reference symbol.
 * _plan_symbols: what dabgpu_diversity_plan_banded refuses, then a symbol table entry that is not 4-byte aligned.  The host form takes
 * h_symbol_weight[b] -> [75] floats in host memory (or NULL; NULL array: the banded host form). */
int dabgpu_diversity_plan_symbols(const dabgpu_diversity_branch *h_branches, int n_branches, size_t n_frames, const int8_t *d_bits,
                                  size_t bits_frame_stride, int bits_layout, int symbols_per_block, const float *const *h_band_weight,
                                  const float *const *h_symbol_weight, dabgpu_diversity_geometry *out);
int dabgpu_diversity_combine_frames_symbols(dabgpu_ctx *ctx, const dabgpu_diversity_branch *h_branches, int n_branches, size_t n_frames,
                                            int8_t *d_bits, size_t bits_frame_stride, int bits_layout, int symbols_per_block,
                                            float *d_soft_scale, uint32_t *d_live_mask, const float *const *h_band_weight,
                                            const float *const *h_symbol_weight, void *stream);
int dabgpu_diversity_combine_symbols_host_sync(dabgpu_ctx *ctx, const float *const *h_dqpsk, const float *h_scale, const float *h_weight,
                                               const int *h_valid, int n_branches, int bits_layout, int8_t *h_bits, float *h_soft_scale,
                                               uint32_t *h_live_mask, const float *const *h_band_weight,
                                               const float *const *h_symbol_weight);

/* ------------------------------------------------------------------------------------------------
 * Sampling-clock tracker: the slope of the phase ramp that a sampling-clock error leaves over the carriers of a frame's DQPSK products,
 * and the products with that ramp taken out (mode I; batched, one kernel launch per call, no host state: both calls may be captured
 * in a HIP graph; the tracking state is the caller's array).  A clock error eps moves the sampling instant by eps * 2552 samples from
 * one OFDM symbol to the next.  A product of two neighbouring symbols keeps that as theta * k cycles at carrier number k,
 * theta = eps * 2552 / 2048: 34 degrees at k = +-768 for 100 ppm, against a decision boundary at 45.  The synchroniser's time correction
 * cannot see it (a constant window offset cancels in the product).  d_dqpsk holds X[s] * conj(X[s + 1]), the LATER symbol conjugated,
 * so a positive clock error leaves the ramp -theta * k on it; steps 1 and 7 are written for that, and a positive slope word stands
 * for a positive clock error.  The reference has no such code; this section is the definition.
 * Carrier number: k(c) = c - 768 for c < 768, c - 767 from there on.
 *   slope word    slope_q64: int64, cycles per carrier as Q0.64 in two's complement.  The ramp of carrier k is the exact product
 *                 k * slope_q64 mod 2^64; its angle is the top 24 bits as cycles in [-0.5, 0.5), and (cos, sin) of it those of the channel
 *                 model's oscillator (csrc/channel_core.h: ch_osc_cycles, ch_cos_sin).
 * Estimator, per frame, from d_dqpsk [n_frames][75][1536] complex float in carrier order c:
 *   1 lag         p[s][c] = d[s][c] * conj(d[s][c + L]), L = DABGPU_CLOCK_LAG = 32, for c in 0 .. 735 and 768 .. 1503 (1472 pairs a row:
 *                 both carriers in one half of the block, so their numbers differ by exactly L); with lo = d[s][c], hi = d[s][c + L]:
 *                 re = fma(lo.re, hi.re, lo.im * hi.im), im = fma(lo.im, hi.re, -(lo.re * hi.im)).  Channel, common phase and
 *                 amplitude profile drop out: arg p = theta * L + a multiple of a quarter turn.
 *   2 prior       with s_in = slope_in clamped to +-DABGPU_CLOCK_MAX_SLOPE: p is rotated by the frame's one constant
 *                 (cos, -sin)(L * s_in), in the product order of step 7 -- what de-rotating every product by s_in would do to p.
 *                 s_in = 0: no rotation.
 *   3 fold        into the sector |arg| <= 45 degrees by sign and swap only: |re| >= |im|: p where re >= 0, else -p; otherwise -i p
 *                 where im > 0, else i p.  A pair with a component that is not finite contributes nothing and is counted.
 *   4 sum         A = the sum of the folded products, re and im apart.  Order: a row's 768 float4 positions j (carriers 2 j, 2 j + 1;
 *                 position j pairs with j + 16; positions 368 .. 383 and 752 .. 767 have no partner) are dealt to owners t = 0 .. 255:
 *                 owner t has j = t, t + 256, t + 512.  An owner chains from +0 over the rows s = 0 .. 74, in a row over its positions
 *                 in that order, carrier 2 j before 2 j + 1.  Owners 64 w .. 64 w + 63 meet in the wavefront tree of "Noise profile"
 *                 step 5; the four sums join as (p0 + p1) + (p2 + p3).  Independent of launch geometry.
 *   5 angle       valid: re A a normal positive finite number, |im A| <= re A, and fewer than half of the 110400 pairs dropped.
 *                 t = im A * (1 / re A), the reciprocal that of "Receive diversity"; residual = atan(t) / (2 pi) cycles by a fixed odd
 *                 polynomial of degree 11 in fma Horner form (csrc/clock_core.h, clk_atan_cycles), within 2.5e-6 rad of atan on
 *                 [-1, 1]: 0.01 ppm.
 *   6 update      residual_q64 = rint(residual * 2^59): the residual over L as a slope word.  step = residual_q64 for gain = 1, else
 *                 rint((gain * residual) * 2^59); slope_out = clamp(s_in + step, +-DABGPU_CLOCK_MAX_SLOPE), the slope of 1000 ppm.
 *                 d_slope_out may be d_slope_in itself: the state is then the caller's array, and a zeroed array starts cleanly.
 *   skipped       a frame whose record in d_sync (optional) has sync_valid = 0: its products are stale and none is read; or a frame
 *                 that is not valid by step 5.  slope_out = slope_in as it came, 0 to d_residual and d_corr, d_valid cleared.
 * De-rotator:
 *   7 de-rotate   v[s][c] = d[s][c] * (cos, sin)(k(c) * slope), which takes the ramp -k * slope off: with (c, m) = (cos, sin),
 *                 b0 = m * d.im, b1 = m * d.re, v = (fma(c, d.re, -b0), fma(c, d.im, b1)): the product order of the channel model.
 *                 A frame whose slope word is 0 is a copy bit for bit (in place it is not touched at all); a frame skipped through
 *                 d_sync is neither read nor written.  Out of place or in place (d_dqpsk_out == d_dqpsk_in); any other overlap is
 *                 refused.
 * ppm: slope = ppm * 1e-6 * 2552 / 2048 cycles per carrier.  The sign is that of dabgpu_simulate_transmitter --clock-ppm: a stream
 * made with --clock-ppm X tracks to +X, and dabgpu_resample_step_q62(r, r, -X) ahead of the demodulator would undo it.
 * Limits: the fold errs where noise turns a lag product past 45 degrees, so the estimate under-reads at low SNR and the loop needs more
 * frames to settle; a residual beyond +-45 degrees over L carriers (1/256 cycle per carrier, 3135 ppm) aliases; a ramp that changes
 * within a frame is averaged.
 * Arithmetic: csrc/clock_core.h; the device equals dabgpu_clock_estimate_host / dabgpu_clock_derotate_host and the tests' host model
 * bit for bit. */
#define DABGPU_CLOCK_LAG 32
#define DABGPU_CLOCK_MAX_SLOPE 22986372498099012LL     /* round(1000e-6 * 2552 / 2048 * 2^64) */
/* What a dabgpu_clock_estimate_frames call with these arguments launches; needs no device (no address is dereferenced).
 * DABGPU_ERR_INVALID_ARG, with the reason in dabgpu_last_error, for: a null result; a transmission_mode other than 1; n_frames of 0 or
 * above 2^24; d_dqpsk null or not 16-byte aligned; d_slope_in, d_slope_out or d_residual not 8-byte aligned; d_sync, d_corr or d_valid
 * not 4-byte aligned; gain outside (0, 1] (NaN included); d_slope_in and d_slope_out that overlap without being equal; no output at
 * all. */
int dabgpu_clock_estimate_plan(int transmission_mode, const float *d_dqpsk, size_t n_frames, const dabgpu_sync_state *d_sync,
                               const int64_t *d_slope_in, float gain, const int64_t *d_slope_out, const int64_t *d_residual,
                               const float *d_corr, const uint32_t *d_valid, dabgpu_noise_geometry *out);
/* What a dabgpu_clock_derotate_frames call launches (symbols_per_block = 0) or a _split call with that run length: as above, for a null
 * result; a mode other than 1; n_frames of 0 or above 2^24; products null or not 16-byte aligned; in and out that overlap without being
 * equal; d_slope null or not 8-byte aligned; d_sync not 4-byte aligned; symbols_per_block outside 0 .. 75.  symbols_per_block = 0: the
 * planner chooses as dabgpu_diversity_plan does; the result never depends on it. */
int dabgpu_clock_derotate_plan(int transmission_mode, const float *d_dqpsk_in, const float *d_dqpsk_out, size_t n_frames,
                               const dabgpu_sync_state *d_sync, const int64_t *d_slope, int symbols_per_block,
                               dabgpu_diversity_geometry *out);
/* d_dqpsk and d_sync are dabgpu_ofdm_sync_demod_frames_branch's d_dqpsk and records.  d_slope_in [n_frames] may be NULL: zero.
 * d_slope_out, d_residual [n_frames] int64, d_corr [n_frames][2] (A: re, im), d_valid [n_frames]: every output is optional.  One
 * launch, one workgroup per frame. */
int dabgpu_clock_estimate_frames(dabgpu_ctx *ctx, const float *d_dqpsk, size_t n_frames, const dabgpu_sync_state *d_sync,
                                 const int64_t *d_slope_in, float gain, int64_t *d_slope_out, int64_t *d_residual, float *d_corr,
                                 uint32_t *d_valid, void *stream);
/* One launch.  _split: the same with the rows of a frame dealt to workgroups in runs of symbols_per_block (1 .. 75, 0 = the planner's
 * choice); the bytes written do not depend on it. */
int dabgpu_clock_derotate_frames(dabgpu_ctx *ctx, const float *d_dqpsk_in, float *d_dqpsk_out, size_t n_frames,
                                 const dabgpu_sync_state *d_sync, const int64_t *d_slope, void *stream);
int dabgpu_clock_derotate_frames_split(dabgpu_ctx *ctx, const float *d_dqpsk_in, float *d_dqpsk_out, size_t n_frames,
                                       const dabgpu_sync_state *d_sync, const int64_t *d_slope, int symbols_per_block, void *stream);
/* One frame from host memory through both kernels, synchronous, on the context's stream: h_dqpsk_in [75][1536] complex float; *slope is
 * the state, read and written; the products de-rotated by the NEW slope go to h_dqpsk_out (may be h_dqpsk_in; NULL: estimate only).
 * h_corr [2] may be NULL.  Returns DABGPU_OK with *h_valid (may be NULL) 1 or 0. */
int dabgpu_clock_track_host_sync(dabgpu_ctx *ctx, const float *h_dqpsk_in, float *h_dqpsk_out, int64_t *slope, float gain, float *h_corr,
                                 uint32_t *h_valid);
/* the whole definition on the host (no device).  _estimate_host: one frame's products -> *slope_out, corr [2] (either may be NULL);
 * 1 for a valid frame, 0 for a skipped one, -1 for null products or a gain outside (0, 1].  _derotate_host: step 7 of one frame,
 * dqpsk_out may be dqpsk_in; 0, or -1 for a null argument. */
int dabgpu_clock_estimate_host(const float *dqpsk, int64_t slope_in, float gain, int64_t *slope_out, float *corr);
int dabgpu_clock_derotate_host(const float *dqpsk_in, float *dqpsk_out, int64_t slope_q64);
int64_t dabgpu_clock_slope_q64(double ppm);
double dabgpu_clock_ppm(int64_t slope_q64);

#ifdef __cplusplus
}
#endif
#endif /* DABGPU_H */
