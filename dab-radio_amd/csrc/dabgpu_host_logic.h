// dabgpu_host_logic.h -- the part of libdabgpu.so that never touches the device: constant tables, protection-profile plans, codeword
// validation, the mapping cost model, run-length rules, the planners (decode, demodulation, channel encoder, channel model: what a call will
// launch, decided before any device header enters), capture-format and wav-header parsing, error text.  Plain C++ (no HIP headers):
// compiled into the library by the same Makefile, and on its own with -fsanitize=address,undefined by tests/test_host_sanitizers.py,
// which fuzzes it (tests/cpp/host_logic_fuzz.cpp).
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "dabgpu.h"

#if defined(__HIPCC__)
#define DABGPU_HD __host__ __device__
#else
#define DABGPU_HD
#endif

void dabgpu_set_error(const char* fmt, ...);          // thread-local detail of the last failure (dabgpu_last_error)

struct dabgpu_msc_plan {            // device-side sub-channel plan (one per sub-channel of the multiplex)
    uint32_t start_address;         // CUs
    uint32_t n_steps;               // trellis steps incl. tail
    uint32_t seg_pi[4];
    uint32_t seg_steps[4];
    uint32_t out_offset;            // byte offset of this sub-channel inside one CIF's output record
    uint32_t n_out_bytes;
    uint32_t lane_mapped;           // this call decodes the sub-channel with the lane-per-codeword kernel: viterbi_kernel skips it
};
struct dabgpu_vit_tables {          // constant tables of the Viterbi kernels, built on the host at context creation
    uint16_t pi_tab[25 * 8];        // [PI][group]: kept count | running prefix << 8 (puncture_codes.h:42-67)
    unsigned char prbs[512];        // energy-dispersal bytes, period 511 (additive_scrambler.h:16-35)
};

// geometry of the four transmission modes (src/ofdm/dab_ofdm_params_ref.cpp:11-60)
namespace dabgpu {
struct ModeGeom { int n_sym, period, null_period, n_fft, n_cp, n_carriers, frame_samples, sym_bits, frame_bits; };

DABGPU_HD inline bool mode_geometry(int mode, ModeGeom& g) {
    switch (mode) {
    case 1: g.n_sym = 76; g.period = 2552; g.null_period = 2656; g.n_fft = 2048; g.n_carriers = 1536; break;
    case 2: g.n_sym = 76; g.period = 638; g.null_period = 664; g.n_fft = 512; g.n_carriers = 384; break;
    case 3: g.n_sym = 153; g.period = 319; g.null_period = 345; g.n_fft = 256; g.n_carriers = 192; break;
    case 4: g.n_sym = 76; g.period = 1276; g.null_period = 1328; g.n_fft = 1024; g.n_carriers = 768; break;
    default: return false;
    }
    g.n_cp = g.period - g.n_fft;
    g.frame_samples = g.n_sym * g.period + g.null_period;
    g.sym_bits = 2 * g.n_carriers;
    g.frame_bits = (g.n_sym - 1) * g.sym_bits;
    return true;
}

}  // namespace dabgpu

// ---- sizes of the batch decoders' scratch areas ----
// decisions are stored two steps per row pair; the chain-back reads whole 24-step chunks
DABGPU_HD static inline uint32_t dabgpu_vit_alloc_steps(uint32_t n_steps) { return (n_steps + 6u + 63u) & ~63u; }
#define DABGPU_VIT_SCHED_PREFETCH 6u          // entries past the last step the trellis loops may load (viterbi_lanes.hip, viterbi_octet.hip)
static_assert(((0u + 6u + 63u) & ~63u) >= 0u + DABGPU_VIT_SCHED_PREFETCH && ((58u + 6u + 63u) & ~63u) >= 58u + DABGPU_VIT_SCHED_PREFETCH,
              "dabgpu_vit_alloc_steps must leave room for the schedule prefetch");
// soft bits a codeword consumes (dab_viterbi_decoder.cpp:131-181): 8 + PI per 8 steps, 12 for the tail
DABGPU_HD static inline uint32_t dabgpu_vit_in_bytes(const uint32_t* seg_pi, const uint32_t* seg_steps) {
    uint32_t n = 12;
    for (int k = 0; k < 4; k++) n += (seg_steps[k] >> 3) * (8u + seg_pi[k]);
    return n;
}
// symbol rows: 4 kept soft bits per row, + the row the last step's two-row window reaches into + one the prefetch may touch
DABGPU_HD static inline uint32_t dabgpu_vit_in_rows(uint32_t n_in) { return (n_in + 3u) / 4u + 2u; }

// a codeword's puncturing from "segments + tail": PI only where a segment has steps, n_steps = sum + the 6 tail steps
DABGPU_HD static inline void dabgpu_cw_set_segments(dabgpu_codeword* D, const uint32_t* seg_pi, const uint32_t* seg_steps) {
    D->n_steps = 6;
    for (int k = 0; k < 4; k++) { D->seg_pi[k] = seg_steps[k] ? seg_pi[k] : 0u; D->seg_steps[k] = seg_steps[k]; D->n_steps += seg_steps[k]; }
}
// the FIB group's codeword (fic_decoder.cpp:53-84): PI_16 x 21 blocks, PI_15 x 3 blocks, tail; 3 FIBs of 32 bytes with a CRC each
#define DABGPU_FIC_STEPS 774u
#define DABGPU_FIC_SEG_PI {16u, 15u, 0u, 0u}
#define DABGPU_FIC_SEG_STEPS {32u * 21u, 32u * 3u, 0u, 0u}
#define DABGPU_FIC_OUT_BYTES 96u
#define DABGPU_FIC_CRC_BLOCKS 3u
DABGPU_HD static inline void dabgpu_cw_set_fic(dabgpu_codeword* D) {
    const uint32_t pi[4] = DABGPU_FIC_SEG_PI, steps[4] = DABGPU_FIC_SEG_STEPS;
    dabgpu_cw_set_segments(D, pi, steps);
    D->n_crc_blocks = DABGPU_FIC_CRC_BLOCKS;
}

// symbols_per_block = 0 of the mode I demodulator
int dabgpu_host_small_batch_spb(size_t n_frames);
int dabgpu_host_spb_bucket(size_t n_frames);
int dabgpu_host_spb_variant(int src, int bits_layout, bool tail);
// argument check of one dabgpu_codeword (index i only for the message)
int dabgpu_host_validate_codeword(const dabgpu_codeword& d, size_t i);
// DABGPU_VIT_MAP_AUTO: cost model of the three decoder mappings (n_simd = SIMDs of the device); forced_mapping != AUTO is returned as is
int dabgpu_host_choose_mapping(int forced_mapping, double n_simd, size_t n_cw, size_t n_groups, double sum_cw_steps, double sum_group_steps,
                               double max_steps, bool staged_gather);
// the same for the MSC of n_ens ensembles sharing a multiplex (steps[j] = trellis steps of sub-channel j); model_us[3] (may be null) = the
// modelled WAVE / LANE / OCTET times
int dabgpu_host_choose_msc_mapping(int forced_mapping, double n_simd, size_t n_ens, const uint32_t* steps, int n_sub, double* model_us);
// the device-side plans of a multiplex's sub-channels (msc_decoder.cpp:77-154): DABGPU_OK, or DABGPU_ERR_INVALID_ARG for an invalid
// profile / a sub-channel outside the 864 capacity units / more than 64 sub-channels
int dabgpu_host_build_msc_plans(const dabgpu_subchannel* subs, int n_sub, std::vector<dabgpu_msc_plan>& plans, uint32_t* cif_out_bytes,
                                uint32_t* max_steps, uint32_t* max_out_bytes);
void dabgpu_host_fill_vit_tables(dabgpu_vit_tables* T);
// The lane and octet gathers keep a CIF ring's offsets in 32 bits (viterbi_lanes.hip, vit_prep_kernel): is the largest one they can form
// -- last frame, last CIF of a frame, last time-interleaver class of a class-order row -- below 2^32?  The one rule behind the decode
// planner (n_slots = 4 history frames of 230400 soft bits) and behind the generic batch's ring-form code words.
bool dabgpu_host_ring_fits_lanes(uint64_t n_slots, uint64_t cifs_per_frame, uint64_t frame_stride, uint64_t cif_stride);

// ---- decode planner: what a batch decode call will launch, from its arguments alone (no device address enters) ----
// what the planner may not decide for itself: the device, the environment (read once per entry-point call), the context's setting
struct dabgpu_decode_limits {
    double n_simd;              // SIMDs of the device (cost model)
    size_t max_dec_rows;        // decision rows one lane / octet launch may hold (DABGPU_VIT_SCRATCH_MB at 768 bytes per row), >= 1
    int hybrid_k;               // DABGPU_VIT_HYBRID_K (tests): that many longest sub-channels stay with viterbi_kernel; -1: not given
    int forced_mapping;         // DABGPU_VIT_MAP_* of the context (dabgpu_viterbi_set_mapping)
};
// one puncturing schedule for a whole batch (FIC, uniform codeword batches): groups of 64 consecutive codewords, in bounded slices
struct dabgpu_uniform_plan {
    int mapping;                // DABGPU_VIT_MAP_WAVE / _LANE / _OCTET
    uint32_t dec_rows, in_rows; // decision / symbol rows of one group
    size_t slice_groups;        // groups per launch
};
dabgpu_uniform_plan dabgpu_host_plan_uniform(size_t n_cw, uint32_t n_steps, const uint32_t* seg_pi, const uint32_t* seg_steps, bool staged_gather,
                                             const dabgpu_decode_limits& lim);
inline dabgpu_uniform_plan dabgpu_host_plan_fic(size_t n_cw, bool staged_gather, const dabgpu_decode_limits& lim) {
    const uint32_t pi[4] = DABGPU_FIC_SEG_PI, steps[4] = DABGPU_FIC_SEG_STEPS;
    return dabgpu_host_plan_uniform(n_cw, DABGPU_FIC_STEPS, pi, steps, staged_gather, lim);
}

// lane-per-codeword decoder (viterbi_lanes.hip): a GROUP = up to 64 codewords with one puncturing schedule.
// Symbol area of a group: the codewords' KEPT soft bits only, transposed -- row j, lane L = input bytes 4 j .. 4 j + 3 of lane L's
// codeword (after the time de-interleaver, -128 clamped to -127).  The trellis kernel de-punctures with wave-uniform selectors.
struct dabgpu_vit_group {
    uint32_t first, stride, count;  // lane L decodes descs[first + L * stride], L < count
    uint32_t n_steps;               // trellis steps incl. tail
    uint32_t alloc_steps;           // rows of the group's decision area (dabgpu_vit_alloc_steps)
    uint32_t seg_pi[4];
    uint32_t seg_steps[4];
    uint32_t in_rows;               // rows of the group's symbol area (dabgpu_vit_in_rows)
    uint64_t sched_off;             // entries into the schedule tables: (symbol row, v_perm_b32 selector) per trellis step
    uint64_t sym_off;               // dwords into the symbol scratch   [in_rows][64]
    uint64_t dec_off;               // dwords into the decision scratch [alloc_steps][64][2]
    int64_t res_delta;              // bytes added to &results[first + L * stride]: groups of ONE launch may report into different arrays
                                    // (the FIB groups of a frame decoded inside the MSC launch, dabgpu_decode_frames_layout)
};
// groups appended to another launch's: descriptor index, schedule entries, symbol / decision dwords and result bytes they start at
struct dabgpu_vit_group_base { uint32_t first; uint64_t sched_off, sym_off, dec_off; int64_t res_delta; };

// MSC (+ FIC of the newest frame) of n_ens ensembles sharing a multiplex.  Sub-channels in descending trellis length: the first k_wave go
// to viterbi_kernel (one wavefront per codeword), the other n_lane to the lane / octet kernels, group (li, gq) = lane-mapped sub-channel
// li of ensemble-CIFs 64 gq .. 64 gq + 63, ensembles sliced so that a launch stays inside max_dec_rows.
enum dabgpu_fic_place {
    DABGPU_FIC_NONE,            // not asked for
    DABGPU_FIC_OWN_LAUNCH,      // decoded first, by the FIC entry point's own path
    DABGPU_FIC_IN_LANES,        // every sub-channel lane-mapped and the call one slice: the FIB groups are further groups of the lane launch
    DABGPU_FIC_IN_WAVE,         // every sub-channel in viterbi_kernel and the FIC alone would be too: codewords n_cw .. of that launch
};
struct dabgpu_decode_plan {
    std::vector<dabgpu_msc_plan> subs;      // as staged (table 0), lane_mapped set
    std::vector<uint64_t> lane_subs;        // as staged (table 1): [n_lane] x (sub-channel, decision rows before it, symbol rows before it)
    int mapping;                            // the pure choice (forced, or the cost model's) and what the model expects of WAVE / LANE / OCTET
    double model_us[3];
    int n_sub, k_wave, n_lane, octet;
    dabgpu_fic_place fic;
    size_t n_ens, n_cw, n_fic_cw;           // codewords of the sub-channels / FIB groups (sizes saturate at SIZE_MAX instead of wrapping)
    uint32_t cif_out_bytes;
    uint32_t max_steps, max_out_bytes;      // of the viterbi_kernel launch (the FIB group's included under DABGPU_FIC_IN_WAVE)
    uint32_t lane_max_steps, lane_max_in_rows, sched_stride;
    uint32_t fic_dec_rows, fic_in_rows;     // rows of one group of FIB codewords
    size_t dec_rows_per_gq, sym_rows_per_gq, ens_per_slice;
    size_t descs_bytes, plans_bytes, lane_subs_bytes, sched_bytes;      // SCR_CW_DESCS, SCR_MSC_PLANS, SCR_LANE_SUBS, SCR_VIT_SCHED
};
// DABGPU_OK, or dabgpu_host_build_msc_plans's status
int dabgpu_host_plan_decode(const dabgpu_subchannel* subs, int n_sub, size_t n_ens, int hist_frames, bool want_fic, const dabgpu_decode_limits& lim,
                            dabgpu_decode_plan* out);
// the lane launch over ensembles e0 .. e0 + ne - 1 (e0 a multiple of ens_per_slice)
struct dabgpu_decode_slice {
    size_t ne, cw0;                         // ensembles; first codeword (descriptor and result index)
    uint32_t gps;                           // groups per lane-mapped sub-channel
    size_t n_groups, n_fic_groups;          // MSC groups, appended FIB groups (DABGPU_FIC_IN_LANES)
    size_t sym_rows, dec_rows;              // SCR_VIT_SYM / SCR_VIT_DEC, rows of 64 / 128 dwords, appended groups included
    size_t groups_bytes;                    // SCR_VIT_GROUPS
    dabgpu_vit_group_base fic_base;         // where the appended groups start behind the MSC's (res_delta: the executor's, two device addresses)
};
dabgpu_decode_slice dabgpu_host_decode_slice(const dabgpu_decode_plan& p, size_t e0);

// ---- demodulation planner: which kernel one demodulator launch runs and over what grid (dabgpu_launch_demod launches from it) ----
// Four kernel families: the register-resident mode I kernel (ofdm_demod.hip), the size-generic kernel (ofdm_modes.hip), one wavefront per
// run of symbols for modes II-IV, and two symbols per wavefront for mode III (ofdm_wave512.hip).  Each keeps a table of its kernels,
// indexed by `variant`:
//   mode I:        ((src * 2 + bank) * 3 + layout), layout 0 = soft bits, 1 = + display views, 2 = soft bits in class order;
//                  weighted soft bits (DABGPU_SOFT_CSI) follow as 24 + src * 3 + layout for aligned frames, and behind those as
//                  36 + src * 2 + (class order) for a bank round that states bank_soft (a bank round has no display views),
//                  and last 44 + src for a bank round that states bank_products: the weighted soft bits plus the frame's DQPSK products
//                  at the descriptor's bits slot (dabgpu_stream_bank_set_products)
//   other families: 0 without descriptors (complex float only), 1 + src with them
enum dabgpu_demod_family { DABGPU_DEMOD_MODE1, DABGPU_DEMOD_GENERIC, DABGPU_DEMOD_WAVE, DABGPU_DEMOD_WAVE3 };
enum dabgpu_demod_tail { DABGPU_DEMOD_TAIL_NONE, DABGPU_DEMOD_TAIL_FUSED, DABGPU_DEMOD_TAIL_LAUNCH };
constexpr int DABGPU_DEMOD_MODE1_NORMALISED_VARIANTS = 4 * 2 * 3, DABGPU_DEMOD_MODE1_BANK_SOFT_FIRST = DABGPU_DEMOD_MODE1_NORMALISED_VARIANTS + 4 * 3,
              DABGPU_DEMOD_MODE1_VARIANTS = DABGPU_DEMOD_MODE1_BANK_SOFT_FIRST + 4 * 2;
// (DABGPU_DEMOD_MODE1_VARIANTS keeps its value, 44: tests/cpp/bank_soft_plan_driver.cpp pins it as the end of the bank_soft variants.  The four
// variants of bank_products follow it, and the kernel table has DABGPU_DEMOD_MODE1_KERNELS entries)
constexpr int DABGPU_DEMOD_MODE1_BANK_PRODUCTS_FIRST = DABGPU_DEMOD_MODE1_VARIANTS, DABGPU_DEMOD_MODE1_KERNELS = DABGPU_DEMOD_MODE1_BANK_PRODUCTS_FIRST + 4;
constexpr int DABGPU_DEMOD_LOADER_VARIANTS = 1 + 4;
// the facts of a call that are not addresses.  The views, class order, sync records, frame stride and phase outputs are the mode I kernel's:
// the other families have none of them (the FFT view apart, which only the size-generic kernel writes) and do not look at these facts.
struct dabgpu_demod_facts {
    int src = 0;                            // loader: 0 complex float, 1 u8, 2 s8, 3 s16 (dabgpu_fused_loader)
    bool desc = false;                      // bank round: frame descriptors
    bool fft = false, dqpsk = false;        // display views
    bool sync = false, frame_stride = false;
    bool total_phase = false, fine_freq = false;
    bool classed = false;
    int symbols_per_block = 0, n_frames = 0;
    bool generic_mode1 = false;             // mode I runs on the size-generic kernel too (dabgpu_ofdm_demod_frames_mode: the tests cross-check the two)
    bool switch_generic = false;            // DABGPU_MODE_GENERIC: modes II-IV stay on the size-generic kernel
    bool switch_mode3_single = false;       // DABGPU_MODE3_SINGLE: mode III, one symbol per wavefront
    int soft_policy = DABGPU_SOFT_NORMALISED;   // DABGPU_SOFT_CSI: the mode I kernel without descriptors only
    float soft_level = 64.0f;               // [1, 127], looked at under DABGPU_SOFT_CSI
    bool bank_soft = false;                 // the bank round asks for the weighted policy: needs desc and DABGPU_SOFT_CSI, mode I, no display views
    bool bank_products = false;             // the bank round also stores the frames' DQPSK products by bits slot: needs bank_soft; no class order, no display views
};
struct dabgpu_demod_plan {
    int status;                             // DABGPU_OK, or DABGPU_ERR_INVALID_ARG (reason in dabgpu_last_error): nothing else is set then
    dabgpu_demod_family family;
    int variant;
    int symbols_per_block, chunks;          // run length as resolved, runs per frame
    uint32_t grid, threads;
    uint32_t lds_bytes;                     // dynamic LDS; 0 for mode I: its kernel's own constant
    bool raise_lds_limit;                   // more than 48 KB: the kernel's attribute is set first (the size-generic kernel in mode I only)
    dabgpu_demod_tail tail;
    int fine_stride;                        // floats between the fine-frequency words of two frames
};
dabgpu_demod_plan dabgpu_host_plan_demod(int mode, const dabgpu_demod_facts& f);
// a dabgpu_soft_cfg as an entry point receives it (`who` names it in the message): a policy that exists, a level in [1, 127]
int dabgpu_host_check_soft_cfg(const char* who, const dabgpu_soft_cfg* cfg);

// ---- receive diversity planner (diversity.hip launches from it; include/dabgpu.h, dabgpu_diversity_plan) ----
// the facts of a call that are not addresses: DABGPU_OK and the geometry, or DABGPU_ERR_INVALID_ARG with the reason.  symbols_per_block = 0
// resolves as the demodulator's small-batch rule does (dabgpu_host_small_batch_spb): the combiner has no halo symbol, a shorter run costs
// it one more set-up (scale, six de-interleave positions) and nothing else.
#define DABGPU_DIVERSITY_THREADS 256u
#define DABGPU_DIVERSITY_LDS_BYTES (2u * 3072u)        // two symbol rows of soft bits: scatter into one while the other is stored
int dabgpu_host_plan_diversity(int n_branches, size_t n_frames, int bits_layout, int symbols_per_block, size_t bits_frame_stride,
                               dabgpu_diversity_geometry* out);
// the planner of every diversity call (dabgpu_diversity_plan_banded and _plan_symbols are this one): dabgpu_diversity_plan's checks, then
// the band tables', then the symbol tables' (either array may be null), each refusal under its own planner's name.  *mode (may be null)
// receives the call's effective mode, diversity.hip's dv_mode: 2 where a symbol entry is given, else 1 where a band entry is, else 0
int dabgpu_host_plan_diversity_mode(const dabgpu_diversity_branch* h_branches, int n_branches, size_t n_frames, const int8_t* d_bits,
                                    size_t bits_frame_stride, int bits_layout, int symbols_per_block, const float* const* h_band_weight,
                                    const float* const* h_symbol_weight, dabgpu_diversity_geometry* out, int* mode);

// ---- the per-frame estimators: their planners (dabgpu_host_logic.cpp) are lists of plan_prelude.h's checks with each one's own rules ----
// ---- noise estimator (noise.hip launches from dabgpu_noise_plan; include/dabgpu.h, "Noise estimate") ----
// one 256-thread workgroup per frame; static LDS: the transform's patches, 2048 bin powers, 192 group energies, 24 floor shares, the four
// wave sums of the frame power and the decision word
#define DABGPU_NOISE_THREADS 256u
#define DABGPU_NOISE_LDS_BYTES (18432u + 8192u + 768u + 96u + 16u + 4u)

// ---- noise profile (noise_profile.hip launches from dabgpu_noise_profile_plan; include/dabgpu.h, "Noise profile") ----
// one 256-thread workgroup per frame; static LDS: the transform's patches, 2048 bin powers, the two wave sums of the mean
#define DABGPU_NOISE_PROFILE_THREADS 256u
#define DABGPU_NOISE_PROFILE_LDS_BYTES (18432u + 8192u + 8u)
// the banded combiner's instantiation adds the two wave sums of every branch's mean weight to the combiner's LDS
#define DABGPU_DIVERSITY_BANDED_LDS_BYTES (DABGPU_DIVERSITY_LDS_BYTES + 8u * 2u * 4u)

// ---- decision-directed noise profile (dd_profile.hip launches from dabgpu_dd_profile_plan; include/dabgpu.h) ----
// one 256-thread workgroup per frame; static LDS: 1536 carrier values, the two wave sums of the mean
#define DABGPU_DD_PROFILE_THREADS 256u
#define DABGPU_DD_PROFILE_LDS_BYTES (6144u + 8u)

// ---- symbol noise profile (sym_profile.hip launches from dabgpu_sym_profile_plan; include/dabgpu.h) ----
// one 256-thread workgroup per frame; static LDS: 75 x 4 x 3 wave sums, three rows of 75 figures, three medians
#define DABGPU_SYM_PROFILE_THREADS 256u
#define DABGPU_SYM_PROFILE_LDS_BYTES (3600u + 900u + 12u)

// ---- sampling-clock tracker (clock.hip launches from dabgpu_clock_estimate_plan / _derotate_plan; include/dabgpu.h) ----
// estimator: one 256-thread workgroup per frame; static LDS: 4 x 2 wave sums, 4 counts.  De-rotator: a workgroup per run of rows (the
// combiner's symbols_per_block rule); static LDS: the frame's 1536 rotations
#define DABGPU_CLOCK_THREADS 256u
#define DABGPU_CLOCK_ESTIMATE_LDS_BYTES (32u + 16u)
#define DABGPU_CLOCK_DEROTATE_LDS_BYTES (1536u * 8u)

// ---- channel encoder planner (dab_encode.hip launches from it; include/dabgpu.h, dabgpu_tx_encode_plan) ----
#define DABGPU_TX_TAIL_KEEP_MASK 0x00333333u        // PI_X: 2 of the 4 mother bits of each of the six tail steps
struct dabgpu_tx_plan {
    std::vector<dabgpu_tx_sub_plan> subs;           // n_sub sub-channels in list order, then the FIB group
    std::vector<dabgpu_tx_sched_entry> sched;       // kept-bit schedules, one per distinct (PI, L) list
    std::vector<uint32_t> gaps;                     // (start, length) in capacity units of the ranges no sub-channel occupies, ascending
    uint32_t cif_in_bytes = 0;
    uint32_t ring_slot_dwords = 0;                  // one slot of an ensemble's time-interleaver ring (16 slots per ensemble)
    uint32_t max_length = 0;                        // capacity units of the largest sub-channel
};
// DABGPU_OK, or DABGPU_ERR_INVALID_ARG with the reason in dabgpu_last_error
int dabgpu_host_tx_plan(const dabgpu_subchannel* subs, int n_sub, dabgpu_tx_plan* out);

// ---- channel BER planner (channel_ber.hip launches from it; include/dabgpu.h, dabgpu_ber_plan) ----
#define DABGPU_BER_WAVES 4u                         // wavefronts (code words) per workgroup
struct dabgpu_ber_launch {
    dabgpu_tx_plan tx;                              // the encoder's plan of the multiplex: sub-channels, FIB group, schedules
    dabgpu_ber_geometry geo;
};
// DABGPU_OK, or DABGPU_ERR_INVALID_ARG with the reason in dabgpu_last_error (the order of the checks: include/dabgpu.h)
int dabgpu_host_ber_plan(const dabgpu_subchannel* subs, int n_sub, size_t n_ens, int hist_frames, size_t ens_stride, size_t out_ens_stride,
                         int bits_layout, dabgpu_ber_launch* out);
// LDS dwords one wavefront holds a code word of `length` capacity units in (whole blocks of 512 bits)
DABGPU_HD static inline uint32_t dabgpu_ber_cw_dwords(uint32_t length) { return 16u * ((length + 7u) / 8u); }

// ---- channel model planner (channel.hip launches from it; include/dabgpu.h, dabgpu_channel_plan) ----
// DABGPU_OK and the geometry, or DABGPU_ERR_INVALID_ARG with the reason (stream index, field) in dabgpu_last_error
int dabgpu_host_channel_plan(const dabgpu_channel_stream* params, size_t n_streams, dabgpu_channel_geometry* out);
// dabgpu_channel_bank_set_params: the launch geometry (kernel variant, LDS size) is the one of the bank's creation -- a captured call has it
// baked in -- so new parameters must fit it: DABGPU_OK, or DABGPU_ERR_INVALID_ARG with the reason
int dabgpu_host_channel_fits(const dabgpu_channel_geometry& created, const dabgpu_channel_geometry& wanted);
// the arguments of a dabgpu_channel_bank_apply call (no device address is dereferenced): `who` names the entry point in the message;
// *out_stride_bytes = 0 is replaced by the default.  device_pointers = false (the host form): no alignment rule, rows of any length >= n_out
// samples, the default stride is the row itself
int dabgpu_host_channel_check_apply(const char* who, size_t n_streams, const void* in, size_t in_stride_samples, size_t n_in, size_t n_out,
                                    const void* out, int out_format, size_t* out_stride_bytes, float u8_scale, bool device_pointers = true);
// the fading tables of a bank (dabgpu_channel_bank_create_fading / _set_fading) against its parameters: kinds below n_taps STATIC or FADING,
// the amplitudes of fading taps finite; `who` names the entry point
int dabgpu_host_channel_fading_check(const char* who, const dabgpu_channel_stream* params, const dabgpu_channel_fading_stream* tables, size_t n_streams);
// the geometry of a fading bank from the plain one: always staged, the tile's grid gains behind the staged input
dabgpu_channel_geometry dabgpu_host_channel_fading_geometry(dabgpu_channel_geometry plain);

// ---- interferer planner (interferer.hip launches from it; include/dabgpu.h, dabgpu_interferer_plan) ----
// DABGPU_OK and the geometry, or DABGPU_ERR_INVALID_ARG with the reason (stream, source, field); `who` names the entry point
int dabgpu_host_interferer_plan(const char* who, const dabgpu_interferer_stream* params, size_t n_streams, const dabgpu_interferer_shape* shapes,
                                int n_shapes, dabgpu_interferer_geometry* out);
// dabgpu_interferer_bank_set_params: new parameters must fit the LDS slots of the bank's creation (a captured call has them baked in)
int dabgpu_host_interferer_fits(const dabgpu_interferer_geometry& created, const dabgpu_interferer_geometry& wanted);
// the arguments of a dabgpu_interferer_bank_apply call, as dabgpu_host_channel_check_apply; in may be NULL, in == out is in place
int dabgpu_host_interferer_check_apply(const char* who, size_t n_streams, const void* in, size_t in_stride_samples, size_t n_out, const void* out,
                                       int out_format, size_t* out_stride_bytes, float u8_scale, bool device_pointers = true);

// ---- IQ balance planner (iqbal.hip launches from it; include/dabgpu.h, dabgpu_iqbal_plan) ----
// who = the entry point's name for the refusal text
int dabgpu_host_iqbal_plan(const char* who, const dabgpu_iqbal_stream* params, size_t n_streams, size_t max_samples_per_call,
                           dabgpu_iqbal_geometry* out);
// the arguments of a dabgpu_iqbal_bank_apply call (no device address is dereferenced); *out_stride_bytes: 0 is replaced by the default
int dabgpu_host_iqbal_check_apply(const char* who, size_t n_streams, const dabgpu_iqbal_geometry& geom, const void* in, size_t in_stride_samples,
                                  size_t n, const void* out, int out_format, size_t* out_stride_bytes, float u8_scale, uint32_t flags,
                                  bool device_pointers = true);

// ---- impulse blanker planner (blanker.hip launches from it; include/dabgpu.h, dabgpu_blanker_plan) ----
// DABGPU_OK and the geometry, or DABGPU_ERR_INVALID_ARG with the reason (stream, field); `who` names the entry point
int dabgpu_host_blanker_plan(const char* who, const dabgpu_blanker_stream* params, size_t n_streams, dabgpu_blanker_geometry* out);
// dabgpu_blanker_bank_set_params: new parameters must fit the reach of the bank's creation (a captured call has its LDS size baked in)
int dabgpu_host_blanker_fits(const dabgpu_blanker_geometry& created, const dabgpu_blanker_geometry& wanted);
// the arguments of a dabgpu_blanker_bank_apply call (no device address is dereferenced); *out_stride_bytes and *mask_stride_words: 0 is
// replaced by the default
int dabgpu_host_blanker_check_apply(const char* who, size_t n_streams, const void* in, size_t in_stride_samples, size_t n_in, size_t n_out,
                                    const void* out, size_t* out_stride_bytes, const void* mask, size_t* mask_stride_words, bool device_pointers = true);

// ---- resampler planner (resample.hip launches from it; include/dabgpu.h, dabgpu_resample_plan) ----
// DABGPU_OK and the geometry, or DABGPU_ERR_INVALID_ARG with the reason (stream index, field); `who` names the entry point.
// max_step_q62: the largest step the bank's design serves (dabgpu_host_resample_max_step_q62 of its max_step)
int dabgpu_host_resample_plan(const char* who, const dabgpu_resample_stream* params, size_t n_streams, uint64_t max_step_q62,
                              dabgpu_resample_geometry* out);
uint64_t dabgpu_host_resample_max_step_q62(double max_step);       // max_step rounded UP to Q2.62, within [2^61, 2^63]; 0: not a valid max_step
// dabgpu_resample_bank_set_params: new parameters must fit the window and the table rows of the bank's creation
int dabgpu_host_resample_fits(const dabgpu_resample_geometry& created, const dabgpu_resample_geometry& wanted);

// ---- channeliser planner (channelise.hip launches from it; include/dabgpu.h, dabgpu_channeliser_plan) ----
// DABGPU_OK and the geometry, or DABGPU_ERR_INVALID_ARG with the reason (channel index, field); `who` names the entry point.
// first (NULL, or n_streams + 1 words): first[s] .. first[s + 1] are the channels of stream s in the sorted list
int dabgpu_host_channeliser_plan(const char* who, const dabgpu_channeliser_channel* channels, size_t n_channels, size_t n_streams, int64_t start,
                                 int decim, dabgpu_channeliser_geometry* out, uint32_t* first);
// the workgroups of a call: DABGPU_OK and *tiles, or DABGPU_ERR_INVALID_ARG when tiles x rows does not fit one grid
int dabgpu_host_channeliser_tiles(const char* who, size_t n_out, uint32_t tile, size_t rows, uint32_t* tiles);

// ---- DAB+ super-frame encoder (dabplus_tx.hip; include/dabgpu.h, dabgpu_dabplus_superframe_layout) ----
// Where the access units of a super frame start (ETSI TS 102 563 5.2, as AAC_Frame_Processor reads it back, aac_frame_processor.cpp:266-283),
// one body for the host entry point and the kernel.  au_len: the first num_aus entries are read; start[0 .. num_aus] are written, the rest
// of start[7] zeroed.  0, or DABGPU_DABPLUS_TX_BAD_FRAME_SIZE / _BAD_FILL / _BAD_START (then start[] holds no layout).
DABGPU_HD inline int dabgpu_dabplus_layout(uint32_t frame_bytes, uint32_t descriptor, const uint16_t* au_len, uint32_t* start, int* num_aus,
                                           uint32_t* n_rs) {
    *num_aus = 0; *n_rs = 0;
    for (int i = 0; i < 7; i++) start[i] = 0;
    if (frame_bytes < 24u || frame_bytes > 1536u || frame_bytes % 24u) return DABGPU_DABPLUS_TX_BAD_FRAME_SIZE;
    const int dac_rate = (descriptor >> 6) & 1, sbr = (descriptor >> 5) & 1;
    const int na = dac_rate ? (sbr ? 3 : 6) : (sbr ? 2 : 4);                     // :275-279
    *num_aus = na; *n_rs = frame_bytes / 24u;
    uint32_t s = 3u + (12u * (uint32_t)(na - 1) + 7u) / 8u;
    start[0] = s;
    for (int i = 0; i < 6; i++) if (i < na) { s += (uint32_t)au_len[i] + 2u; start[i + 1] = s; }      // at most 6 x 65537 + 11
    if (s != 110u * *n_rs) return DABGPU_DABPLUS_TX_BAD_FILL;
    for (int i = 1; i < 6; i++) if (i < na && start[i] > 4095u) return DABGPU_DABPLUS_TX_BAD_START;
    return 0;
}
