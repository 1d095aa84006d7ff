// dabgpu_host_logic.cpp -- see dabgpu_host_logic.h.  No device code and no HIP call in this file.
#include "dabgpu_host_logic.h"
#include "packet_fec_core.h"
#include "softbit_csi_core.h"
#include "diversity_core.h"
#include "noise_core.h"
#include "noise_profile_core.h"
#include "dd_profile_core.h"
#include "sym_profile_core.h"
#include "clock_core.h"
#include "plan_prelude.h"

#include <math.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <string>

static thread_local std::string g_last_error;

void dabgpu_set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    g_last_error = buf;
}


extern "C" {

const char* dabgpu_strerror(int status) {
    switch (status) {
    case DABGPU_OK: return "ok";
    case DABGPU_ERR_NO_DEVICE: return "no usable gfx950 device (this library has no CPU fallback)";
    case DABGPU_ERR_INVALID_ARG: return "invalid argument";
    case DABGPU_ERR_HIP: return "HIP runtime error";
    case DABGPU_ERR_NOT_READY: return "not ready";
    case DABGPU_ERR_UNSUPPORTED: return "unsupported transmission mode";
    default: return "unknown status";
    }
}
const char* dabgpu_last_error(void) { return g_last_error.c_str(); }
int dabgpu_abi_version(void) { return DABGPU_ABI_VERSION; }

// ---- built-in tables ----
// ETSI EN 300 401 14.3.2 tables 23/24 (mode I) and the mode II-IV tables of docs/DAB_implementation_in_SDR_detailed.pdf
// appendix B, as (row of the h table, offset n) per block of 32 carriers, lowest carrier first
// (replaces get_DAB_PRS_reference, src/ofdm/dab_prs_ref.cpp:25-195)
static const signed char PRS_ROW_I[4][48] = {
    { 0,1,2,3, 0,1,2,3, 0,1,2,3, 0,1,2,3, 0,1,2,3, 0,1,2,3,  0,3,2,1, 0,3,2,1, 0,3,2,1, 0,3,2,1, 0,3,2,1, 0,3,2,1 },
    { 0,1,2,3,0,1,  2,1,0,3,2,1 },
    { 0,1,2,  3,2,1 },
    { 0,1,2,3, 0,1,2,3, 0,1,2,3,  0,3,2,1, 0,3,2,1, 0,3,2,1 },
};
static const signed char PRS_ROW_N[4][48] = {
    { 1,2,0,1, 3,2,2,3, 2,1,2,3, 1,2,3,3, 2,2,2,1, 1,3,1,2,  3,1,1,1, 2,2,1,0, 2,2,3,3, 0,2,1,3, 3,3,3,0, 3,0,1,1 },
    { 2,3,2,2,1,2,  0,2,2,1,0,3 },
    { 2,3,0,  2,2,2 },
    { 0,1,1,2, 2,2,0,3, 3,1,3,2,  0,1,0,2, 0,1,2,2, 2,1,3,0 },
};
static const signed char PRS_H_TABLE[4][32] = {
    {0,2,0,0,0,0,1,1,2,0,0,0,2,2,1,1,0,2,0,0,0,0,1,1,2,0,0,0,2,2,1,1},
    {0,3,2,3,0,1,3,0,2,1,2,3,2,3,3,0,0,3,2,3,0,1,3,0,2,1,2,3,2,3,3,0},
    {0,0,0,2,0,2,1,3,2,2,0,2,2,0,1,3,0,0,0,2,0,2,1,3,2,2,0,2,2,0,1,3},
    {0,1,2,1,0,3,3,2,2,3,2,1,2,1,3,2,0,1,2,1,0,3,3,2,2,3,2,1,2,1,3,2},
};

int dabgpu_get_prs_fft_ref(int mode, float* out) {
    if (!out) return DABGPU_ERR_INVALID_ARG;
    int geom[9];
    if (dabgpu_get_ofdm_params(mode, geom)) return DABGPU_ERR_INVALID_ARG;
    const int N = geom[3], nb = geom[5], rows = nb / 32, half = rows / 2;
    memset(out, 0, sizeof(float) * 2 * (size_t)N);
    for (int row = 0; row < rows; row++) {
        const int k_min = (row < half) ? (-nb / 2 + 32 * row) : (1 + 32 * (row - half));
        for (int j = 0; j < 32; j++) {
            const int k = k_min + j;
            const int h = PRS_H_TABLE[(int)PRS_ROW_I[mode - 1][row]][j];
            const float phi = (float)M_PI / 2.0f * (float)(h + PRS_ROW_N[mode - 1][row]);
            const int bin = (k < 0) ? (N + k) : k;
            out[2 * bin] = cosf(phi);
            out[2 * bin + 1] = sinf(phi);
        }
    }
    return DABGPU_OK;
}

// ETSI EN 300 401 14.6.1 (replaces get_DAB_mapper_ref, src/ofdm/dab_mapper_ref.cpp:10-51)
int dabgpu_get_carrier_mapper(int mode, int* out) {
    if (!out) return DABGPU_ERR_INVALID_ARG;
    int geom[9];
    if (dabgpu_get_ofdm_params(mode, geom)) return DABGPU_ERR_INVALID_ARG;
    const int N = geom[3], nb = geom[5], dc = N / 2, lo = dc - nb / 2, hi = dc + nb / 2;
    int v = 0, n = 0;
    for (int i = 0; i < N; i++) {
        if (i > 0) v = (13 * v + N / 4 - 1) % N;
        if (v < lo || v > hi || v == dc) continue;
        out[n++] = (v < dc) ? (v - lo) : (v - lo - 1);
    }
    return DABGPU_OK;
}

int dabgpu_get_fft_twiddles(float* out) {
    if (!out) return DABGPU_ERR_INVALID_ARG;
    for (int m = 0; m < DABGPU_NB_FFT; m++) {
        const double a = 2.0 * M_PI * (double)m / (double)DABGPU_NB_FFT;
        out[2 * m] = (float)cos(a);
        out[2 * m + 1] = (float)(-sin(a));
    }
    return DABGPU_OK;
}

void dabgpu_sync_cfg_default(dabgpu_sync_cfg* cfg) {          // ofdm_demodulator.h:34-44
    if (!cfg) return;
    cfg->fine_freq_update_beta = 0.9f;
    cfg->is_coarse_freq_correction = 1;
    cfg->max_coarse_freq_correction_norm = 0.5f;
    cfg->coarse_freq_slow_beta = 0.1f;
    cfg->impulse_peak_threshold_db = 20.0f;
    cfg->impulse_peak_distance_probability = 0.15f;
}

void dabgpu_soft_cfg_default(dabgpu_soft_cfg* cfg) {
    if (!cfg) return;
    cfg->policy = DABGPU_SOFT_NORMALISED;
    cfg->level = 64.0f;
}

float dabgpu_soft_scale_host(const float* h_prs_useful, float level) {
    if (!h_prs_useful || !dabgpu::sb_level_ok(level)) return 0.0f;
    return dabgpu::sb_scale(level, dabgpu::sb_frame_power(h_prs_useful));
}

float dabgpu_diversity_scale_host(const float* k, const float* w, const int* valid, int n_branches, uint32_t* live_mask) {
    if (live_mask) *live_mask = 0;
    if (!k || n_branches < 1 || n_branches > DABGPU_DIVERSITY_MAX_BRANCHES) return 0.0f;
    return dabgpu::dv_scale(k, w, valid, n_branches, live_mask);
}

int dabgpu_diversity_plan(const dabgpu_diversity_branch* h_branches, int n_branches, size_t n_frames, const int8_t* d_bits, size_t bits_frame_stride,
                          int bits_layout, int symbols_per_block, dabgpu_diversity_geometry* out) {
    if (out) *out = dabgpu_diversity_geometry{};              // a refusal leaves no geometry behind
    if (!h_branches || !out) { dabgpu_set_error("diversity_plan: null branch table or result"); return DABGPU_ERR_INVALID_ARG; }
    const int st = dabgpu_host_plan_diversity(n_branches, n_frames, bits_layout, symbols_per_block, bits_frame_stride, out);
    if (st) return st;
    *out = dabgpu_diversity_geometry{};
    if (!d_bits || ((uintptr_t)d_bits & 15)) { dabgpu_set_error("diversity_plan: d_bits must be non-null and 16-byte aligned"); return DABGPU_ERR_INVALID_ARG; }
    for (int b = 0; b < n_branches; b++) {
        const dabgpu_diversity_branch& B = h_branches[b];
        if (!B.d_dqpsk || !B.d_scale) { dabgpu_set_error("diversity_plan: branch %d has no products or no scales", b); return DABGPU_ERR_INVALID_ARG; }
        if ((uintptr_t)B.d_dqpsk & 15) { dabgpu_set_error("diversity_plan: branch %d: d_dqpsk must be 16-byte aligned", b); return DABGPU_ERR_INVALID_ARG; }
        if (((uintptr_t)B.d_scale | (uintptr_t)B.d_weight | (uintptr_t)B.d_sync) & 3) {
            dabgpu_set_error("diversity_plan: branch %d: scales, weights and sync records must be 4-byte aligned", b); return DABGPU_ERR_INVALID_ARG;
        }
    }
    return dabgpu_host_plan_diversity(n_branches, n_frames, bits_layout, symbols_per_block, bits_frame_stride, out);
}

float dabgpu_noise_unbias(void) { return dabgpu::NOISE_UNBIAS; }

int dabgpu_noise_floor_host(const float group_energy[192], float signal_power, dabgpu_noise_record* out) {
    if (out) *out = dabgpu_noise_record{};
    if (!group_energy || !out) return 0;
    return dabgpu::noise_finish(dabgpu::noise_floor(group_energy), signal_power, out) ? 1 : 0;
}

using namespace dabgpu;           // (from here on: the planners below read as their rules)

int dabgpu_noise_plan(int transmission_mode, const float* d_iq, size_t n_frames, size_t stream_stride_samples, size_t null_offset_samples,
                      const dabgpu_sync_state* d_states, const float* d_freq_offset, const float* d_noise_power, const float* d_signal_power,
                      const float* d_weight, const float* d_snr, const float* d_group_energy, const uint32_t* d_valid, dabgpu_noise_geometry* out) {
    static const char who[] = "noise_plan";
    if (plan_open(who, out, transmission_mode, n_frames) || plan_input(who, plan_or(d_iq), 8, "samples", "d_iq") ||
        plan_aligned(who, plan_or(d_states, d_freq_offset, d_noise_power, d_signal_power, d_weight, d_snr, d_group_energy, d_valid), 4,
                     "records, offsets and outputs") ||
        plan_null_reach(who, stream_stride_samples, null_offset_samples, NOISE_REACH, d_states != nullptr) ||
        plan_any_output(who, plan_or(d_noise_power, d_signal_power, d_weight, d_snr, d_group_energy, d_valid)))
        return DABGPU_ERR_INVALID_ARG;
    return plan_per_frame(out, n_frames, DABGPU_NOISE_THREADS, DABGPU_NOISE_LDS_BYTES);
}

int dabgpu_noise_profile_plan(int transmission_mode, const float* d_iq, size_t n_frames, size_t stream_stride_samples, size_t null_offset_samples,
                              const dabgpu_sync_state* d_states, const float* d_freq_offset, const uint32_t* d_exclude, const float* d_profile_in,
                              float alpha, const float* d_profile_out, const float* d_band_weight, const float* d_mean_noise,
                              const float* d_carrier_power, const uint32_t* d_valid, dabgpu_noise_geometry* out) {
    static const char who[] = "noise_profile_plan";
    if (plan_open(who, out, transmission_mode, n_frames) || plan_input(who, plan_or(d_iq), 8, "samples", "d_iq") ||
        plan_aligned(who, plan_or(d_states, d_freq_offset, d_exclude, d_profile_in, d_profile_out, d_band_weight, d_mean_noise, d_carrier_power, d_valid), 4,
                     "records, offsets, tables and outputs") ||
        plan_null_reach(who, stream_stride_samples, null_offset_samples, NP_NULL, d_states != nullptr))
        return DABGPU_ERR_INVALID_ARG;
    if (!np_alpha_ok(alpha)) { dabgpu_set_error("%s: alpha %g outside (0, 1]", who, (double)alpha); return DABGPU_ERR_INVALID_ARG; }
    if (plan_in_place(who, d_profile_in, d_profile_out, (uintptr_t)n_frames * NP_BANDS * sizeof(float), "d_profile_in", "d_profile_out") ||
        plan_any_output(who, plan_or(d_profile_out, d_band_weight, d_mean_noise, d_carrier_power, d_valid)))
        return DABGPU_ERR_INVALID_ARG;
    return plan_per_frame(out, n_frames, DABGPU_NOISE_PROFILE_THREADS, DABGPU_NOISE_PROFILE_LDS_BYTES);
}

int dabgpu_noise_profile_bands_host(const float carrier_power[1536], const uint32_t* exclude, const float* profile_in, float alpha,
                                    float* profile_out, float* band_weight, float* mean_noise) {
    if (!carrier_power || !dabgpu::np_alpha_ok(alpha)) return -1;
    return dabgpu::np_frame_bands(carrier_power, exclude, profile_in, alpha, profile_out, band_weight, mean_noise) ? 1 : 0;
}

int dabgpu_noise_profile_exclude_tii(const uint8_t* main_ids, const uint8_t* sub_ids, int n, uint32_t out[48]) {
    if (!out || n < 0 || (n > 0 && (!main_ids || !sub_ids))) { dabgpu_set_error("noise_profile_exclude_tii: null argument"); return DABGPU_ERR_INVALID_ARG; }
    for (int i = 0; i < dabgpu::NP_EXCLUDE_WORDS; i++) out[i] = 0u;
    for (int i = 0; i < n; i++) {
        if (main_ids[i] >= DABGPU_TII_NB_MAIN || sub_ids[i] >= DABGPU_TII_COMBS) {
            dabgpu_set_error("noise_profile_exclude_tii: transmitter %d: main_id %d, sub_id %d out of range", i, main_ids[i], sub_ids[i]);
            for (int j = 0; j < dabgpu::NP_EXCLUDE_WORDS; j++) out[j] = 0u;
            return DABGPU_ERR_INVALID_ARG;
        }
        for (int q = 0; q < 32; q++) {
            int k0;
            const int c = dabgpu::np_carrier_index(dabgpu::tii_carrier(main_ids[i], sub_ids[i], q, &k0));
            out[c >> 5] |= 1u << (c & 31);
        }
    }
    return DABGPU_OK;
}

int dabgpu_dd_profile_plan(int transmission_mode, const float* d_dqpsk, size_t n_frames, const dabgpu_sync_state* d_sync, const uint32_t* d_exclude,
                           const float* d_profile_in, float alpha, const float* d_profile_out, const float* d_band_weight, const float* d_mean_noise,
                           const float* d_carrier_noise, const float* d_carrier_amplitude, const uint32_t* d_valid, dabgpu_noise_geometry* out) {
    static const char who[] = "dd_profile_plan";
    if (plan_open(who, out, transmission_mode, n_frames) || plan_input(who, plan_or(d_dqpsk), 16, "products", "d_dqpsk") ||
        plan_aligned(who, plan_or(d_sync, d_exclude, d_profile_in, d_profile_out, d_band_weight, d_mean_noise, d_valid), 4, "records, tables and outputs") ||
        plan_aligned(who, plan_or(d_carrier_noise, d_carrier_amplitude), 8, "d_carrier_noise and d_carrier_amplitude"))
        return DABGPU_ERR_INVALID_ARG;
    if (!np_alpha_ok(alpha)) { dabgpu_set_error("%s: alpha %g outside (0, 1]", who, (double)alpha); return DABGPU_ERR_INVALID_ARG; }
    if (plan_in_place(who, d_profile_in, d_profile_out, (uintptr_t)n_frames * NP_BANDS * sizeof(float), "d_profile_in", "d_profile_out") ||
        plan_any_output(who, plan_or(d_profile_out, d_band_weight, d_mean_noise, d_carrier_noise, d_carrier_amplitude, d_valid)))
        return DABGPU_ERR_INVALID_ARG;
    return plan_per_frame(out, n_frames, DABGPU_DD_PROFILE_THREADS, DABGPU_DD_PROFILE_LDS_BYTES);
}

int dabgpu_dd_profile_carriers_host(const float* dqpsk, float* carrier_noise, float* carrier_amplitude) {
    if (!dqpsk) return -1;
    dabgpu::ddp_frame_carriers(dqpsk, carrier_noise, carrier_amplitude);
    return 0;
}

int dabgpu_sym_profile_plan(int transmission_mode, const float* d_dqpsk, size_t n_frames, const dabgpu_sync_state* d_sync, const float* d_symbol_weight,
                            const float* d_symbol_noise, const float* d_ref_noise, const uint32_t* d_valid, dabgpu_noise_geometry* out) {
    static const char who[] = "sym_profile_plan";
    if (plan_open(who, out, transmission_mode, n_frames) || plan_input(who, plan_or(d_dqpsk), 16, "products", "d_dqpsk") ||
        plan_aligned(who, plan_or(d_sync, d_symbol_weight, d_symbol_noise, d_ref_noise, d_valid), 4, "records and outputs") ||
        plan_any_output(who, plan_or(d_symbol_weight, d_symbol_noise, d_ref_noise, d_valid)))
        return DABGPU_ERR_INVALID_ARG;
    return plan_per_frame(out, n_frames, DABGPU_SYM_PROFILE_THREADS, DABGPU_SYM_PROFILE_LDS_BYTES);
}

int dabgpu_sym_profile_rows_host(const float* dqpsk, float* symbol_weight, float* symbol_noise, float* ref_noise) {
    if (!dqpsk) return -1;
    return dabgpu::syp_frame(dqpsk, true, symbol_weight, symbol_noise, ref_noise) ? 1 : 0;
}

int dabgpu_clock_estimate_plan(int transmission_mode, const float* d_dqpsk, size_t n_frames, const dabgpu_sync_state* d_sync, const int64_t* d_slope_in,
                               float gain, const int64_t* d_slope_out, const int64_t* d_residual, const float* d_corr, const uint32_t* d_valid,
                               dabgpu_noise_geometry* out) {
    static const char who[] = "clock_estimate_plan";
    if (plan_open(who, out, transmission_mode, n_frames) || plan_input(who, plan_or(d_dqpsk), 16, "products", "d_dqpsk") ||
        plan_aligned(who, plan_or(d_slope_in, d_slope_out, d_residual), 8, "slope words") ||
        plan_aligned(who, plan_or(d_sync, d_corr, d_valid), 4, "records and outputs"))
        return DABGPU_ERR_INVALID_ARG;
    if (!clk_gain_ok(gain)) { dabgpu_set_error("%s: gain %g outside (0, 1]", who, (double)gain); return DABGPU_ERR_INVALID_ARG; }
    if (plan_in_place(who, d_slope_in, d_slope_out, (uintptr_t)n_frames * sizeof(int64_t), "d_slope_in", "d_slope_out") ||
        plan_any_output(who, plan_or(d_slope_out, d_residual, d_corr, d_valid)))
        return DABGPU_ERR_INVALID_ARG;
    return plan_per_frame(out, n_frames, DABGPU_CLOCK_THREADS, DABGPU_CLOCK_ESTIMATE_LDS_BYTES);
}

int dabgpu_clock_derotate_plan(int transmission_mode, const float* d_dqpsk_in, const float* d_dqpsk_out, size_t n_frames, const dabgpu_sync_state* d_sync,
                               const int64_t* d_slope, int symbols_per_block, dabgpu_diversity_geometry* out) {
    static const char who[] = "clock_derotate_plan";
    if (plan_open(who, out, transmission_mode, n_frames) ||
        plan_input(who, d_dqpsk_in && d_dqpsk_out ? plan_or(d_dqpsk_in, d_dqpsk_out) : 0, 16, "products", "products") ||
        plan_in_place(who, d_dqpsk_in, d_dqpsk_out, (uintptr_t)n_frames * CLK_SYMBOLS * CLK_CARRIERS * 2 * sizeof(float), "d_dqpsk_in", "d_dqpsk_out") ||
        plan_input(who, plan_or(d_slope), 8, "slope words", "slope words") || plan_aligned(who, plan_or(d_sync), 4, "records"))
        return DABGPU_ERR_INVALID_ARG;
    if (symbols_per_block < 0 || symbols_per_block > CLK_SYMBOLS) {
        dabgpu_set_error("%s: symbols_per_block %d outside 0 .. 75", who, symbols_per_block); return DABGPU_ERR_INVALID_ARG;
    }
    const uint32_t spb = symbols_per_block ? (uint32_t)symbols_per_block : (uint32_t)dabgpu_host_small_batch_spb(n_frames);
    out->symbols_per_block = spb;
    out->runs_per_frame = (75u + spb - 1u) / spb;
    out->grid = (uint32_t)n_frames * out->runs_per_frame;            // at most 2^24 x 75
    out->threads = DABGPU_CLOCK_THREADS;
    out->lds_bytes = DABGPU_CLOCK_DEROTATE_LDS_BYTES;
    return DABGPU_OK;
}

int dabgpu_clock_estimate_host(const float* dqpsk, int64_t slope_in, float gain, int64_t* slope_out, float* corr) {
    if (!dqpsk || !dabgpu::clk_gain_ok(gain)) return -1;
    const dabgpu::clk_update u = dabgpu::clk_estimate_frame(dqpsk, true, slope_in, gain, corr);
    if (slope_out) *slope_out = u.slope;
    return u.valid ? 1 : 0;
}

int dabgpu_clock_derotate_host(const float* dqpsk_in, float* dqpsk_out, int64_t slope_q64) {
    if (!dqpsk_in || !dqpsk_out) return -1;
    dabgpu::clk_derotate_frame(dqpsk_in, dqpsk_out, slope_q64);
    return 0;
}

// slope = ppm * 1e-6 * 2552 / 2048 cycles per carrier, as Q0.64
int64_t dabgpu_clock_slope_q64(double ppm) {
    const double s = ppm * (2552.0 / 2048.0 * 1e-6) * 18446744073709551616.0;
    if (s != s) return 0;
    if (s < -9.2e18) return INT64_MIN;
    if (s > 9.2e18) return INT64_MAX;
    return (int64_t)llrint(s);
}
double dabgpu_clock_ppm(int64_t slope_q64) { return (double)slope_q64 * (1.0 / 18446744073709551616.0) * (2048.0 / 2552.0 * 1e6); }

float dabgpu_diversity_band_mean_host(const float band_weight[128]) { return band_weight ? dabgpu::np_branch_weight(band_weight) : 0.0f; }

int dabgpu_diversity_plan_banded(const dabgpu_diversity_branch* h_branches, int n_branches, size_t n_frames, const int8_t* d_bits,
                                 size_t bits_frame_stride, int bits_layout, int symbols_per_block, const float* const* h_band_weight,
                                 dabgpu_diversity_geometry* out) {
    return dabgpu_host_plan_diversity_mode(h_branches, n_branches, n_frames, d_bits, bits_frame_stride, bits_layout, symbols_per_block, h_band_weight,
                                           nullptr, out, nullptr);
}

int dabgpu_diversity_plan_symbols(const dabgpu_diversity_branch* h_branches, int n_branches, size_t n_frames, const int8_t* d_bits,
                                  size_t bits_frame_stride, int bits_layout, int symbols_per_block, const float* const* h_band_weight,
                                  const float* const* h_symbol_weight, dabgpu_diversity_geometry* out) {
    return dabgpu_host_plan_diversity_mode(h_branches, n_branches, n_frames, d_bits, bits_frame_stride, bits_layout, symbols_per_block, h_band_weight,
                                           h_symbol_weight, out, nullptr);
}

void dabgpu_stream_cfg_default(dabgpu_stream_cfg* c) {
    if (!c) return;
    c->signal_l1_update_beta = 0.95f; c->signal_l1_nb_samples = 100; c->signal_l1_nb_decimate = 5;      // ofdm_demodulator.h:25-29
    c->thresh_null_start = 0.35f; c->thresh_null_end = 0.75f;                                            // :30-33
    dabgpu_sync_cfg_default(&c->sync);
}

int dabgpu_get_ofdm_params(int mode, int* out9) {
    dabgpu::ModeGeom g;
    if (!out9 || !dabgpu::mode_geometry(mode, g)) { dabgpu_set_error("get_ofdm_params: invalid transmission mode %d", mode); return DABGPU_ERR_INVALID_ARG; }
    out9[0] = g.n_sym; out9[1] = g.period; out9[2] = g.null_period; out9[3] = g.n_fft; out9[4] = g.n_cp; out9[5] = g.n_carriers;
    out9[6] = g.frame_samples; out9[7] = g.sym_bits; out9[8] = g.frame_bits;
    return DABGPU_OK;
}

int dabgpu_iq_format_from_mode(const char* mode) {
    static const char* const NAMES[14] = {"raw_u8", "raw_s8", "raw_s16l", "raw_s16b", "raw_u16l", "raw_u16b", "raw_s32l",
                                          "raw_s32b", "raw_u32l", "raw_u32b", "raw_f32l", "raw_f32b", "raw_f64l", "raw_f64b"};
    if (!mode) return -1;
    for (int i = 0; i < 14; i++) if (strcmp(mode, NAMES[i]) == 0) return i;
    return -1;
}

size_t dabgpu_iq_format_sample_bytes(int format) {
    if (format < 0 || format >= DABGPU_IQ_NB_FORMATS) return 0;
    // bytes per component: raw u8 s8 | s16l s16b u16l u16b | s32l s32b u32l u32b | f32l f32b | f64l f64b | wav pcm8 pcm16 pcm24 pcm32 f32 f64 alaw mulaw
    static const unsigned char SIZE[DABGPU_IQ_NB_FORMATS] = {1, 1, 2, 2, 2, 2, 4, 4, 4, 4, 4, 4, 8, 8, 1, 2, 3, 4, 4, 8, 1, 1};
    return 2 * (size_t)SIZE[format];
}

}  // extern "C"

// batches too small to fill the chip with three workgroups per frame: more, shorter runs -- a single frame in three runs of 25 symbols is
// three workgroups 25 symbols long (130 us); in 25 runs of 3 symbols (4 transforms each, one of them the halo) it is 25 workgroups 20 us
// long.  Aim at ~256 workgroups, at most 25 runs per frame; from 86 frames on the usual three runs.
int dabgpu_host_small_batch_spb(size_t n_frames) {
    if (n_frames >= 86) return 25;
    const size_t chunks = std::min<size_t>(25, (256 + n_frames - 1) / n_frames);
    return (int)((75 + chunks - 1) / chunks);
}

// size bucket of a batch: ceil(log2(n_frames)) -- 513..1024 frames share a bucket, 1025..2048 the next
int dabgpu_host_spb_bucket(size_t n_frames) {
    int b = 0;
    while (((size_t)1 << b) < n_frames && b < 40) b++;
    return b;
}
// kernel variant of a call: loader (0..3), soft-bit layout, whether the phase tail runs with it (fused at 75, a second launch otherwise)
int dabgpu_host_spb_variant(int src, int bits_layout, bool tail) { return src * 4 + (bits_layout == DABGPU_BITS_MSC_CLASSED ? 2 : 0) + (tail ? 1 : 0); }

int dabgpu_host_check_soft_cfg(const char* who, const dabgpu_soft_cfg* cfg) {
    if (!cfg) { dabgpu_set_error("%s: null soft-decision configuration", who); return DABGPU_ERR_INVALID_ARG; }
    if (cfg->policy != DABGPU_SOFT_NORMALISED && cfg->policy != DABGPU_SOFT_CSI) {
        dabgpu_set_error("%s: no soft-decision policy %d", who, cfg->policy); return DABGPU_ERR_INVALID_ARG;
    }
    if (!dabgpu::sb_level_ok(cfg->level)) { dabgpu_set_error("%s: soft level %g outside [1, 127]", who, (double)cfg->level); return DABGPU_ERR_INVALID_ARG; }
    return DABGPU_OK;
}

int dabgpu_host_plan_diversity(int n_branches, size_t n_frames, int bits_layout, int symbols_per_block, size_t bits_frame_stride,
                               dabgpu_diversity_geometry* out) {
    *out = dabgpu_diversity_geometry{};
    if (n_branches < 1 || n_branches > DABGPU_DIVERSITY_MAX_BRANCHES) {
        dabgpu_set_error("diversity_plan: n_branches %d outside 1 .. %d", n_branches, DABGPU_DIVERSITY_MAX_BRANCHES); return DABGPU_ERR_INVALID_ARG;
    }
    if (n_frames > (size_t)(1 << 24)) { dabgpu_set_error("diversity_plan: n_frames too large"); return DABGPU_ERR_INVALID_ARG; }
    if (bits_layout != DABGPU_BITS_NATURAL && bits_layout != DABGPU_BITS_MSC_CLASSED) {
        dabgpu_set_error("diversity_plan: unknown bits_layout %d", bits_layout); return DABGPU_ERR_INVALID_ARG;
    }
    if (symbols_per_block < 0 || symbols_per_block > 75) {
        dabgpu_set_error("diversity_plan: symbols_per_block %d outside 0 .. 75", symbols_per_block); return DABGPU_ERR_INVALID_ARG;
    }
    if (bits_frame_stride != 0 && (bits_frame_stride < DABGPU_NB_FRAME_BITS || (bits_frame_stride & 15))) {
        dabgpu_set_error("diversity_plan: bits_frame_stride must be 0 or a multiple of 16 >= 230400"); return DABGPU_ERR_INVALID_ARG;
    }
    const uint32_t spb = symbols_per_block ? (uint32_t)symbols_per_block : (uint32_t)dabgpu_host_small_batch_spb(n_frames ? n_frames : 1);
    out->symbols_per_block = spb;
    out->runs_per_frame = (75u + spb - 1u) / spb;
    out->grid = (uint32_t)n_frames * out->runs_per_frame;            // at most 2^24 x 75
    out->threads = DABGPU_DIVERSITY_THREADS;
    out->lds_bytes = DABGPU_DIVERSITY_LDS_BYTES;
    return DABGPU_OK;
}

// an optional table per branch (band weights, symbol weights): every entry given 4-byte aligned and, where the table stands in for the
// branch's weight, no d_weight beside it.  0: no entry at all, 1: at least one, -1: refused, the reason set
static int dv_optional_tables(const char* who, const char* noun, const float* const* table, const dabgpu_diversity_branch* br, int n, bool for_weight) {
    int any = 0;
    for (int b = 0; table && b < n; b++) {
        if (!table[b]) continue;
        any = 1;
        if ((uintptr_t)table[b] & 3) { dabgpu_set_error("%s: branch %d: %s weights must be 4-byte aligned", who, b, noun); return -1; }
        if (for_weight && br[b].d_weight) { dabgpu_set_error("%s: branch %d has both a %s table and d_weight", who, b, noun); return -1; }
    }
    return any;
}

int dabgpu_host_plan_diversity_mode(const dabgpu_diversity_branch* h_branches, int n_branches, size_t n_frames, const int8_t* d_bits,
                                    size_t bits_frame_stride, int bits_layout, int symbols_per_block, const float* const* h_band_weight,
                                    const float* const* h_symbol_weight, dabgpu_diversity_geometry* out, int* mode) {
    if (mode) *mode = 0;
    const int st = dabgpu_diversity_plan(h_branches, n_branches, n_frames, d_bits, bits_frame_stride, bits_layout, symbols_per_block, out);
    if (st) return st;
    const int band = dv_optional_tables("diversity_plan_banded", "band", h_band_weight, h_branches, n_branches, true);
    const int sym = band < 0 ? -1 : dv_optional_tables("diversity_plan_symbols", "symbol", h_symbol_weight, h_branches, n_branches, false);
    if (sym < 0) { *out = dabgpu_diversity_geometry{}; return DABGPU_ERR_INVALID_ARG; }
    if (band || sym) out->lds_bytes = DABGPU_DIVERSITY_BANDED_LDS_BYTES;      // the third instantiation keeps the banded one's LDS
    if (mode) *mode = sym ? 2 : band;
    return DABGPU_OK;
}

dabgpu_demod_plan dabgpu_host_plan_demod(int mode, const dabgpu_demod_facts& f) {
    dabgpu_demod_plan p = {};
    p.status = DABGPU_ERR_INVALID_ARG;
    dabgpu::ModeGeom g;
    if (!dabgpu::mode_geometry(mode, g)) { dabgpu_set_error("ofdm_demod: invalid transmission mode %d", mode); return p; }
    const bool mode1 = mode == 1 && !f.generic_mode1;
    const bool views = f.fft || f.dqpsk;
    if (mode1) {
        if (f.src < 0 || f.src > 3) { dabgpu_set_error("ofdm_demod: no loader %d", f.src); return p; }
        if (f.classed && views) { dabgpu_set_error("ofdm_demod: soft bits in class order come without the display views"); return p; }
        if (f.desc && (f.sync || f.frame_stride)) { dabgpu_set_error("ofdm_demod: a bank round takes neither sync records nor a frame stride"); return p; }
        p.family = DABGPU_DEMOD_MODE1;
        p.variant = (f.src * 2 + (f.desc ? 1 : 0)) * 3 + (f.classed ? 2 : views ? 1 : 0);
    }
    // bank_soft is the stream bank's explicit statement that its round runs the weighted policy: it means nothing without descriptors or
    // under the normalised policy, and a caller that hands descriptors without it is refused as before
    if (f.bank_soft && !f.desc) { dabgpu_set_error("ofdm_demod: bank_soft is a bank round's fact: it needs frame descriptors"); return p; }
    if (f.bank_soft && f.soft_policy == DABGPU_SOFT_NORMALISED) { dabgpu_set_error("ofdm_demod: bank_soft asks for DABGPU_SOFT_CSI, the policy is the normalised one"); return p; }
    // bank_products is the bank's statement that the round also stores every frame's DQPSK products at the frame's bits slot: a round under
    // the weighted policy (bank_soft and all it asks for), in the natural layout, without the display views (whose buffers are indexed by
    // stream, not by slot)
    if (f.bank_products && !f.bank_soft) { dabgpu_set_error("ofdm_demod: bank_products is a weighted bank round's fact: it needs bank_soft"); return p; }
    if (f.bank_products && f.classed) { dabgpu_set_error("ofdm_demod: bank_products comes in the natural layout: classed is not available with it"); return p; }
    if (f.bank_products && f.fft) { dabgpu_set_error("ofdm_demod: bank_products has no FFT view: fft is not available with it"); return p; }
    if (f.bank_products && f.dqpsk) { dabgpu_set_error("ofdm_demod: bank_products stores the products by bits slot: dqpsk, the view by frame, is not available with it"); return p; }
    if (f.soft_policy != DABGPU_SOFT_NORMALISED) {
        if (f.soft_policy != DABGPU_SOFT_CSI) { dabgpu_set_error("ofdm_demod: no soft-decision policy %d", f.soft_policy); return p; }
        if (!mode1) { dabgpu_set_error("ofdm_demod: the weighted soft bits exist for the transmission mode I kernel only (mode %d)", mode); return p; }
        if (f.desc && !f.bank_soft) { dabgpu_set_error("ofdm_demod: the weighted soft bits have no stream-bank loader (frame descriptors)"); return p; }
        if (f.bank_soft && views) { dabgpu_set_error("ofdm_demod: a bank round has no display views under the weighted policy"); return p; }
        if (!dabgpu::sb_level_ok(f.soft_level)) { dabgpu_set_error("ofdm_demod: soft level %g outside [1, 127]", (double)f.soft_level); return p; }
        p.variant = f.bank_products ? DABGPU_DEMOD_MODE1_BANK_PRODUCTS_FIRST + f.src
                    : f.bank_soft   ? DABGPU_DEMOD_MODE1_BANK_SOFT_FIRST + f.src * 2 + (f.classed ? 1 : 0)
                                : DABGPU_DEMOD_MODE1_NORMALISED_VARIANTS + f.src * 3 + (f.classed ? 2 : views ? 1 : 0);
    }
    if (!mode1) {
        // modes II-IV run register-resident unless the FFT view, which only the size-generic kernel writes, is wanted
        p.family = (mode == 1 || f.fft || f.switch_generic) ? DABGPU_DEMOD_GENERIC
                   : (mode == 3 && !f.switch_mode3_single)   ? DABGPU_DEMOD_WAVE3
                                                             : DABGPU_DEMOD_WAVE;
        // (a loader these kernels do not know runs as s16, as it always has: the entry points check the format, dabgpu_fused_loader)
        p.variant = !f.desc ? 0 : 1 + ((f.src >= 0 && f.src <= 2) ? f.src : 3);
    }
    // mode I default: three runs per frame (one extra FFT per run).  A whole frame per workgroup (75) is 1 % faster when 1024 frames are
    // exactly one round of a 256-CU chip (and lets the phase tail run inside the kernel) but 25 % slower on boxes whose CUs do not
    // all run at one speed (workgroup lifetimes 0.33 .. 0.53 ms in one static round: 0.536 against 0.427 ms): callers that care
    // time both (bench.py does) and pass it.  The other modes: 19 symbols.
    const int n_out = g.n_sym - 1;
    p.symbols_per_block = (f.symbols_per_block <= 0 || f.symbols_per_block > n_out) ? (mode1 ? 25 : 19) : f.symbols_per_block;
    p.chunks = (n_out + p.symbols_per_block - 1) / p.symbols_per_block;
    const uint64_t units = (uint64_t)(f.n_frames > 0 ? f.n_frames : 0) * (uint64_t)p.chunks;
    const bool wave = p.family == DABGPU_DEMOD_WAVE || p.family == DABGPU_DEMOD_WAVE3;      // four runs, one per wavefront, to a workgroup
    p.grid = (uint32_t)(wave ? (units + 3) / 4 : units);
    // size-generic kernel, measured (tools/bench_io.py, 2048 frames): FFT 512 / 256 run best with 128 threads (0.94 / 1.01 ms; 256 threads
    // 1.03 / 1.47, 64 threads 1.19 / 1.01), FFT 1024 with 256 (1.93 ms; 128 threads 2.58): fewer idle butterfly lanes against fewer resident wavefronts
    p.threads = (p.family == DABGPU_DEMOD_GENERIC && (mode == 2 || mode == 3)) ? 128 : 256;
    // size-generic kernel: one PLL-corrected symbol, three transform buffers, 2 x 256 reduction leaves
    p.lds_bytes = p.family == DABGPU_DEMOD_GENERIC ? (uint32_t)((g.period + 3 * g.n_fft) * 8 + 2048) : 0;
    p.raise_lds_limit = p.lds_bytes > 48u * 1024u;
    // the phase tail (mode I): inside the kernel when one workgroup walks the whole frame, else a launch of its own; a bank round runs its
    // own phase kernel over the descriptors.  With sync records the fine-frequency word is the record's.
    p.fine_stride = f.sync ? (int)(sizeof(dabgpu_sync_state) / sizeof(float)) : 1;
    const bool want_tail = mode1 && !f.desc && (f.total_phase || f.fine_freq || f.sync);
    p.tail = !want_tail ? DABGPU_DEMOD_TAIL_NONE : (p.chunks == 1 && !views) ? DABGPU_DEMOD_TAIL_FUSED : DABGPU_DEMOD_TAIL_LAUNCH;
    p.status = DABGPU_OK;
    return p;
}


// ETSI EN 300 401 tables 8 + 15: {size CU, kbps, level, L1..L4, PI1..PI4, padding bits}; row order (and the two
// exchanged size fields of rows 33/34) as the reference lists them, src/dab/constants/subchannel_protection_tables.h:21-86,
// because FIG 0/1 short-form sub-channels index this table by position
static const uint16_t UEP_ROWS[64][12] = {
    {16,32,5,3,4,17,0,5,3,2,0,0},       {21,32,4,3,3,18,0,11,6,5,0,0},      {24,32,3,3,4,14,3,15,9,6,8,0},
    {29,32,2,3,4,14,3,22,13,8,13,0},    {35,32,1,3,5,13,3,24,17,12,17,4},   {24,48,5,4,3,26,3,5,4,2,3,0},
    {29,48,4,3,4,26,3,9,6,4,6,0},       {35,48,3,3,4,26,3,15,10,6,9,4},     {42,48,2,3,4,26,3,24,14,8,15,0},
    {52,48,1,3,5,25,3,24,18,13,18,0},   {29,56,5,6,10,23,3,5,4,2,3,0},      {35,56,4,6,10,23,3,9,6,4,5,0},
    {42,56,3,6,12,21,3,16,7,6,9,0},     {52,56,2,6,10,23,3,23,13,8,13,8},   {32,64,5,6,9,31,2,5,3,2,3,0},
    {42,64,4,6,9,33,0,11,6,5,0,0},      {48,64,3,6,12,27,3,16,8,6,9,0},     {58,64,2,6,10,29,3,23,13,8,13,8},
    {70,64,1,6,11,28,3,24,18,12,18,4},  {40,80,5,6,10,41,3,6,3,2,3,0},      {52,80,4,6,10,41,3,11,6,5,6,0},
    {58,80,3,6,11,40,3,16,8,6,7,0},     {70,80,2,6,10,41,3,23,13,8,13,8},   {84,80,1,6,10,41,3,24,17,12,18,4},
    {48,96,5,7,9,53,3,5,4,2,4,0},       {58,96,4,7,10,52,3,9,6,4,6,0},      {70,96,3,6,12,51,3,16,9,6,10,4},
    {84,96,2,6,10,53,3,22,12,9,12,0},   {104,96,1,6,13,50,3,24,18,13,19,0}, {58,112,5,14,17,50,3,5,4,2,5,0},
    {70,112,4,11,21,49,3,9,6,4,8,0},    {84,112,3,11,23,47,3,16,8,6,9,0},   {104,112,2,11,21,49,3,23,12,9,14,4},
    {84,128,5,12,19,62,3,5,3,2,4,0},    {64,128,4,11,21,61,3,11,6,5,7,0},   {96,128,3,11,22,60,3,16,9,6,10,4},
    {116,128,2,11,21,61,3,22,12,9,14,0},{140,128,1,11,20,62,3,24,17,13,19,8},{80,160,5,11,19,87,3,5,4,2,4,0},
    {104,160,4,11,23,83,3,11,6,5,9,0},  {116,160,3,11,24,82,3,16,8,6,11,0}, {140,160,2,11,21,85,3,22,11,9,13,0},
    {168,160,1,11,22,84,3,24,18,12,19,0},{96,192,5,11,20,110,3,6,4,2,5,0},  {116,192,4,11,22,108,3,10,6,4,9,0},
    {140,192,3,11,24,106,3,16,10,6,11,0},{168,192,2,11,20,110,3,22,13,9,13,8},{208,192,1,11,21,109,3,24,20,13,24,0},
    {116,224,5,12,22,131,3,8,6,2,6,4},  {140,224,4,12,26,127,3,12,8,4,11,0},{168,224,3,11,20,134,3,16,10,7,9,0},
    {208,224,2,11,22,132,3,24,16,10,15,0},{232,224,1,11,24,130,3,24,20,12,20,4},{128,256,5,11,24,154,3,6,5,2,5,0},
    {168,256,4,11,24,154,3,12,9,5,10,4},{192,256,3,11,27,151,3,16,10,7,10,0},{232,256,2,11,22,156,3,24,14,10,13,8},
    {280,256,1,11,26,152,3,24,19,14,18,4},{160,320,5,11,26,200,3,8,5,2,6,4}, {208,320,4,11,25,201,3,13,9,5,10,8},
    {280,320,2,11,26,200,3,24,17,9,17,0},{192,384,5,11,27,247,3,8,6,2,7,0}, {280,384,3,11,24,250,3,16,9,7,10,4},
    {416,384,1,12,28,245,3,24,20,14,23,8},
};
// ETSI EN 300 401 tables 9/18 (EEP-A) and 10/20 (EEP-B): {CU multiple, m1, b1, m2, b2, PI1, PI2}, L = m*n + b;
// same data as subchannel_protection_tables.h:121-139
static const int EEP_A_ROWS[4][7] = { {12,6,-3,0,3,24,23}, {8,2,-3,4,3,14,13}, {6,6,-3,0,3,8,7}, {4,4,-3,2,3,3,2} };
static const int EEP_2A_N1[7] = { 8,0,5,0,1,13,12 };
static const int EEP_B_ROWS[4][7] = { {27,24,-3,0,3,10,9}, {21,24,-3,0,3,6,5}, {18,24,-3,0,3,4,3}, {15,24,-3,0,3,2,1} };

extern "C" int dabgpu_subchannel_plan(const dabgpu_subchannel* sc, int* pi, int* lx, int* n_decoded_bytes) {
    if (!sc || !pi || !lx) return -1;
    int nseg, total = 0;
    for (int i = 0; i < 4; i++) { pi[i] = 0; lx[i] = 0; }
    if (!sc->is_uep) {
        if (sc->eep_prot_level < 0 || sc->eep_prot_level > 3 || sc->length <= 0 || sc->length > 864) return -1;       // (a CIF has 864 capacity units)
        const int* d = (sc->eep_type == 0) ? ((sc->length == 8) ? EEP_2A_N1 : EEP_A_ROWS[sc->eep_prot_level])
                                            : EEP_B_ROWS[sc->eep_prot_level];       // GetEEPDescriptor :145-154
        const int n = sc->length / d[0];
        pi[0] = d[5]; lx[0] = d[1] * n + d[2];
        pi[1] = d[6]; lx[1] = d[3] * n + d[4];
        if (lx[0] < 0 || lx[1] < 0) return -1;
        nseg = 2;
    } else {
        if (sc->uep_prot_index < 0 || sc->uep_prot_index > 63) return -1;
        const uint16_t* d = UEP_ROWS[sc->uep_prot_index];
        for (int i = 0; i < 4; i++) { lx[i] = d[3 + i]; pi[i] = d[7 + i]; }
        nseg = 4;
    }
    for (int i = 0; i < nseg; i++) total += lx[i];
    if (n_decoded_bytes) *n_decoded_bytes = 4 * total;     // (32*sum(L) + 6 - 6) / 8, msc_decoder.cpp:99-103
    return nseg;
}


void dabgpu_host_fill_vit_tables(dabgpu_vit_tables* T) {
    memset(T, 0, sizeof(*T));
    static const int order[8] = {0, 4, 2, 6, 1, 5, 3, 7};
    for (int pi = 1; pi <= 24; pi++) {
        int cnt[8];
        for (int g = 0; g < 8; g++) cnt[g] = 1;
        for (int e = 0; e < pi; e++) cnt[order[e % 8]]++;
        int pre = 0;
        for (int g = 0; g < 8; g++) { T->pi_tab[pi * 8 + g] = (uint16_t)(cnt[g] | (pre << 8)); pre += cnt[g]; }
    }
    unsigned reg = 0xFFFFu;
    for (int k = 0; k < 511; k++) {
        unsigned b = 0;
        for (int i = 0; i < 8; i++) {
            const unsigned v = ((reg >> 8) ^ (reg >> 4)) & 1u;
            b |= v << (7 - i);
            reg = ((reg << 1) | v) & 0xFFFFu;
        }
        T->prbs[k] = (unsigned char)b;
    }
}

// DABGPU_VIT_MAP_AUTO: a cost model of the three mappings on this part (profiles/r01/ab_notes.md, profiles/r03/ab_notes.md; microseconds).
//   WAVE   one wavefront per codeword keeps every SIMD busy: t = sum over codewords of (0.0189 ns x steps + 0.038 us)
//   LANE   a group of 64 codewords is one wavefront that needs 0.5 us per trellis step however many of its lanes are used, and
//          a SIMD works through its groups at that same rate: t = 0.5 us x max(longest schedule, rounds x mean steps) with
//          rounds = ceil(groups / SIMDs), + the gather pass (3.3e-3 / 8.5e-3 us per codeword-kilostep, staged / byte-wise)
//   OCTET  a group is 8 wavefronts of ~57 instructions per step; two of them share a SIMD at 4 cycles per instruction (a lone one
//          issues at half rate, so one costs what two cost): t = 0.095 us x max(2 x longest schedule, rounds8 x mean steps) with
//          rounds8 = ceil(8 groups / SIMDs), + the same gather pass
// n_cw codewords in n_groups groups; sums and maximum of their trellis steps.  Returns DABGPU_VIT_MAP_WAVE / _LANE / _OCTET
int dabgpu_host_choose_mapping(int forced_mapping, double n_simd, size_t n_cw, size_t n_groups, double sum_cw_steps, double sum_group_steps, double max_steps,
                          bool staged_gather) {
    if (forced_mapping != DABGPU_VIT_MAP_AUTO) return forced_mapping;
    if (n_groups == 0) return DABGPU_VIT_MAP_WAVE;
    const double mean = sum_group_steps / (double)n_groups;
    const double gather = (staged_gather ? 3.3e-6 : 8.5e-6) * sum_cw_steps;
    // microseconds.  viterbi_kernel (re-fitted in round 5, after its chain-back went scalar): the latency of the longest code word on a lone wavefront
    // (~0.08 us per trellis step) + the throughput share of every code word -- 229 / 317 / 445 / 660 us for 32 / 64 / 100 / 160 ensembles of
    // 18 x 48 CU + FIC, 163 / 510 / 1926 us for the FIC of 1024 / 4096 / 16384 frames (tools/exp/map_crossover.py, profiles/r05/bench_fic_v4.json:
    // the fit is within 9 %).  The batch mappings: their rounds of wavefronts + the gather + ~20 us for their three set-up launches.
    const double t_wave = 0.08 * max_steps + 2.2e-5 * sum_cw_steps + 0.0113 * (double)n_cw;
    const double t_lane = 0.5 * std::max(max_steps, std::ceil((double)n_groups / n_simd) * mean) + gather + 20.0;
    const double t_oct = 0.095 * std::max(2.0 * max_steps, std::ceil(8.0 * (double)n_groups / n_simd) * mean) + gather + 20.0;
    if (t_wave <= t_lane && t_wave <= t_oct) return DABGPU_VIT_MAP_WAVE;
    return t_oct < t_lane ? DABGPU_VIT_MAP_OCTET : DABGPU_VIT_MAP_LANE;
}

// The MSC of n_ens ensembles that share a multiplex of n_sub sub-channels (steps[j] trellis steps each, 4 CIFs per call): the same cost
// model, groups = n_sub x ceil(4 n_ens / 64).  AUTO compares the three pure choices (a partial viterbi_kernel launch is one lockstep round of
// wavefronts and measured 2x its share of a full one: hybrids did not pay).  model_us (may be null) receives the modelled WAVE / LANE / OCTET
// times in microseconds.
int dabgpu_host_choose_msc_mapping(int forced_mapping, double n_simd, size_t n_ens, const uint32_t* steps, int n_sub, double* model_us) {
    double sum_steps = 0.0, max_st = 0.0;
    for (int j = 0; j < n_sub; j++) { sum_steps += (double)steps[j]; max_st = std::max(max_st, (double)steps[j]); }
    const double groups = (double)n_sub * (double)((n_ens * 4 + 63) / 64), mean = n_sub ? sum_steps / (double)n_sub : 0.0;
    const double gather = 3.3e-6 * sum_steps * (double)(n_ens * 4);
    const double t_wave = 0.08 * max_st + (double)(n_ens * 4) * (2.2e-5 * sum_steps + 0.0113 * (double)n_sub);
    const double t_lane = 0.5 * std::max(max_st, std::ceil(groups / n_simd) * mean) + gather + 20.0;
    const double t_oct = 0.095 * std::max(2.0 * max_st, std::ceil(8.0 * groups / n_simd) * mean) + gather + 20.0;
    if (model_us) { model_us[0] = t_wave; model_us[1] = t_lane; model_us[2] = t_oct; }
    if (forced_mapping != DABGPU_VIT_MAP_AUTO) return forced_mapping;
    if (t_lane < t_wave || t_oct < t_wave) return t_oct < t_lane ? DABGPU_VIT_MAP_OCTET : DABGPU_VIT_MAP_LANE;
    return DABGPU_VIT_MAP_WAVE;
}

int dabgpu_host_validate_codeword(const dabgpu_codeword& d, size_t i) {
    if (d.flags & DABGPU_CW_DEPUNCTURED) {            // mother code handed over: no segment tables, any length, direct source only
        if (d.n_steps < 1 || d.n_steps > DABGPU_MAX_TRELLIS_STEPS || d.n_slots != 0 || !d.d_src || !d.d_out) {
            dabgpu_set_error("codeword %zu: DABGPU_CW_DEPUNCTURED needs 1 <= n_steps <= %u, n_slots = 0 and non-null addresses", i, (unsigned)DABGPU_MAX_TRELLIS_STEPS);
            return DABGPU_ERR_INVALID_ARG;
        }
        return DABGPU_OK;
    }
    uint64_t steps = 0;
    for (int k = 0; k < 4; k++) {
        if (d.seg_steps[k] == 0) continue;
        if (d.seg_pi[k] < 1 || d.seg_pi[k] > 24 || (d.seg_steps[k] & 7)) {
            dabgpu_set_error("codeword %zu: segment %d has PI=%u steps=%u (PI must be 1..24, steps a multiple of 8)", i, k,
                             d.seg_pi[k], d.seg_steps[k]);
            return DABGPU_ERR_INVALID_ARG;
        }
        steps += d.seg_steps[k];
    }
    if (steps + 6 > DABGPU_MAX_TRELLIS_STEPS) {
        dabgpu_set_error("codeword %zu: %llu trellis steps, at most %u are decoded (the decoded bytes of a code word are assembled in LDS)", i,
                         (unsigned long long)steps + 6, (unsigned)DABGPU_MAX_TRELLIS_STEPS);
        return DABGPU_ERR_INVALID_ARG;
    }
    if (steps + 6 != d.n_steps || ((d.n_steps - 6) & 7) || !d.d_src || !d.d_out) {
        dabgpu_set_error("codeword %zu: n_steps=%u does not equal sum(seg_steps)+6 with whole output bytes, or null address", i, d.n_steps);
        return DABGPU_ERR_INVALID_ARG;
    }
    if ((d.flags & DABGPU_CW_CLASSED) && d.n_slots != 0 && (d.cif_stride == 0 || (d.cif_stride & 15))) {
        dabgpu_set_error("codeword %zu: DABGPU_CW_CLASSED needs cif_stride = soft bits per ring row, a multiple of 16 (got %u)", i, d.cif_stride);
        return DABGPU_ERR_INVALID_ARG;
    }
    if (d.n_slots != 0 && (d.n_slots < 16 || d.cifs_per_frame == 0 || d.newest_slot >= d.n_slots)) {
        dabgpu_set_error("codeword %zu: bad CIF ring geometry (n_slots=%u newest=%u cifs_per_frame=%u)", i, d.n_slots, d.newest_slot, d.cifs_per_frame);
        return DABGPU_ERR_INVALID_ARG;
    }
    return DABGPU_OK;
}


int dabgpu_host_build_msc_plans(const dabgpu_subchannel* h_sub, int n_sub, std::vector<dabgpu_msc_plan>& plans, uint32_t* cif_out_bytes,
                                uint32_t* max_steps_out, uint32_t* max_out_bytes) {
    if (!h_sub || n_sub < 0 || n_sub > 64) { dabgpu_set_error("msc_decode_frames: %d sub-channels (0..64 are accepted)", n_sub); return DABGPU_ERR_INVALID_ARG; }
    plans.assign((size_t)n_sub, dabgpu_msc_plan{});
    uint32_t off = 0, max_steps = 0, max_out = 0;
    for (int s = 0; s < n_sub; s++) {
        int pi[4], lx[4], nb = 0;
        // (ranges first: start + length of a hostile descriptor overflows int)
        if (h_sub[s].length <= 0 || h_sub[s].length > 864 || h_sub[s].start_address < 0 || h_sub[s].start_address > 864 - h_sub[s].length ||
            dabgpu_subchannel_plan(&h_sub[s], pi, lx, &nb) < 0) {
            dabgpu_set_error("msc_decode_frames: sub-channel %d has an invalid protection profile or exceeds 864 CU", s);
            return DABGPU_ERR_INVALID_ARG;
        }
        {   // a profile that consumes more soft bits than the sub-channel holds (a UEP table row paired with another size) would make the
            // gather read its neighbours: the reference's decoder runs out of symbols instead (dab_viterbi_decoder.cpp:157-160); refuse it
            uint32_t need = 12;
            for (int k = 0; k < 4; k++) need += 4u * (uint32_t)lx[k] * (8u + (uint32_t)pi[k]);
            if (need > (uint32_t)h_sub[s].length * 64u) {
                dabgpu_set_error("msc_decode_frames: sub-channel %d: its protection profile consumes %u soft bits, %d capacity units hold %u", s, need,
                                 h_sub[s].length, (uint32_t)h_sub[s].length * 64u);
                return DABGPU_ERR_INVALID_ARG;
            }
        }
        dabgpu_msc_plan& P = plans[(size_t)s];
        P.start_address = (uint32_t)h_sub[s].start_address;
        uint32_t steps = 0;
        for (int k = 0; k < 4; k++) { P.seg_pi[k] = lx[k] ? (uint32_t)pi[k] : 0u; P.seg_steps[k] = 32u * (uint32_t)lx[k]; steps += P.seg_steps[k]; }
        P.n_steps = steps + 6;
        P.out_offset = off;
        P.n_out_bytes = (uint32_t)nb;
        off += (uint32_t)nb;
        max_steps = std::max(max_steps, P.n_steps);
        max_out = std::max(max_out, (uint32_t)nb);
    }
    if (cif_out_bytes) *cif_out_bytes = off;
    if (max_steps_out) *max_steps_out = max_steps;
    if (max_out_bytes) *max_out_bytes = max_out;
    return DABGPU_OK;
}

// ---- decode planner ----
static size_t mul_sat(size_t a, size_t b) { size_t r; return __builtin_mul_overflow(a, b, &r) ? SIZE_MAX : r; }
static size_t add_sat(size_t a, size_t b) { size_t r; return __builtin_add_overflow(a, b, &r) ? SIZE_MAX : r; }

dabgpu_uniform_plan dabgpu_host_plan_uniform(size_t n_cw, uint32_t n_steps, const uint32_t* seg_pi, const uint32_t* seg_steps, bool staged_gather,
                                             const dabgpu_decode_limits& lim) {
    dabgpu_uniform_plan u;
    const size_t n_groups = n_cw / 64 + (n_cw % 64 != 0);
    u.mapping = dabgpu_host_choose_mapping(lim.forced_mapping, lim.n_simd, n_cw, n_groups, (double)n_cw * n_steps, (double)n_groups * n_steps,
                                           (double)n_steps, staged_gather);
    u.dec_rows = dabgpu_vit_alloc_steps(n_steps);
    u.in_rows = dabgpu_vit_in_rows(dabgpu_vit_in_bytes(seg_pi, seg_steps));
    u.slice_groups = std::max<size_t>(1, lim.max_dec_rows / u.dec_rows);
    return u;
}

// vit_prep_kernel forms, in uint32_t, aoff = frame * frame_stride + cif * cif_stride + class * (cif_stride / 16) with
// frame <= (n_slots - 1) / cifs_per_frame, cif <= cifs_per_frame - 1, class <= 15 (class-order rows only; counted for both layouts), and
// widens before it adds the bit's index inside the row.  So aoff alone has to stay below 2^32.  (The 4-CIF ring gathers of the decode
// calls widen every term; they are held to the same rule so that one multiplex decodes by one rule whatever its alignment.)
bool dabgpu_host_ring_fits_lanes(uint64_t n_slots, uint64_t cifs_per_frame, uint64_t frame_stride, uint64_t cif_stride) {
    if (n_slots == 0 || cifs_per_frame == 0) return false;
    uint64_t top, cif;
    if (__builtin_mul_overflow((n_slots - 1) / cifs_per_frame, frame_stride, &top)) return false;
    if (__builtin_mul_overflow(cifs_per_frame - 1, cif_stride, &cif) || __builtin_add_overflow(top, cif, &top)) return false;
    if (__builtin_add_overflow(top, 15 * (cif_stride >> 4), &top)) return false;
    return top < ((uint64_t)1 << 32);
}

// Which sub-channels go to the lane-per-codeword kernel?  The k longest can be left to viterbi_kernel and the rest given to vit_lanes_kernel in
// the same call; AUTO only compares the pure choices k = 0 and k = n_sub -- a partial viterbi_kernel launch is a single lockstep round of
// wavefronts and measured 2x its share of a full one, so hybrids did not pay (hybrid_k forces one, for the tests).  The lane mapping keeps
// ring offsets in 32 bits: one ensemble's ring must stay below 4 GiB.  Fills mapping, model_us, k_wave, n_lane, octet and order[n_sub]
// (sub-channels by descending trellis length).
static void choose_lane_subchannels(dabgpu_decode_plan& p, int hist_frames, const dabgpu_decode_limits& lim, int* order) {
    const int n_sub = p.n_sub;
    uint32_t steps[64];
    for (int j = 0; j < n_sub; j++) { order[j] = j; steps[j] = p.subs[(size_t)j].n_steps; }
    std::sort(order, order + n_sub, [&](int a, int b) { return steps[a] > steps[b]; });
    const int m = dabgpu_host_choose_msc_mapping(lim.forced_mapping, lim.n_simd, p.n_ens, steps, n_sub, p.model_us);
    const bool lanes_allowed = hist_frames > 0 && dabgpu_host_ring_fits_lanes((uint64_t)hist_frames * 4, 4, DABGPU_NB_FRAME_BITS, DABGPU_NB_CIF_BITS) &&
                               lim.forced_mapping != DABGPU_VIT_MAP_WAVE;
    p.mapping = lanes_allowed ? m : DABGPU_VIT_MAP_WAVE;
    p.k_wave = p.mapping == DABGPU_VIT_MAP_WAVE ? n_sub : 0;
    p.octet = p.mapping == DABGPU_VIT_MAP_OCTET;
    if (lanes_allowed && lim.forced_mapping == DABGPU_VIT_MAP_AUTO && lim.hybrid_k >= 0 && lim.hybrid_k <= n_sub) p.k_wave = lim.hybrid_k;
    p.n_lane = n_sub - p.k_wave;
    for (int j = p.k_wave; j < n_sub; j++) p.subs[(size_t)order[j]].lane_mapped = 1;
}

// the lane table (sub-channel, decision rows before it, symbol rows before it) and what follows from it: rows per group quartet (16
// ensembles x 4 CIFs = one group per lane-mapped sub-channel), ensembles per slice, the schedule tables' stride
static void lay_out_lanes(dabgpu_decode_plan& p, const int* order, const dabgpu_decode_limits& lim) {
    p.lane_subs.assign((size_t)3 * p.n_lane, 0);
    for (int j = 0; j < p.n_lane; j++) {
        const int sidx = order[p.k_wave + j];
        const dabgpu_msc_plan& P = p.subs[(size_t)sidx];
        const uint32_t in_rows = dabgpu_vit_in_rows(dabgpu_vit_in_bytes(P.seg_pi, P.seg_steps));
        p.lane_subs[(size_t)3 * j] = (uint64_t)sidx;
        p.lane_subs[(size_t)3 * j + 1] = p.dec_rows_per_gq;
        p.lane_subs[(size_t)3 * j + 2] = p.sym_rows_per_gq;
        p.dec_rows_per_gq += dabgpu_vit_alloc_steps(P.n_steps);
        p.sym_rows_per_gq += in_rows;
        p.lane_max_steps = std::max(p.lane_max_steps, P.n_steps);
        p.lane_max_in_rows = std::max(p.lane_max_in_rows, in_rows);
    }
    if (p.n_lane == 0) return;
    p.ens_per_slice = mul_sat(std::max<size_t>(1, lim.max_dec_rows / p.dec_rows_per_gq), 16);
    p.sched_stride = dabgpu_vit_alloc_steps(p.lane_max_steps);
}

// Where the FIC of the newest frames is decoded.  Inside the lane launch when every sub-channel is lane-mapped and the call is one slice
// with the FIB groups' rows counted in (16 ensembles = 64 FIB groups = one more group of codewords in the launch's scratch): the MSC's
// groups rarely fill the last round of wavefront slots (4096 ensembles x 18 sub-channels = 4608 groups on 5120 slots), so the FIC then costs
// its 20 us gather and nothing else.  In viterbi_kernel's launch when every sub-channel is there and the FIC alone would be too (a handful
// of ensembles: one receiver behind the classes is 4 + 72 codewords, and the two launches used to run one after the other on the stream,
// 109 + 213 us, for work that is independent).  Otherwise first, by the FIC entry point's own path.
static dabgpu_fic_place place_fic(const dabgpu_decode_plan& p, const dabgpu_decode_limits& lim) {
    if (p.k_wave == 0 && p.n_lane > 0 && p.n_cw <= UINT32_MAX &&
        p.n_ens <= mul_sat(std::max<size_t>(1, lim.max_dec_rows / (p.dec_rows_per_gq + p.fic_dec_rows)), 16))
        return DABGPU_FIC_IN_LANES;
    if (p.k_wave == p.n_sub && dabgpu_host_plan_fic(p.n_fic_cw, true, lim).mapping == DABGPU_VIT_MAP_WAVE) return DABGPU_FIC_IN_WAVE;
    return DABGPU_FIC_OWN_LAUNCH;
}

int dabgpu_host_plan_decode(const dabgpu_subchannel* subs, int n_sub, size_t n_ens, int hist_frames, bool want_fic, const dabgpu_decode_limits& lim,
                            dabgpu_decode_plan* out) {
    dabgpu_decode_plan& p = *out;
    p = dabgpu_decode_plan{};
    const int st = dabgpu_host_build_msc_plans(subs, n_sub, p.subs, &p.cif_out_bytes, &p.max_steps, &p.max_out_bytes);
    if (st) return st;
    const dabgpu_uniform_plan fic_group = dabgpu_host_plan_fic(0, true, lim);
    p.n_sub = n_sub; p.n_ens = n_ens;
    p.n_cw = mul_sat(mul_sat(n_ens, 4), (size_t)n_sub);
    p.fic_dec_rows = fic_group.dec_rows; p.fic_in_rows = fic_group.in_rows;
    int order[64];
    choose_lane_subchannels(p, hist_frames, lim, order);
    lay_out_lanes(p, order, lim);
    if (want_fic) {
        p.n_fic_cw = mul_sat(n_ens, 4);
        p.fic = place_fic(p, lim);
    }
    if (p.fic == DABGPU_FIC_IN_WAVE) { p.max_steps = std::max(p.max_steps, DABGPU_FIC_STEPS); p.max_out_bytes = std::max(p.max_out_bytes, DABGPU_FIC_OUT_BYTES); }
    p.descs_bytes = mul_sat(add_sat(p.n_cw, p.n_fic_cw), sizeof(dabgpu_codeword));
    p.plans_bytes = p.subs.size() * sizeof(dabgpu_msc_plan);
    p.lane_subs_bytes = p.lane_subs.size() * sizeof(uint64_t);
    p.sched_bytes = ((size_t)p.n_lane * p.sched_stride + (p.fic == DABGPU_FIC_IN_LANES ? p.fic_dec_rows : 0)) * 2 * sizeof(uint32_t);
    return DABGPU_OK;
}

dabgpu_decode_slice dabgpu_host_decode_slice(const dabgpu_decode_plan& p, size_t e0) {
    dabgpu_decode_slice s = {};
    s.ne = std::min(p.n_ens - e0, p.ens_per_slice);
    s.cw0 = mul_sat(mul_sat(e0, 4), (size_t)p.n_sub);
    s.gps = (uint32_t)((s.ne * 4 + 63) / 64);
    s.n_groups = (size_t)p.n_lane * s.gps;
    s.sym_rows = p.sym_rows_per_gq * s.gps;
    s.dec_rows = p.dec_rows_per_gq * s.gps;
    if (p.fic == DABGPU_FIC_IN_LANES) {         // one slice (e0 = 0): descriptors n_cw .., schedule, symbol and decision areas behind the MSC's
        s.n_fic_groups = (p.n_fic_cw + 63) / 64;
        s.fic_base.first = (uint32_t)p.n_cw;
        s.fic_base.sched_off = (uint64_t)p.n_lane * p.sched_stride;
        s.fic_base.sym_off = (uint64_t)s.sym_rows * 64;
        s.fic_base.dec_off = (uint64_t)s.dec_rows * 128;
        s.sym_rows += s.n_fic_groups * p.fic_in_rows;
        s.dec_rows += s.n_fic_groups * p.fic_dec_rows;
    }
    s.groups_bytes = (s.n_groups + s.n_fic_groups) * sizeof(dabgpu_vit_group);
    return s;
}

extern "C" {
// ---- wav header (host only) ---------------------------------------------------------------------------------------
namespace {
struct byte_cursor {
    const uint8_t* p; size_t n; size_t pos;
    bool take(size_t k, const uint8_t** out) { if (n - pos < k) return false; *out = p + pos; pos += k; return true; }
};
inline uint32_t le32(const uint8_t* b) { return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24); }
inline uint16_t le16(const uint8_t* b) { return (uint16_t)(b[0] | (b[1] << 8)); }
static int map_wav_code(uint16_t code, uint16_t* out) {
    switch (code) { case 1: case 3: case 6: case 7: case 0xFFFE: *out = code; return 1; default: return 0; }
}
}  // namespace

int dabgpu_wav_parse_header(const uint8_t* bytes, size_t n_bytes, dabgpu_wav_header* out) {
#define FAIL(...) do { dabgpu_set_error(__VA_ARGS__); return DABGPU_ERR_INVALID_ARG; } while (0)
    if (!bytes || !out) FAIL("wav_parse_header: null argument");
    byte_cursor cur{bytes, n_bytes, 0};
    const uint8_t* b;
    memset(out, 0, sizeof(*out));
    if (!cur.take(12, &b)) FAIL("wav: insufficient bytes while reading RIFF chunk");
    if (memcmp(b, "RIFF", 4) != 0) FAIL("wav: chunk id is not 'RIFF'");
    if (memcmp(b + 8, "WAVE", 4) != 0) FAIL("wav: wave id is not 'WAVE'");
    if (!cur.take(24, &b)) FAIL("wav: insufficient bytes while reading format chunk");
    if (memcmp(b, "fmt ", 4) != 0) FAIL("wav: chunk id is not 'fmt '");
    const uint32_t fmt_size = le32(b + 4);
    if (fmt_size != 16 && fmt_size != 18 && fmt_size != 40) FAIL("wav: invalid format chunk size %u, expected 16, 18 or 40", fmt_size);
    uint16_t code;
    if (!map_wav_code(le16(b + 8), &code)) FAIL("wav: invalid audio format code %04X", le16(b + 8));
    out->total_channels = le16(b + 10);
    if (out->total_channels != 1 && out->total_channels != 2) FAIL("wav: expected mono or stereo but got %u channels", out->total_channels);
    out->samples_per_second = le32(b + 12);
    out->average_bytes_per_second = le32(b + 16);
    out->data_block_align_bytes = le16(b + 20);
    out->bits_per_sample = le16(b + 22);
    if (fmt_size > 16) {
        const size_t ext = fmt_size - 16;
        if (!cur.take(ext, &b)) FAIL("wav: insufficient bytes while reading format chunk extension fields");
        const uint16_t ext_size = le16(b);
        if (ext_size != ext - 2) FAIL("wav: extension field size %u does not match actual size %zu", ext_size, ext - 2);
        if (ext_size == 22) {
            uint16_t sub;
            if (!map_wav_code(le16(b + 8), &sub)) FAIL("wav: invalid audio format code %04X", le16(b + 8));
            if (sub == 0xFFFE) FAIL("wav: extensible format again in sub-format");
            static const uint8_t GUID[14] = {0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71};
            if (memcmp(GUID, b + 10, 14) != 0) FAIL("wav: extensible format guid does not match");
            code = sub;
        }
    }
    if (code != 1) {                                   // fact chunk for non-PCM formats
        if (!cur.take(8, &b)) FAIL("wav: insufficient bytes while reading fact chunk");
        if (memcmp(b, "fact", 4) != 0) FAIL("wav: chunk id is not 'fact'");
        const uint32_t fact_size = le32(b + 4);
        if (fact_size < 4) FAIL("wav: fact chunk smaller than 4 bytes (%u)", fact_size);
        if (!cur.take(fact_size, &b)) FAIL("wav: insufficient bytes while reading fact chunk data");
    }
    for (;;) {
        if (!cur.take(8, &b)) FAIL("wav: insufficient bytes while reading possible data chunk");
        const uint32_t size = le32(b + 4);
        if (memcmp(b, "data", 4) != 0) {
            // the reference fseek()s past the chunk and fails on the next header read when the file ends first
            if (cur.n - cur.pos < size) FAIL("wav: insufficient bytes while reading possible data chunk");
            cur.pos += size;
            continue;
        }
        out->data_chunk_size = size;
        out->data_chunk_offset = cur.pos;
        break;
    }
    out->audio_format = code;
    int f = -1;
    switch (code) {
    case 1:
        switch (out->bits_per_sample) {
        case 8: f = DABGPU_IQ_WAV_PCM8; break;
        case 16: f = DABGPU_IQ_WAV_PCM16; break;
        case 24: f = DABGPU_IQ_WAV_PCM24; break;
        case 32: f = DABGPU_IQ_WAV_PCM32; break;
        default: FAIL("wav: unhandled PCM format with %u bits per sample", out->bits_per_sample);
        }
        break;
    case 3:
        switch (out->bits_per_sample) {
        case 32: f = DABGPU_IQ_WAV_F32; break;
        case 64: f = DABGPU_IQ_WAV_F64; break;
        default: FAIL("wav: unhandled IEEE754 format with %u bits per sample", out->bits_per_sample);
        }
        break;
    case 6:
        if (out->bits_per_sample != 8) FAIL("wav: unhandled G711 A law format with %u bits per sample", out->bits_per_sample);
        f = DABGPU_IQ_WAV_ALAW; break;
    case 7:
        if (out->bits_per_sample != 8) FAIL("wav: unhandled G711 mu law format with %u bits per sample", out->bits_per_sample);
        f = DABGPU_IQ_WAV_MULAW; break;
    default: FAIL("wav: unhandled extensible wav audio format is not supported");
    }
    out->iq_format = f;
    return DABGPU_OK;
#undef FAIL
}

}  // extern "C"

extern "C" int dabgpu_subchannel_validate(const dabgpu_subchannel* sc) {
    if (!sc) { dabgpu_set_error("subchannel_validate: null descriptor"); return DABGPU_ERR_INVALID_ARG; }
    std::vector<dabgpu_msc_plan> one;
    return dabgpu_host_build_msc_plans(sc, 1, one, nullptr, nullptr, nullptr);
}

// ---- channel encoder planner ----
// keep mask of PI over one run of 32 mother bits (8 input bits x 4 generator outputs, bit 4 g + r = output r of input bit g): the
// first cnt[g] outputs of each input bit survive (EN 300 401 table 13, in the order puncture_codes.h:42-67 lists them)
static uint32_t tx_keep_mask(uint32_t pi) {
    static const int order[8] = {0, 4, 2, 6, 1, 5, 3, 7};
    int cnt[8];
    for (int g = 0; g < 8; g++) cnt[g] = 1;
    for (uint32_t e = 0; e < pi; e++) cnt[order[e % 8]]++;
    uint32_t m = 0;
    for (int g = 0; g < 8; g++) m |= ((1u << cnt[g]) - 1u) << (4 * g);
    return m;
}

// schedule of a code word "segments + tail", appended to `sched` unless an equal one is there already; returns its first entry
static uint32_t tx_add_schedule(dabgpu_tx_plan* P, std::vector<std::pair<std::vector<uint32_t>, uint32_t>>& known, const uint32_t* pi,
                                const uint32_t* blocks, uint32_t* kept_bits) {
    std::vector<uint32_t> key;
    uint32_t kept = 12;
    for (int k = 0; k < 4; k++) { key.push_back(blocks[k] ? pi[k] : 0u); key.push_back(blocks[k]); kept += 4u * blocks[k] * (8u + pi[k]); }
    *kept_bits = kept;
    for (const auto& kn : known) if (kn.first == key) return kn.second;
    const uint32_t first = (uint32_t)P->sched.size();
    uint32_t bit = 0;
    for (int k = 0; k < 4; k++)
        for (uint32_t b = 0; b < blocks[k]; b++) { P->sched.push_back({bit, tx_keep_mask(pi[k])}); bit += 4u * (8u + pi[k]); }
    P->sched.push_back({bit, DABGPU_TX_TAIL_KEEP_MASK});
    known.emplace_back(key, first);
    return first;
}

int dabgpu_host_tx_plan(const dabgpu_subchannel* subs, int n_sub, dabgpu_tx_plan* P) {
    *P = dabgpu_tx_plan{};
    if (n_sub < 0 || n_sub > 64 || (n_sub > 0 && !subs)) { dabgpu_set_error("tx_encode_plan: %d sub-channels (0..64 are accepted)", n_sub); return DABGPU_ERR_INVALID_ARG; }
    std::vector<std::pair<std::vector<uint32_t>, uint32_t>> known;
    unsigned char used[864];
    memset(used, 0, sizeof(used));
    P->subs.assign((size_t)n_sub + 1, dabgpu_tx_sub_plan{});
    for (int s = 0; s < n_sub; s++) {
        const dabgpu_subchannel& sc = subs[s];
        int pi[4], lx[4], nb = 0;
        // (ranges first: start + length of a hostile descriptor overflows int)
        if (sc.length <= 0 || sc.length > 864 || sc.start_address < 0 || sc.start_address > 864 - sc.length) {
            dabgpu_set_error("tx_encode_plan: sub-channel %d lies outside the 864 capacity units", s); return DABGPU_ERR_INVALID_ARG;
        }
        if (dabgpu_subchannel_plan(&sc, pi, lx, &nb) < 0) { dabgpu_set_error("tx_encode_plan: sub-channel %d has an invalid protection profile", s); return DABGPU_ERR_INVALID_ARG; }
        for (int cu = sc.start_address; cu < sc.start_address + sc.length; cu++) {
            if (used[cu]) { dabgpu_set_error("tx_encode_plan: sub-channel %d overlaps another at capacity unit %d", s, cu); return DABGPU_ERR_INVALID_ARG; }
            used[cu] = 1;
        }
        dabgpu_tx_sub_plan& D = P->subs[(size_t)s];
        D.start_address = (uint32_t)sc.start_address; D.length = (uint32_t)sc.length;
        for (int k = 0; k < 4; k++) { D.seg_blocks[k] = (uint32_t)lx[k]; D.seg_pi[k] = lx[k] ? (uint32_t)pi[k] : 0u; D.n_words += (uint32_t)lx[k]; }
        if (D.n_words == 0) { dabgpu_set_error("tx_encode_plan: sub-channel %d carries no data", s); return DABGPU_ERR_INVALID_ARG; }
        D.sched_offset = tx_add_schedule(P, known, D.seg_pi, D.seg_blocks, &D.kept_bits);
        if (D.kept_bits > D.length * 64u) {
            dabgpu_set_error("tx_encode_plan: sub-channel %d: its code word has %u bits, %u capacity units hold %u", s, D.kept_bits, D.length, D.length * 64u);
            return DABGPU_ERR_INVALID_ARG;
        }
        D.in_offset = P->cif_in_bytes; D.in_bytes = (uint32_t)nb;
        P->cif_in_bytes += (uint32_t)nb;
        // ring slot: 16 class rows of ceil(length / 8) dwords (4 bits per capacity unit and class)
        D.ring_offset = P->ring_slot_dwords; D.ring_row_dwords = (D.length + 7u) / 8u;
        P->ring_slot_dwords += 16u * D.ring_row_dwords;
        P->max_length = std::max(P->max_length, D.length);
    }
    dabgpu_tx_sub_plan& F = P->subs[(size_t)n_sub];
    const uint32_t fpi[4] = DABGPU_FIC_SEG_PI, fsteps[4] = DABGPU_FIC_SEG_STEPS;
    F.length = DABGPU_NB_FIB_GROUP_BITS / 64; F.in_bytes = DABGPU_FIC_OUT_BYTES;
    for (int k = 0; k < 4; k++) { F.seg_pi[k] = fpi[k]; F.seg_blocks[k] = fsteps[k] / 32u; F.n_words += F.seg_blocks[k]; }
    F.sched_offset = tx_add_schedule(P, known, F.seg_pi, F.seg_blocks, &F.kept_bits);
    for (int cu = 0; cu < 864;) {
        if (used[cu]) { cu++; continue; }
        int e = cu;
        while (e < 864 && !used[e]) e++;
        P->gaps.push_back((uint32_t)cu); P->gaps.push_back((uint32_t)(e - cu));
        cu = e;
    }
    return DABGPU_OK;
}

extern "C" int dabgpu_tx_encode_plan(const dabgpu_subchannel* subs, int n_sub, dabgpu_tx_sub_plan* plans, uint32_t* cif_in_bytes,
                                     dabgpu_tx_sched_entry* sched, size_t sched_capacity, size_t* n_sched, uint32_t* ring_slot_dwords) {
    dabgpu_tx_plan P;
    const int st = dabgpu_host_tx_plan(subs, n_sub, &P);
    if (st) return st;
    if (plans) memcpy(plans, P.subs.data(), P.subs.size() * sizeof(dabgpu_tx_sub_plan));
    if (cif_in_bytes) *cif_in_bytes = P.cif_in_bytes;
    if (n_sched) *n_sched = P.sched.size();
    if (ring_slot_dwords) *ring_slot_dwords = P.ring_slot_dwords;
    if (sched && sched_capacity >= P.sched.size()) memcpy(sched, P.sched.data(), P.sched.size() * sizeof(dabgpu_tx_sched_entry));
    return DABGPU_OK;
}

// ---- channel BER planner ----
int dabgpu_host_ber_plan(const dabgpu_subchannel* subs, int n_sub, size_t n_ens, int hist_frames, size_t ens_stride, size_t out_ens_stride,
                         int bits_layout, dabgpu_ber_launch* L) {
    *L = dabgpu_ber_launch{};
    if (n_sub < 0 || n_sub > 64 || (n_sub > 0 && !subs)) { dabgpu_set_error("ber_plan: %d sub-channels (0..64 are accepted)", n_sub); return DABGPU_ERR_INVALID_ARG; }
    int st;
    for (int s = 0; s < n_sub; s++)
        if ((st = dabgpu_subchannel_validate(&subs[s]))) return st;
    if ((st = dabgpu_host_tx_plan(subs, n_sub, &L->tx))) return st;
    if (n_ens == 0 || n_ens > (size_t)(1 << 20)) { dabgpu_set_error("ber_plan: %zu ensembles (1..1048576 are accepted)", n_ens); return DABGPU_ERR_INVALID_ARG; }
    if (bits_layout != DABGPU_BITS_NATURAL && bits_layout != DABGPU_BITS_MSC_CLASSED) {
        dabgpu_set_error("ber_plan: unknown bits_layout %d", bits_layout); return DABGPU_ERR_INVALID_ARG;
    }
    if (hist_frames < 5) { dabgpu_set_error("ber_plan: history_frames %d (>= 5: 16 CIFs of delay + the 4 new ones)", hist_frames); return DABGPU_ERR_INVALID_ARG; }
    if (ens_stride / DABGPU_NB_FRAME_BITS < (size_t)hist_frames || (ens_stride & 15)) {
        dabgpu_set_error("ber_plan: ensemble_stride %zu must be a multiple of 16 >= %d x 230400", ens_stride, hist_frames); return DABGPU_ERR_INVALID_ARG;
    }
    const dabgpu_tx_plan& P = L->tx;
    if (n_sub > 0 && (out_ens_stride < (size_t)4 * P.cif_in_bytes || (out_ens_stride & 3))) {
        dabgpu_set_error("ber_plan: out_ensemble_stride %zu must be a multiple of 4 >= 4 x %u", out_ens_stride, P.cif_in_bytes); return DABGPU_ERR_INVALID_ARG;
    }
    dabgpu_ber_geometry& G = L->geo;
    G.n_sub = (uint32_t)n_sub;
    G.codewords_per_ensemble = 4u * (uint32_t)n_sub + 4u;
    G.cif_bytes = P.cif_in_bytes;
    G.n_sched = (uint32_t)P.sched.size();
    uint32_t max_length = 0;
    for (size_t s = 0; s < P.subs.size(); s++) {
        G.sched_offset[s] = P.subs[s].sched_offset;
        G.max_kept_bits = std::max(G.max_kept_bits, P.subs[s].kept_bits);
        max_length = std::max(max_length, P.subs[s].length);
    }
    G.lds_bytes = 4u * dabgpu_ber_cw_dwords(max_length);
    G.waves_per_block = DABGPU_BER_WAVES; G.block_threads = 64u * DABGPU_BER_WAVES;
    G.grid = (uint32_t)((n_ens * G.codewords_per_ensemble + DABGPU_BER_WAVES - 1u) / DABGPU_BER_WAVES);      // <= 2^20 x 260 / 4
    return DABGPU_OK;
}

extern "C" int dabgpu_ber_plan(const dabgpu_subchannel* subs, int n_sub, size_t n_ens, int hist_frames, size_t ens_stride, size_t out_ens_stride,
                               int bits_layout, dabgpu_ber_geometry* out) {
    if (!out) { dabgpu_set_error("ber_plan: null result"); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_ber_launch L;
    const int st = dabgpu_host_ber_plan(subs, n_sub, n_ens, hist_frames, ens_stride, out_ens_stride, bits_layout, &L);
    if (st) return st;
    *out = L.geo;
    return DABGPU_OK;
}

extern "C" int dabgpu_dabplus_superframe_layout(uint32_t frame_bytes, uint8_t descriptor, const uint16_t* au_len, uint16_t* au_start, int* num_aus,
                                                uint32_t* n_rs) {
    if (!au_len) return -1;
    uint32_t start[7], nrs;
    int na;
    const int st = dabgpu_dabplus_layout(frame_bytes, descriptor, au_len, start, &na, &nrs);
    if (num_aus) *num_aus = na;
    if (n_rs) *n_rs = nrs;
    if (st == 0 && au_start) for (int i = 0; i < 7; i++) au_start[i] = (uint16_t)start[i];       // <= 110 x 64 = 7040
    return st;
}

// ---- packet mode, transmit direction (include/dabgpu.h, "MSC packet mode"; arithmetic in packet_fec_core.h) ----
namespace {
struct PacketLayoutState {
    size_t n_entries;
    uint32_t t, used, ci;            // FEC frame, bytes of its application table filled, continuity index of the next data packet
};
}
extern "C" int dabgpu_packet_tx_layout(const uint32_t* group_len, size_t n_groups, uint32_t address, uint32_t packet_length, uint32_t frame_bytes,
                                       uint64_t start_byte, uint32_t continuity_index, int n_fec_frames, dabgpu_packet_tx_entry* table,
                                       size_t max_entries, uint32_t* frame_first, size_t* groups_consumed, uint64_t* end_start_byte,
                                       uint32_t* end_continuity_index) {
    using namespace dabgpu::pkt;
    if (groups_consumed) *groups_consumed = 0;
    if (address < 1 || address > (uint32_t)MAX_ADDRESS) return DABGPU_PACKET_TX_BAD_ADDRESS;
    if (!length_valid((int)packet_length) || packet_length > 96u) return DABGPU_PACKET_TX_BAD_LENGTH;
    if (frame_bytes == 0 || frame_bytes % 24u) return DABGPU_PACKET_TX_BAD_FRAME_BYTES;
    if (frame_bytes < packet_length) return DABGPU_PACKET_TX_FRAME_TOO_SMALL;
    if (n_groups && !group_len) return -1;
    for (size_t g = 0; g < n_groups; g++) if (group_len[g] > (uint32_t)MAX_GROUP_BYTES) return DABGPU_PACKET_TX_BAD_GROUP;
    if (start_byte % 24u) return DABGPU_PACKET_TX_BAD_START;
    if (n_fec_frames < 0 || n_fec_frames > (1 << 20) || !table || !frame_first) return -1;
    if (max_entries < (size_t)MAX_FRAME_PACKETS * (size_t)n_fec_frames) return -1;
    const uint32_t K = (uint32_t)n_fec_frames, L = packet_length, room = L - 5;
    PacketLayoutState S{0, 0, 0, continuity_index & 3u};
    if (K) frame_first[0] = 0;
    // one packet of `len` bytes at the current position; a full table closes its FEC frame
    auto place = [&](int32_t group, uint32_t offset, uint32_t len, uint32_t useful, uint32_t flags, uint32_t ci) {
        dabgpu_packet_tx_entry& e = table[S.n_entries++];
        e.group = group; e.offset = offset; e.position = S.t * (uint32_t)RING_BYTES + S.used;
        e.length = (uint8_t)len; e.useful = (uint8_t)useful; e.flags = (uint8_t)flags; e.continuity_index = (uint8_t)ci;
        S.used += len;
        if (S.used == (uint32_t)APP_TABLE_BYTES) { S.t++; S.used = 0; frame_first[S.t] = (uint32_t)S.n_entries; }
    };
    auto fits = [&](uint32_t len) {
        const uint64_t at = start_byte + (uint64_t)S.t * RING_BYTES + S.used;
        return S.used + len <= (uint32_t)APP_TABLE_BYTES && at % frame_bytes + len <= frame_bytes;
    };
    size_t g = 0;
    for (; g < n_groups && S.t < K; g++) {
        const PacketLayoutState before = S;
        uint32_t done = 0;
        bool first = true, whole = false;
        while (S.t < K) {
            if (!fits(L)) { place(-1, 0, 24, 0, 0, 0); continue; }
            const uint32_t left = group_len[g] - done, take = std::min(left, room);
            const bool last = (take == left);
            place((int32_t)g, done, L, take, (first ? 2u : 0u) | (last ? 1u : 0u), S.ci);
            S.ci = (S.ci + 1) & 3u;
            done += take;
            first = false;
            if (last) { whole = true; break; }
        }
        if (!whole) {                                       // the group does not end inside this call: it is not begun
            S = before;
            break;
        }
    }
    while (S.t < K) place(-1, 0, 24, 0, 0, 0);
    if (groups_consumed) *groups_consumed = g;
    if (end_start_byte) *end_start_byte = start_byte + (uint64_t)K * RING_BYTES;
    if (end_continuity_index) *end_continuity_index = S.ci;
    return 0;
}

// ---- channel model (include/dabgpu.h, "Channel model") ----
int dabgpu_host_channel_plan(const dabgpu_channel_stream* params, size_t n_streams, dabgpu_channel_geometry* out) {
    if (out) *out = dabgpu_channel_geometry{0, DABGPU_CHANNEL_BLOCK, 0, 0};
    if (n_streams == 0 || n_streams > (size_t)(1 << 20)) { dabgpu_set_error("channel_plan: %zu streams (1..1048576 are accepted)", n_streams); return DABGPU_ERR_INVALID_ARG; }
    if (!params) { dabgpu_set_error("channel_plan: null parameters"); return DABGPU_ERR_INVALID_ARG; }
    uint32_t halo = 0, staged = 0;
    for (size_t s = 0; s < n_streams; s++) {
        const dabgpu_channel_stream& P = params[s];
        if (P.n_taps < 1 || P.n_taps > DABGPU_CHANNEL_MAX_TAPS) {
            dabgpu_set_error("channel_plan: stream %zu: %d taps (1..%d are accepted)", s, P.n_taps, DABGPU_CHANNEL_MAX_TAPS); return DABGPU_ERR_INVALID_ARG;
        }
        if (!std::isfinite(P.gain)) { dabgpu_set_error("channel_plan: stream %zu: gain is not finite", s); return DABGPU_ERR_INVALID_ARG; }
        if (!std::isfinite(P.noise_sigma)) { dabgpu_set_error("channel_plan: stream %zu: noise_sigma is not finite", s); return DABGPU_ERR_INVALID_ARG; }
        if (P.noise_sigma < 0.0f) { dabgpu_set_error("channel_plan: stream %zu: noise_sigma is negative", s); return DABGPU_ERR_INVALID_ARG; }
        if (P.start > DABGPU_CHANNEL_MAX_POSITION || P.start < -DABGPU_CHANNEL_MAX_POSITION) {
            dabgpu_set_error("channel_plan: stream %zu: start outside +-2^62", s); return DABGPU_ERR_INVALID_ARG;
        }
        for (int k = 0; k < P.n_taps; k++) {
            if (P.tap_delay[k] < 0 || P.tap_delay[k] > DABGPU_CHANNEL_MAX_DELAY) {
                dabgpu_set_error("channel_plan: stream %zu: tap %d: delay %d (0..%d are accepted)", s, k, P.tap_delay[k], DABGPU_CHANNEL_MAX_DELAY);
                return DABGPU_ERR_INVALID_ARG;
            }
            if (!std::isfinite(P.tap_re[k]) || !std::isfinite(P.tap_im[k])) {
                dabgpu_set_error("channel_plan: stream %zu: tap %d is not finite", s, k); return DABGPU_ERR_INVALID_ARG;
            }
            halo = std::max(halo, ((uint32_t)P.tap_delay[k] + 1u) & ~1u);
        }
        if (!(P.n_taps == 1 && P.tap_delay[0] == 0)) staged = 1;
    }
    if (out) {
        out->halo = halo; out->staged = staged;
        out->lds_bytes = staged ? (DABGPU_CHANNEL_BLOCK + halo + 2u) * 8u : 0u;
    }
    return DABGPU_OK;
}

int dabgpu_host_channel_check_apply(const char* who, size_t n_streams, const void* in, size_t in_stride_samples, size_t n_in, size_t n_out,
                                    const void* out, int out_format, size_t* out_stride_bytes, float u8_scale, bool device_pointers) {
    if (out_format != DABGPU_IQ_RAW_F32L && out_format != DABGPU_IQ_RAW_U8) {
        dabgpu_set_error("%s: output format %d (DABGPU_IQ_RAW_F32L or DABGPU_IQ_RAW_U8 only)", who, out_format); return DABGPU_ERR_INVALID_ARG;
    }
    if (n_in == 0 || n_in > ((size_t)1 << 40)) { dabgpu_set_error("%s: n_in = %zu (1..2^40 are accepted)", who, n_in); return DABGPU_ERR_INVALID_ARG; }
    if (n_out > ((size_t)1 << 31)) { dabgpu_set_error("%s: n_out = %zu (up to 2^31 per call)", who, n_out); return DABGPU_ERR_INVALID_ARG; }
    if (!in || (n_out > 0 && !out)) { dabgpu_set_error("%s: null input / output", who); return DABGPU_ERR_INVALID_ARG; }
    if (in_stride_samples != 0 && (in_stride_samples < n_in || ((in_stride_samples & 1) && device_pointers))) {
        dabgpu_set_error("%s: in_stride_samples must be 0 (one shared input) or an even count >= n_in", who); return DABGPU_ERR_INVALID_ARG;
    }
    const size_t exact = n_out * (out_format == DABGPU_IQ_RAW_F32L ? 8u : 2u);
    const size_t row = device_pointers ? (exact + 15u) & ~(size_t)15 : exact;
    if (*out_stride_bytes == 0) *out_stride_bytes = row;
    if ((device_pointers && (*out_stride_bytes & 15)) || *out_stride_bytes < row) {
        dabgpu_set_error("%s: out_stride_bytes must be 0 or a multiple of 16 that holds n_out samples", who); return DABGPU_ERR_INVALID_ARG;
    }
    if (device_pointers && (((uintptr_t)in & 15) || ((uintptr_t)out & 15))) { dabgpu_set_error("%s: input and output must be 16-byte aligned", who); return DABGPU_ERR_INVALID_ARG; }
    if (out_format == DABGPU_IQ_RAW_U8 && !std::isfinite(u8_scale)) { dabgpu_set_error("%s: u8_scale is not finite", who); return DABGPU_ERR_INVALID_ARG; }
    const size_t tiles = (n_out + 3 + DABGPU_CHANNEL_BLOCK - 1) / DABGPU_CHANNEL_BLOCK;
    if (tiles * n_streams > 0x7FFFFFFFull) { dabgpu_set_error("%s: n_streams x n_out too large for one call", who); return DABGPU_ERR_INVALID_ARG; }
    return DABGPU_OK;
}

int dabgpu_host_channel_fits(const dabgpu_channel_geometry& created, const dabgpu_channel_geometry& wanted) {
    if (wanted.staged && !created.staged) {
        dabgpu_set_error("channel_bank_set_params: the bank was created for single zero-delay taps; these parameters need the staged kernel "
                         "(create the bank with its widest parameters)");
        return DABGPU_ERR_INVALID_ARG;
    }
    if (wanted.halo > created.halo) {
        dabgpu_set_error("channel_bank_set_params: largest delay needs a halo of %u samples, the bank was created with %u", wanted.halo, created.halo);
        return DABGPU_ERR_INVALID_ARG;
    }
    return DABGPU_OK;
}

extern "C" int dabgpu_channel_plan(const dabgpu_channel_stream* params, size_t n_streams, dabgpu_channel_geometry* out) {
    return dabgpu_host_channel_plan(params, n_streams, out);
}

extern "C" uint64_t dabgpu_channel_freq_q64(double cycles) {
    if (!(cycles >= -0.5 && cycles <= 0.5)) return 0;                       // (NaN included)
    const double scaled = std::nearbyint(std::ldexp(cycles, 64));            // in [-2^63, 2^63], exact scaling
    return scaled < 0.0 ? (uint64_t)(int64_t)scaled : (uint64_t)scaled;     // two's complement: -f and 2^64 - f are one frequency
}

extern "C" double dabgpu_channel_freq_cycles(uint64_t freq_q64) { return std::ldexp((double)(int64_t)freq_q64, -64); }

// ---- channel model, fading taps (include/dabgpu.h, "Channel model, fading taps"; the arithmetic is channel_core.h's, shared with the kernel) ----
#include "channel_core.h"

extern "C" int dabgpu_channel_fading_plan(const dabgpu_channel_stream* params, const dabgpu_channel_fading_spec* specs, size_t n_streams,
                                          dabgpu_channel_fading_stream* out) {
    if (!params || !specs || !out) { dabgpu_set_error("channel_fading_plan: null parameters / specs / result"); return DABGPU_ERR_INVALID_ARG; }
    const int st = dabgpu_host_channel_plan(params, n_streams, nullptr);
    if (st) return st;
    for (size_t s = 0; s < n_streams; s++) {
        const dabgpu_channel_fading_spec& S = specs[s];
        if (!(S.doppler_cycles >= 0.0 && S.doppler_cycles <= DABGPU_FADING_MAX_DOPPLER_CYCLES)) {
            dabgpu_set_error("channel_fading_plan: stream %zu: doppler_cycles %g (0..2^-11 are accepted)", s, S.doppler_cycles); return DABGPU_ERR_INVALID_ARG;
        }
        for (int k = 0; k < params[s].n_taps; k++) {
            if (S.kind[k] != DABGPU_TAP_STATIC && S.kind[k] != DABGPU_TAP_FADING) {
                dabgpu_set_error("channel_fading_plan: stream %zu: tap %d: kind %d (STATIC or FADING)", s, k, S.kind[k]); return DABGPU_ERR_INVALID_ARG;
            }
            if (S.kind[k] == DABGPU_TAP_STATIC) continue;
            if (!std::isfinite(S.rice_k[k]) || S.rice_k[k] < 0.0f) {
                dabgpu_set_error("channel_fading_plan: stream %zu: tap %d: rice_k is negative or not finite", s, k); return DABGPU_ERR_INVALID_ARG;
            }
            if (!(S.los_cos[k] >= -1.0f && S.los_cos[k] <= 1.0f)) {
                dabgpu_set_error("channel_fading_plan: stream %zu: tap %d: los_cos outside [-1, 1] or not finite", s, k); return DABGPU_ERR_INVALID_ARG;
            }
        }
    }
    const double two_pi = 6.283185307179586476925286766559;
    for (size_t s = 0; s < n_streams; s++) {
        const dabgpu_channel_fading_spec& S = specs[s];
        dabgpu_channel_fading_stream& F = out[s];
        memset(&F, 0, sizeof(F));
        for (int k = 0; k < params[s].n_taps; k++) {
            if (S.kind[k] != DABGPU_TAP_FADING) continue;
            dabgpu_channel_fading_tap& T = F.tap[k];
            F.kind[k] = DABGPU_TAP_FADING;
            for (int n = 0; n < DABGPU_FADING_OSC; n++) {
                uint32_t w[4];
                dabgpu::ch_philox4x32_10((uint32_t)S.seed, (uint32_t)(S.seed >> 32), (uint32_t)n, (uint32_t)k, (uint32_t)s, 1u, w);
                const double c = (n < 16) ? std::cos(two_pi * ((double)n + ((double)w[0] + 0.5) * 0x1p-32) / 16.0) : (double)S.los_cos[k];
                T.freq_q64[n] = dabgpu_channel_freq_q64(S.doppler_cycles * c);
                T.phase_q64[n] = ((uint64_t)w[2] << 32) | w[3];
            }
            const double K = (double)S.rice_k[k];
            T.amp_diffuse = (float)std::sqrt(1.0 / (K + 1.0)) * 0.25f;
            T.amp_los = (float)std::sqrt(K / (K + 1.0));
        }
    }
    return DABGPU_OK;
}

extern "C" int dabgpu_channel_fading_gain_host(const dabgpu_channel_fading_stream* row, int tap, uint64_t m0, size_t count, float* out) {
    if (!row || (count > 0 && !out)) { dabgpu_set_error("channel_fading_gain_host: null table / result"); return DABGPU_ERR_INVALID_ARG; }
    if (tap < 0 || tap >= DABGPU_CHANNEL_MAX_TAPS) {
        dabgpu_set_error("channel_fading_gain_host: tap %d (0..%d are accepted)", tap, DABGPU_CHANNEL_MAX_TAPS - 1); return DABGPU_ERR_INVALID_ARG;
    }
    const bool fades = row->kind[tap] == DABGPU_TAP_FADING;
    const dabgpu_channel_fading_tap& T = row->tap[tap];
    uint64_t j = 0;
    dabgpu::chf2 g0 = {1.0f, 0.0f}, g1 = g0;
    for (size_t i = 0; i < count; i++) {
        const uint64_t m = m0 + i;
        dabgpu::chf2 g = {1.0f, 0.0f};
        if (fades) {
            if (i == 0 || (m >> dabgpu::CH_FADE_GRID_SHIFT) != j) {
                j = m >> dabgpu::CH_FADE_GRID_SHIFT;
                g0 = dabgpu::ch_fading_grid_gain(T, j); g1 = dabgpu::ch_fading_grid_gain(T, j + 1);
            }
            g = dabgpu::ch_fading_interp(g0, g1, m);
        }
        out[2 * i] = g.re; out[2 * i + 1] = g.im;
    }
    return DABGPU_OK;
}

extern "C" int dabgpu_channel_profile(const char* name, dabgpu_channel_stream* params, dabgpu_channel_fading_spec* spec) {
    if (!name || !params || !spec) { dabgpu_set_error("channel_profile: null name / parameters / spec"); return DABGPU_ERR_INVALID_ARG; }
    struct Preset { const char* name; int n; double delay_us[6]; int delay_samples[6]; double db[6]; };
    static const Preset presets[3] = {
        {"tu6", 6, {0.0, 0.2, 0.5, 1.6, 2.3, 5.0}, {}, {-3.0, 0.0, -2.0, -6.0, -8.0, -10.0}},
        {"ra6", 6, {0.0, 0.1, 0.2, 0.3, 0.4, 0.5}, {}, {0.0, -4.0, -8.0, -12.0, -16.0, -20.0}},
        {"sfn2", 2, {}, {0, 200}, {0.0, -6.0}},
    };
    for (const Preset& p : presets) {
        if (strcmp(name, p.name) != 0) continue;
        const bool samples = p.delay_samples[p.n - 1] != 0;
        double total = 0.0;
        for (int k = 0; k < p.n; k++) total += std::pow(10.0, p.db[k] / 10.0);
        params->n_taps = p.n;
        for (int k = 0; k < DABGPU_CHANNEL_MAX_TAPS; k++) {
            const bool on = k < p.n;
            params->tap_delay[k] = !on ? 0 : samples ? p.delay_samples[k] : (int32_t)std::lround(p.delay_us[k] * 2.048);
            params->tap_re[k] = on ? (float)std::sqrt(std::pow(10.0, p.db[k] / 10.0) / total) : 0.0f;
            params->tap_im[k] = 0.0f;
            spec->kind[k] = on ? DABGPU_TAP_FADING : DABGPU_TAP_STATIC;
            spec->rice_k[k] = 0.0f;
            spec->los_cos[k] = 0.0f;
        }
        if (&p == &presets[1]) { spec->rice_k[0] = (float)(0.91 / 0.41); spec->los_cos[0] = 0.7f; }
        return DABGPU_OK;
    }
    dabgpu_set_error("channel_profile: unknown profile \"%.32s\" (tu6, ra6, sfn2)", name);
    return DABGPU_ERR_INVALID_ARG;
}

int dabgpu_host_channel_fading_check(const char* who, const dabgpu_channel_stream* params, const dabgpu_channel_fading_stream* tables, size_t n_streams) {
    if (!params || !tables) { dabgpu_set_error("%s: null parameters / fading tables", who); return DABGPU_ERR_INVALID_ARG; }
    for (size_t s = 0; s < n_streams; s++) {
        const int n_taps = std::min(std::max(params[s].n_taps, 0), DABGPU_CHANNEL_MAX_TAPS);
        for (int k = 0; k < n_taps; k++) {
            const int kind = tables[s].kind[k];
            if (kind != DABGPU_TAP_STATIC && kind != DABGPU_TAP_FADING) {
                dabgpu_set_error("%s: stream %zu: tap %d: kind %d (STATIC or FADING)", who, s, k, kind); return DABGPU_ERR_INVALID_ARG;
            }
            if (kind == DABGPU_TAP_FADING && (!std::isfinite(tables[s].tap[k].amp_diffuse) || !std::isfinite(tables[s].tap[k].amp_los))) {
                dabgpu_set_error("%s: stream %zu: tap %d: fading amplitudes are not finite", who, s, k); return DABGPU_ERR_INVALID_ARG;
            }
        }
    }
    return DABGPU_OK;
}

extern "C" int dabgpu_channel_plan_fading(const dabgpu_channel_stream* params, size_t n_streams, dabgpu_channel_geometry* out) {
    dabgpu_channel_geometry g;
    const int st = dabgpu_host_channel_plan(params, n_streams, &g);
    if (out) *out = st ? g : dabgpu_host_channel_fading_geometry(g);
    return st;
}

dabgpu_channel_geometry dabgpu_host_channel_fading_geometry(dabgpu_channel_geometry g) {
    g.staged = 1;
    g.lds_bytes = (DABGPU_CHANNEL_BLOCK + g.halo + 2u) * 8u + (uint32_t)(dabgpu::CH_FADE_MAX_POINTS * DABGPU_CHANNEL_MAX_TAPS * 8);
    return g;
}

// ---- resampler (include/dabgpu.h, "Resampler"; the time arithmetic is resample_core.h's, shared with the kernel) ----
#include "resample_core.h"

namespace {

constexpr double RS_PI = 3.14159265358979323846;
constexpr double RS_BETA = 9.25;

// I0(x) by its series sum_k ((x / 2)^k / k!)^2
double rs_bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// the prototype: sinc(t / M) / M under a Kaiser window of `taps` input samples, zero from the window's edge on
double rs_prototype(double t, double M, double i0_beta) {
    const double u = 2.0 * t / (double)DABGPU_RESAMPLE_TAPS;
    if (!(std::fabs(u) < 1.0)) return 0.0;
    const double win = rs_bessel_i0(RS_BETA * std::sqrt(1.0 - u * u)) / i0_beta;
    const double a = RS_PI * t / M;
    const double sinc = (a == 0.0) ? 1.0 : std::sin(a) / a;
    return sinc / M * win;
}

// worst |sum_j c_j e^(2 pi i f (j - taps / 2 + 1 - frac)) - target| over n_f frequencies in [f_lo, f_hi], every phase and three weights
double rs_table_deviation(const float* table, double f_lo, double f_hi, int n_f, double target) {
    constexpr int L = DABGPU_RESAMPLE_PHASES, T = DABGPU_RESAMPLE_TAPS;
    const double weights[3] = {0.0, 0.5, 32767.0 / 32768.0};
    double worst = 0.0;
    for (int fi = 0; fi < n_f; fi++) {
        const double f = f_lo + (f_hi - f_lo) * (double)fi / (double)(n_f - 1);
        const double step_re = std::cos(2.0 * RS_PI * f), step_im = std::sin(2.0 * RS_PI * f);
        for (int wi = 0; wi < 3; wi++) {
            for (int p = 0; p < L; p++) {
                const double frac = ((double)p + weights[wi]) / (double)L;
                const double a0 = 2.0 * RS_PI * f * ((double)(1 - T / 2) - frac);
                double er = std::cos(a0), ei = std::sin(a0), sr = 0.0, si = 0.0;
                const float* h0 = table + (size_t)p * T;
                for (int j = 0; j < T; j++) {
                    const double c = (double)h0[j] + weights[wi] * ((double)h0[T + j] - (double)h0[j]);
                    sr += c * er; si += c * ei;
                    const double nr = er * step_re - ei * step_im;
                    ei = er * step_im + ei * step_re; er = nr;
                }
                worst = std::max(worst, std::hypot(sr - target, si));
            }
        }
    }
    return worst;
}

int rs_check_stream(const char* who, const dabgpu_resample_stream& P, size_t s, uint64_t max_step_q62) {
    if (P.step_q62 < (dabgpu::RS_ONE >> 1) || P.step_q62 > (dabgpu::RS_ONE << 1)) {
        dabgpu_set_error("%s: stream %zu: step %.9g outside [0.5, 2]", who, s, std::ldexp((double)P.step_q62, -62)); return DABGPU_ERR_INVALID_ARG;
    }
    if (P.step_q62 > max_step_q62) {
        dabgpu_set_error("%s: stream %zu: step %.9g above the design's max_step %.9g", who, s, std::ldexp((double)P.step_q62, -62),
                         std::ldexp((double)max_step_q62, -62));
        return DABGPU_ERR_INVALID_ARG;
    }
    if (!std::isfinite(P.gain)) { dabgpu_set_error("%s: stream %zu: gain is not finite", who, s); return DABGPU_ERR_INVALID_ARG; }
    if (P.offset_samples > DABGPU_CHANNEL_MAX_POSITION || P.offset_samples < -DABGPU_CHANNEL_MAX_POSITION) {
        dabgpu_set_error("%s: stream %zu: offset_samples outside +-2^62", who, s); return DABGPU_ERR_INVALID_ARG;
    }
    if (P.offset_frac_q62 >= dabgpu::RS_ONE) { dabgpu_set_error("%s: stream %zu: offset_frac_q62 is 2^62 or more", who, s); return DABGPU_ERR_INVALID_ARG; }
    return DABGPU_OK;
}

}  // namespace

uint64_t dabgpu_host_resample_max_step_q62(double max_step) {
    if (!(max_step >= 0.5 && max_step <= 2.0)) return 0;                    // (NaN included)
    return (uint64_t)std::ceil(std::ldexp(max_step, 62));                   // exact scaling; <= 2^63
}

extern "C" int dabgpu_resample_design(double max_step, double passband_cycles, dabgpu_resample_filter* out) {
    constexpr int L = DABGPU_RESAMPLE_PHASES, T = DABGPU_RESAMPLE_TAPS;
    if (!out) { dabgpu_set_error("resample_design: null result"); return DABGPU_ERR_INVALID_ARG; }
    if (!(max_step >= 0.5 && max_step <= 2.0)) { dabgpu_set_error("resample_design: max_step %g outside [0.5, 2]", max_step); return DABGPU_ERR_INVALID_ARG; }
    if (passband_cycles == 0.0) passband_cycles = DABGPU_RESAMPLE_DEFAULT_PASSBAND;
    if (!(passband_cycles > 0.0 && passband_cycles <= 0.45)) {
        dabgpu_set_error("resample_design: passband %g cycles outside (0, 0.45]", passband_cycles); return DABGPU_ERR_INVALID_ARG;
    }
    const double M = std::max(max_step, 1.0), i0_beta = rs_bessel_i0(RS_BETA);
    for (int p = 0; p < L; p++) {
        double row[T], sum = 0.0;
        for (int j = 0; j < T; j++) { row[j] = rs_prototype((double)p / (double)L + (double)(T / 2 - 1 - j), M, i0_beta); sum += row[j]; }
        for (int j = 0; j < T; j++) out->table[(size_t)p * T + j] = (float)(row[j] / sum);
    }
    out->table[(size_t)L * T] = 0.0f;
    for (int j = 1; j < T; j++) out->table[(size_t)L * T + j] = out->table[j - 1];
    out->max_step = max_step; out->passband_cycles = passband_cycles; out->beta = RS_BETA;
    const double f_pass = passband_cycles / M, f_alias = (1.0 - passband_cycles) / M;
    out->passband_error = rs_table_deviation(out->table, 0.0, f_pass, 65, 1.0);
    out->alias_leakage = (f_alias < 0.5) ? rs_table_deviation(out->table, f_alias, 0.5, 65, 0.0) : 0.0;
    out->error = out->passband_error + out->alias_leakage;
    return DABGPU_OK;
}

int dabgpu_host_resample_plan(const char* who, const dabgpu_resample_stream* params, size_t n_streams, uint64_t max_step_q62,
                              dabgpu_resample_geometry* out) {
    if (out) *out = dabgpu_resample_geometry{DABGPU_RESAMPLE_BLOCK, 0, 0, 0};
    if (n_streams == 0 || n_streams > (size_t)(1 << 20)) { dabgpu_set_error("%s: %zu streams (1..1048576 are accepted)", who, n_streams); return DABGPU_ERR_INVALID_ARG; }
    if (!params) { dabgpu_set_error("%s: null parameters", who); return DABGPU_ERR_INVALID_ARG; }
    if (max_step_q62 == 0) { dabgpu_set_error("%s: the design's max_step is outside [0.5, 2]", who); return DABGPU_ERR_INVALID_ARG; }
    uint64_t step = 0;
    uint32_t rows = 0;
    for (size_t s = 0; s < n_streams; s++) {
        const int st = rs_check_stream(who, params[s], s, max_step_q62);
        if (st) return st;
        step = std::max(step, params[s].step_q62);
        if (!dabgpu::rs_identity(params[s])) rows = std::max(rows, dabgpu::rs_rows_needed(params[s]));
    }
    if (out) {
        out->window_samples = (uint32_t)((step + (((uint64_t)1 << 52) - 1)) >> 52) + DABGPU_RESAMPLE_TAPS + 2u;       // ceil(1024 step) + taps + 2
        out->table_rows = rows;
        out->lds_bytes = ((out->window_samples + 1u) & ~1u) * 8u + rows * (DABGPU_RESAMPLE_TAPS + 1u) * 4u;
    }
    return DABGPU_OK;
}

int dabgpu_host_resample_fits(const dabgpu_resample_geometry& created, const dabgpu_resample_geometry& wanted) {
    if (wanted.window_samples > created.window_samples) {
        dabgpu_set_error("resample_bank_set_params: largest step needs a window of %u samples, the bank was created with %u", wanted.window_samples,
                         created.window_samples);
        return DABGPU_ERR_INVALID_ARG;
    }
    if (wanted.table_rows > created.table_rows) {
        dabgpu_set_error("resample_bank_set_params: these steps touch %u table rows per block, the bank was created for %u (create the bank with "
                         "its widest parameters)", wanted.table_rows, created.table_rows);
        return DABGPU_ERR_INVALID_ARG;
    }
    return DABGPU_OK;
}

extern "C" int dabgpu_resample_plan(const dabgpu_resample_stream* params, size_t n_streams, const dabgpu_resample_filter* design,
                                    dabgpu_resample_geometry* out) {
    if (out) *out = dabgpu_resample_geometry{DABGPU_RESAMPLE_BLOCK, 0, 0, 0};
    if (!design) { dabgpu_set_error("resample_plan: null design"); return DABGPU_ERR_INVALID_ARG; }
    return dabgpu_host_resample_plan("resample_plan", params, n_streams, dabgpu_host_resample_max_step_q62(design->max_step), out);
}

extern "C" uint64_t dabgpu_resample_step_q62(double in_rate_hz, double out_rate_hz, double ppm) {
    if (!(in_rate_hz > 0.0) || !(out_rate_hz > 0.0) || !std::isfinite(ppm)) return 0;
    const double step = in_rate_hz / out_rate_hz * (1.0 + ppm * 1e-6);
    if (!(step > 0.0 && step < 4.0)) return 0;
    return (uint64_t)std::nearbyint(std::ldexp(step, 62));                  // exact scaling, below 2^64
}

extern "C" double dabgpu_resample_step(uint64_t step_q62) { return std::ldexp((double)step_q62, -62); }

extern "C" int dabgpu_resample_input_needed(const dabgpu_resample_stream* params, uint64_t position, size_t n_out, int64_t* first, uint64_t* count) {
    if (!params || !first || !count) { dabgpu_set_error("resample_input_needed: null parameters / result"); return DABGPU_ERR_INVALID_ARG; }
    const int st = rs_check_stream("resample_input_needed", *params, 0, dabgpu::RS_ONE << 1);
    if (st) return st;
    if (position > (uint64_t)DABGPU_CHANNEL_MAX_POSITION || n_out > ((size_t)1 << 31)) {
        dabgpu_set_error("resample_input_needed: position above 2^62 or more than 2^31 samples"); return DABGPU_ERR_INVALID_ARG;
    }
    *first = 0; *count = 0;
    if (n_out == 0) return DABGPU_OK;
    const bool ident = dabgpu::rs_identity(*params);
    const uint64_t before = ident ? 0u : (uint64_t)(DABGPU_RESAMPLE_TAPS / 2 - 1), after = ident ? 0u : (uint64_t)(DABGPU_RESAMPLE_TAPS / 2);
    const dabgpu::RsIndex a = dabgpu::rs_before(dabgpu::rs_index(dabgpu::rs_time(*params, position)), before);
    const dabgpu::RsIndex b = dabgpu::rs_after(dabgpu::rs_index(dabgpu::rs_time(*params, position + (n_out - 1))), after);
    if (!b.neg && (b.n >> 63)) { dabgpu_set_error("resample_input_needed: the span ends above 2^63"); return DABGPU_ERR_INVALID_ARG; }
    *first = (int64_t)a.n;
    *count = b.n - a.n + 1;
    return DABGPU_OK;
}

// ---- channeliser (include/dabgpu.h, "Channeliser"; the index arithmetic is channelise_core.h's, shared with the kernels) ----
#include "channelise_core.h"

namespace {

// worst |sum_j h[j] e^(-2 pi i f (j - peak)) - target| over n_f frequencies in [f_lo, f_hi]
double cs_table_deviation(const float* h, int K, int peak, double f_lo, double f_hi, int n_f, double target) {
    double worst = 0.0;
    for (int fi = 0; fi < n_f; fi++) {
        const double f = f_lo + (f_hi - f_lo) * (double)fi / (double)(n_f - 1);
        const double step_re = std::cos(2.0 * RS_PI * f), step_im = -std::sin(2.0 * RS_PI * f), a0 = 2.0 * RS_PI * f * (double)peak;
        double er = std::cos(a0), ei = std::sin(a0), sr = 0.0, si = 0.0;    // e^(-2 pi i f (j - peak)), stepped from j = 0
        for (int j = 0; j < K; j++) {
            sr += (double)h[j] * er; si += (double)h[j] * ei;
            const double nr = er * step_re - ei * step_im;
            ei = er * step_im + ei * step_re; er = nr;
        }
        worst = std::max(worst, std::hypot(sr - target, si));
    }
    return worst;
}

}  // namespace

extern "C" int dabgpu_channeliser_design(int decim, double passband_cycles, double stopband_cycles, dabgpu_channeliser_filter* out) {
    if (!out) { dabgpu_set_error("channeliser_design: null result"); return DABGPU_ERR_INVALID_ARG; }
    if (decim < 1 || decim > DABGPU_CHANNELISER_MAX_DECIM) {
        dabgpu_set_error("channeliser_design: decimation %d (1..%d are accepted)", decim, DABGPU_CHANNELISER_MAX_DECIM); return DABGPU_ERR_INVALID_ARG;
    }
    if (passband_cycles == 0.0) passband_cycles = DABGPU_CHANNELISER_DEFAULT_PASSBAND;
    if (stopband_cycles == 0.0) stopband_cycles = DABGPU_CHANNELISER_DEFAULT_STOPBAND;
    if (!(passband_cycles > 0.0) || !(stopband_cycles > 0.0)) {             // (NaN included)
        dabgpu_set_error("channeliser_design: edges %g / %g cycles: both must be positive numbers", passband_cycles, stopband_cycles);
        return DABGPU_ERR_INVALID_ARG;
    }
    if (!(passband_cycles < stopband_cycles)) {
        dabgpu_set_error("channeliser_design: passband %g and stopband %g cycles leave no transition", passband_cycles, stopband_cycles);
        return DABGPU_ERR_INVALID_ARG;
    }
    if (!(stopband_cycles <= 0.5 * (double)decim)) {
        dabgpu_set_error("channeliser_design: stopband %g cycles per block sample lies beyond what the wideband stream holds (0.5 x %d)", stopband_cycles,
                         decim);
        return DABGPU_ERR_INVALID_ARG;
    }
    const int D = decim, K = dabgpu::cs_taps(D), peak = dabgpu::cs_peak(D);
    const double fc = 0.5 * (passband_cycles + stopband_cycles);
    for (float& v : out->table) v = 0.0f;
    if (D == 1) out->table[0] = 1.0f;
    else {
        double h[DABGPU_CHANNELISER_TAPS_PER_PHASE * DABGPU_CHANNELISER_MAX_DECIM], sum = 0.0;
        const double i0_beta = rs_bessel_i0(RS_BETA);
        for (int j = 0; j < K; j++) {
            const double t = (double)(j - peak), u = 2.0 * t / (double)K;
            double win = 0.0;
            if (std::fabs(u) < 1.0) win = rs_bessel_i0(RS_BETA * std::sqrt(1.0 - u * u)) / i0_beta;
            const double a = RS_PI * 2.0 * fc * t / (double)D;
            h[j] = 2.0 * fc / (double)D * ((a == 0.0) ? 1.0 : std::sin(a) / a) * win;
            sum += h[j];
        }
        for (int j = 0; j < K; j++) out->table[j] = (float)(h[j] / sum);
    }
    out->decim = D; out->taps = K;
    out->passband_cycles = passband_cycles; out->stopband_cycles = stopband_cycles; out->cutoff_cycles = fc; out->beta = RS_BETA;
    if (D == 1) { out->passband_error = out->stopband_level = out->error = 0.0; return DABGPU_OK; }
    const int n_f = 16 * K + 1;
    out->passband_error = cs_table_deviation(out->table, K, peak, 0.0, passband_cycles / (double)D, n_f, 1.0);
    out->stopband_level = cs_table_deviation(out->table, K, peak, stopband_cycles / (double)D, 0.5, n_f, 0.0);
    out->error = out->passband_error + out->stopband_level;
    return DABGPU_OK;
}

int dabgpu_host_channeliser_plan(const char* who, const dabgpu_channeliser_channel* channels, size_t n_channels, size_t n_streams, int64_t start,
                                 int decim, dabgpu_channeliser_geometry* out, uint32_t* first) {
    if (out) *out = dabgpu_channeliser_geometry{};
    if (decim < 1 || decim > DABGPU_CHANNELISER_MAX_DECIM) { dabgpu_set_error("%s: the design's decimation is %d (1..8)", who, decim); return DABGPU_ERR_INVALID_ARG; }
    if (n_streams == 0 || n_streams > (size_t)(1 << 20)) { dabgpu_set_error("%s: %zu streams (1..1048576 are accepted)", who, n_streams); return DABGPU_ERR_INVALID_ARG; }
    if (n_channels == 0 || n_channels > n_streams * DABGPU_CHANNELISER_MAX_CHANNELS) {
        dabgpu_set_error("%s: %zu channels on %zu streams (1..8 per stream are accepted)", who, n_channels, n_streams); return DABGPU_ERR_INVALID_ARG;
    }
    if (!channels) { dabgpu_set_error("%s: null channel list", who); return DABGPU_ERR_INVALID_ARG; }
    if (start > DABGPU_CHANNELISER_MAX_START || start < -DABGPU_CHANNELISER_MAX_START) { dabgpu_set_error("%s: start outside +-2^61", who); return DABGPU_ERR_INVALID_ARG; }
    size_t run = 0;
    for (size_t c = 0; c < n_channels; c++) {
        const dabgpu_channeliser_channel& C = channels[c];
        if (C.stream >= n_streams) { dabgpu_set_error("%s: channel %zu: stream %u of %zu", who, c, C.stream, n_streams); return DABGPU_ERR_INVALID_ARG; }
        if (c > 0 && C.stream < channels[c - 1].stream) {
            dabgpu_set_error("%s: channel %zu: stream %u behind stream %u (the list is sorted by stream)", who, c, C.stream, channels[c - 1].stream);
            return DABGPU_ERR_INVALID_ARG;
        }
        run = (c > 0 && C.stream == channels[c - 1].stream) ? run + 1 : 1;
        if (run > DABGPU_CHANNELISER_MAX_CHANNELS) {
            dabgpu_set_error("%s: channel %zu: more than %d channels on stream %u", who, c, DABGPU_CHANNELISER_MAX_CHANNELS, C.stream); return DABGPU_ERR_INVALID_ARG;
        }
        if (!std::isfinite(C.gain)) { dabgpu_set_error("%s: channel %zu: gain is not finite", who, c); return DABGPU_ERR_INVALID_ARG; }
    }
    if (first) {
        size_t c = 0;
        for (size_t s = 0; s <= n_streams; s++) {
            while (c < n_channels && channels[c].stream < s) c++;
            first[s] = (uint32_t)c;
        }
    }
    if (out) {
        const uint32_t D = (uint32_t)decim, nt = (uint32_t)dabgpu::cs_phase_taps(decim);
        out->decim = D; out->taps = (uint32_t)dabgpu::cs_taps(decim);
        out->split_tile = DABGPU_CHANNELISER_SPLIT_TILE;
        // D = 1 reads the input directly.  Otherwise (tile + 72) block-rate positions of D samples, the raw window and the rotated one, each
        // as 4 D planes of tile / 4 + 18 + 1 samples (channelise.hip)
        out->split_window = (D == 1) ? 0u : (DABGPU_CHANNELISER_SPLIT_TILE + DABGPU_CHANNELISER_TAPS_PER_PHASE) * D;
        out->split_lds_bytes = (D == 1) ? 0u : 2u * 4u * D * ((DABGPU_CHANNELISER_SPLIT_TILE + DABGPU_CHANNELISER_TAPS_PER_PHASE) / 4u + 1u) * 8u;
        out->combine_tile = DABGPU_CHANNELISER_COMBINE_ROWS * D;
        out->combine_window = DABGPU_CHANNELISER_COMBINE_ROWS + nt - 1u;
        out->combine_lds_bytes = ((out->combine_window + 1u) & ~1u) * 8u;
    }
    return DABGPU_OK;
}

int dabgpu_host_channeliser_tiles(const char* who, size_t n_out, uint32_t tile, size_t rows, uint32_t* tiles) {
    const size_t t = (n_out + tile - 1) / tile + 1;                         // (+ 1: a combine call may begin inside a tile)
    if (t * rows > 0x7FFFFFFFull) { dabgpu_set_error("%s: streams x n_out too large for one call", who); return DABGPU_ERR_INVALID_ARG; }
    *tiles = (uint32_t)(t - 1);
    return DABGPU_OK;
}

extern "C" int dabgpu_channeliser_plan(const dabgpu_channeliser_channel* channels, size_t n_channels, size_t n_streams, int64_t start,
                                       const dabgpu_channeliser_filter* design, dabgpu_channeliser_geometry* out) {
    if (out) *out = dabgpu_channeliser_geometry{};
    if (!design) { dabgpu_set_error("channeliser_plan: null design"); return DABGPU_ERR_INVALID_ARG; }
    return dabgpu_host_channeliser_plan("channeliser_plan", channels, n_channels, n_streams, start, design->decim, out, nullptr);
}

extern "C" uint64_t dabgpu_channeliser_freq_q64(double offset_hz, double rate_hz) {
    if (!(rate_hz > 0.0) || !std::isfinite(rate_hz)) return 0;
    return dabgpu_channel_freq_q64(offset_hz / rate_hz);                    // (0 for NaN and outside +-0.5)
}

extern "C" int dabgpu_channeliser_input_needed(int decim, uint64_t position, int64_t start, size_t n_out, int64_t* first, uint64_t* count) {
    if (!first || !count) { dabgpu_set_error("channeliser_input_needed: null result"); return DABGPU_ERR_INVALID_ARG; }
    *first = 0; *count = 0;
    if (decim < 1 || decim > DABGPU_CHANNELISER_MAX_DECIM) { dabgpu_set_error("channeliser_input_needed: decimation %d (1..8)", decim); return DABGPU_ERR_INVALID_ARG; }
    if (position > (uint64_t)DABGPU_CHANNELISER_MAX_POSITION || n_out > ((size_t)1 << 31)) {
        dabgpu_set_error("channeliser_input_needed: position above 2^58 or more than 2^31 samples"); return DABGPU_ERR_INVALID_ARG;
    }
    if (start > DABGPU_CHANNELISER_MAX_START || start < -DABGPU_CHANNELISER_MAX_START) {
        dabgpu_set_error("channeliser_input_needed: start outside +-2^61"); return DABGPU_ERR_INVALID_ARG;
    }
    if (n_out == 0) return DABGPU_OK;
    *first = dabgpu::cs_split_first(decim, position, start);
    *count = (uint64_t)(n_out - 1) * (uint64_t)decim + (uint64_t)dabgpu::cs_taps(decim);
    return DABGPU_OK;
}

extern "C" int dabgpu_channeliser_decim_for(double rate_hz) {
    for (int d = DABGPU_CHANNELISER_MAX_DECIM; d >= 1; d--) if (rate_hz / (double)d >= 2048000.0) return d;
    return 0;                                                                // (NaN included)
}

// ---- interferer (include/dabgpu.h, "Interferer"; the arithmetic is interferer_core.h's, shared with the kernel) ----
#include "interferer_core.h"

namespace {
constexpr double ITF_BETA = 6.2;            // Kaiser: 16 taps per phase and a transition of 0.25 low-rate cycles give about -65 dB
constexpr int ITF_GRID = 8192;              // the figures' frequencies: 0.5 i / ITF_GRID, i = 0 .. ITF_GRID (a 16384-point spectrum's)
}

extern "C" int dabgpu_interferer_design(double width_cycles, dabgpu_interferer_shape* out) {
    if (!out) { dabgpu_set_error("interferer_design: null result"); return DABGPU_ERR_INVALID_ARG; }
    if (!std::isfinite(width_cycles)) { dabgpu_set_error("interferer_design: width_cycles is not finite"); return DABGPU_ERR_INVALID_ARG; }
    if (width_cycles > 1.0 || width_cycles < DABGPU_INTERFERER_MIN_WIDTH) {
        dabgpu_set_error("interferer_design: width_cycles %g (%g..1 are accepted)", width_cycles, DABGPU_INTERFERER_MIN_WIDTH); return DABGPU_ERR_INVALID_ARG;
    }
    int L = DABGPU_INTERFERER_MAX_INTERP;
    while (L > 1 && !(width_cycles * (double)L + DABGPU_INTERFERER_TRANSITION <= 1.0)) L >>= 1;
    const int K = DABGPU_INTERFERER_TAPS * L;
    const double fc = 0.5 * width_cycles;
    const double centre = 0.5 * (double)(K - 1), i0_beta = rs_bessel_i0(ITF_BETA);
    static thread_local double h[DABGPU_INTERFERER_TAPS * DABGPU_INTERFERER_MAX_INTERP];
    double energy = 0.0;
    for (int j = 0; j < K; j++) {
        const double t = (double)j - centre, u = 2.0 * t / (double)K;
        const double win = rs_bessel_i0(ITF_BETA * std::sqrt(1.0 - u * u)) / i0_beta;
        const double a = RS_PI * 2.0 * fc * t;
        h[j] = 2.0 * fc * ((a == 0.0) ? 1.0 : std::sin(a) / a) * win;
        energy += h[j] * h[j];
    }
    const double scale = std::sqrt(0.5 * (double)L / energy);
    for (float& v : out->taps) v = 0.0f;
    for (int j = 0; j < K; j++) out->taps[j] = (float)(h[j] * scale);
    out->interp = L; out->reserved = 0;
    out->width_cycles = width_cycles; out->cutoff_cycles = fc; out->beta = ITF_BETA;
    // the figures, from the float table
    double lo = INFINITY, hi = 0.0;
    for (int r = 0; r < L; r++) {
        double p = 0.0;
        for (int t = 0; t < DABGPU_INTERFERER_TAPS; t++) p += (double)out->taps[r + L * t] * (double)out->taps[r + L * t];
        lo = std::min(lo, p); hi = std::max(hi, p);
    }
    out->phase_ripple = hi / lo;
    const double stop = 0.5 * width_cycles + 0.5 * DABGPU_INTERFERER_TRANSITION / (double)L;
    double total = 0.0, inband = 0.0, worst_stop = 0.0, p0 = 0.0, p_prev = 0.0, half_width = 0.5;
    bool crossed = false;
    for (int i = 0; i <= ITF_GRID; i++) {
        const double f = 0.5 * (double)i / (double)ITF_GRID;
        const double step_re = std::cos(2.0 * RS_PI * f), step_im = -std::sin(2.0 * RS_PI * f);
        double er = 1.0, ei = 0.0, sr = 0.0, si = 0.0;
        for (int j = 0; j < K; j++) {
            sr += (double)out->taps[j] * er; si += (double)out->taps[j] * ei;
            const double nr = er * step_re - ei * step_im;
            ei = er * step_im + ei * step_re; er = nr;
        }
        const double p = sr * sr + si * si, w = (i == 0 || i == ITF_GRID) ? 0.5 : 1.0;
        if (i == 0) p0 = p;
        total += w * p;
        if (f <= 0.5 * width_cycles) inband += w * p;
        if (f >= stop) worst_stop = std::max(worst_stop, p);
        if (!crossed && i > 0 && p < 0.5 * p0) {                            // the first crossing of half the power at 0, interpolated
            crossed = true;
            half_width = (0.5 / (double)ITF_GRID) * ((double)(i - 1) + (p_prev - 0.5 * p0) / (p_prev - p));
        }
        p_prev = p;
    }
    out->width_3db_cycles = 2.0 * half_width;
    out->inband_share = inband / total;
    out->stopband_level = std::sqrt(worst_stop / p0);
    return DABGPU_OK;
}

int dabgpu_host_interferer_plan(const char* who, const dabgpu_interferer_stream* params, size_t n_streams, const dabgpu_interferer_shape* shapes,
                                int n_shapes, dabgpu_interferer_geometry* out) {
    if (out) *out = dabgpu_interferer_geometry{DABGPU_INTERFERER_BLOCK, 0, 0, 0};
    if (n_streams == 0 || n_streams > (size_t)(1 << 20)) { dabgpu_set_error("%s: %zu streams (1..1048576 are accepted)", who, n_streams); return DABGPU_ERR_INVALID_ARG; }
    if (n_shapes < 0 || n_shapes > DABGPU_INTERFERER_MAX_SHAPES) {
        dabgpu_set_error("%s: %d shapes (0..%d are accepted)", who, n_shapes, DABGPU_INTERFERER_MAX_SHAPES); return DABGPU_ERR_INVALID_ARG;
    }
    if (!params || (n_shapes > 0 && !shapes)) { dabgpu_set_error("%s: null parameters / shapes", who); return DABGPU_ERR_INVALID_ARG; }
    uint32_t slot_bytes = 0, band_slots = 0;
    for (int i = 0; i < n_shapes; i++) {
        const int L = shapes[i].interp;
        if (L < 1 || L > DABGPU_INTERFERER_MAX_INTERP || (L & (L - 1))) {
            dabgpu_set_error("%s: shape %d: interp %d (a power of two in 1..%d)", who, i, L, DABGPU_INTERFERER_MAX_INTERP); return DABGPU_ERR_INVALID_ARG;
        }
        for (int j = 0; j < DABGPU_INTERFERER_TAPS * L; j++)
            if (!std::isfinite(shapes[i].taps[j])) { dabgpu_set_error("%s: shape %d: tap %d is not finite", who, i, j); return DABGPU_ERR_INVALID_ARG; }
        slot_bytes = std::max(slot_bytes, dabgpu::itf_slot_bytes(L));
    }
    for (size_t s = 0; s < n_streams; s++) {
        const dabgpu_interferer_stream& P = params[s];
        if (P.n_sources < 0 || P.n_sources > DABGPU_INTERFERER_MAX) {
            dabgpu_set_error("%s: stream %zu: %d sources (0..%d are accepted)", who, s, P.n_sources, DABGPU_INTERFERER_MAX); return DABGPU_ERR_INVALID_ARG;
        }
        uint32_t shaped = 0;
        for (int k = 0; k < P.n_sources; k++) {
            const dabgpu_interferer_source& S = P.source[k];
            if (S.kind == DABGPU_INTERFERER_OFF) continue;
            if (S.kind != DABGPU_INTERFERER_TONE && S.kind != DABGPU_INTERFERER_BAND) {
                dabgpu_set_error("%s: stream %zu: source %d: kind %d (OFF, TONE or BAND)", who, s, k, S.kind); return DABGPU_ERR_INVALID_ARG;
            }
            if (!std::isfinite(S.amp)) { dabgpu_set_error("%s: stream %zu: source %d: amp is not finite", who, s, k); return DABGPU_ERR_INVALID_ARG; }
            if (S.amp < 0.0f) { dabgpu_set_error("%s: stream %zu: source %d: amp is negative", who, s, k); return DABGPU_ERR_INVALID_ARG; }
            if (S.gate_on > S.gate_period) {
                dabgpu_set_error("%s: stream %zu: source %d: gate_on %llu above gate_period %llu", who, s, k, (unsigned long long)S.gate_on,
                                 (unsigned long long)S.gate_period);
                return DABGPU_ERR_INVALID_ARG;
            }
            if (S.gate_offset >= DABGPU_INTERFERER_MAX_POSITION || S.gate_offset <= -DABGPU_INTERFERER_MAX_POSITION) {
                dabgpu_set_error("%s: stream %zu: source %d: gate_offset at or beyond +-2^62", who, s, k); return DABGPU_ERR_INVALID_ARG;
            }
            if (S.kind == DABGPU_INTERFERER_BAND && (S.shape < -1 || S.shape >= n_shapes)) {
                dabgpu_set_error("%s: stream %zu: source %d: shape %d of %d (-1 = white)", who, s, k, S.shape, n_shapes); return DABGPU_ERR_INVALID_ARG;
            }
            if (dabgpu::itf_shaped(S)) shaped++;
        }
        band_slots = std::max(band_slots, shaped);
    }
    if (out) { out->band_slots = band_slots; out->slot_bytes = band_slots ? slot_bytes : 0u; out->lds_bytes = band_slots * slot_bytes; }
    return DABGPU_OK;
}

int dabgpu_host_interferer_fits(const dabgpu_interferer_geometry& created, const dabgpu_interferer_geometry& wanted) {
    if (wanted.band_slots > created.band_slots) {
        dabgpu_set_error("interferer_bank_set_params: %u shaped BAND sources on one stream, the bank was created for %u (create the bank with its "
                         "widest parameters)", wanted.band_slots, created.band_slots);
        return DABGPU_ERR_INVALID_ARG;
    }
    return DABGPU_OK;
}

int dabgpu_host_interferer_check_apply(const char* who, size_t n_streams, const void* in, size_t in_stride_samples, size_t n_out, const void* out,
                                       int out_format, size_t* out_stride_bytes, float u8_scale, bool device_pointers) {
    const bool has_in = in != nullptr;                                      // (NULL: the interferer alone, the stride is not read)
    if (out_format != DABGPU_IQ_RAW_F32L && out_format != DABGPU_IQ_RAW_U8) {
        dabgpu_set_error("%s: output format %d (DABGPU_IQ_RAW_F32L or DABGPU_IQ_RAW_U8 only)", who, out_format); return DABGPU_ERR_INVALID_ARG;
    }
    if (n_out > ((size_t)1 << 31)) { dabgpu_set_error("%s: n_out = %zu (up to 2^31 per call)", who, n_out); return DABGPU_ERR_INVALID_ARG; }
    if (n_out > 0 && !out) { dabgpu_set_error("%s: null output", who); return DABGPU_ERR_INVALID_ARG; }
    if (has_in && in_stride_samples != 0 && (in_stride_samples < n_out || ((in_stride_samples & 1) && device_pointers))) {
        dabgpu_set_error("%s: in_stride_samples must be 0 (one shared input) or an even count >= n_out", who); return DABGPU_ERR_INVALID_ARG;
    }
    const size_t exact = n_out * (out_format == DABGPU_IQ_RAW_F32L ? 8u : 2u);
    const size_t row = device_pointers ? (exact + 15u) & ~(size_t)15 : exact;
    if (*out_stride_bytes == 0) *out_stride_bytes = row;
    if ((device_pointers && (*out_stride_bytes & 15)) || *out_stride_bytes < row) {
        dabgpu_set_error("%s: out_stride_bytes must be 0 or a multiple of 16 that holds n_out samples", who); return DABGPU_ERR_INVALID_ARG;
    }
    if (device_pointers && ((has_in && ((uintptr_t)in & 15)) || ((uintptr_t)out & 15))) {
        dabgpu_set_error("%s: input and output must be 16-byte aligned", who); return DABGPU_ERR_INVALID_ARG;
    }
    if (has_in && in == out && (out_format != DABGPU_IQ_RAW_F32L || (n_streams > 1 && in_stride_samples * 8u != *out_stride_bytes))) {
        dabgpu_set_error("%s: in place needs complex float output and rows equally far apart", who); return DABGPU_ERR_INVALID_ARG;
    }
    if (out_format == DABGPU_IQ_RAW_U8 && !std::isfinite(u8_scale)) { dabgpu_set_error("%s: u8_scale is not finite", who); return DABGPU_ERR_INVALID_ARG; }
    const size_t tiles = (n_out + 3 + DABGPU_INTERFERER_BLOCK - 1) / DABGPU_INTERFERER_BLOCK;
    if (tiles * n_streams > 0x7FFFFFFFull) { dabgpu_set_error("%s: n_streams x n_out too large for one call", who); return DABGPU_ERR_INVALID_ARG; }
    return DABGPU_OK;
}

extern "C" int dabgpu_interferer_plan(const dabgpu_interferer_stream* params, size_t n_streams, const dabgpu_interferer_shape* shapes, int n_shapes,
                                      dabgpu_interferer_geometry* out) {
    return dabgpu_host_interferer_plan("interferer_plan", params, n_streams, shapes, n_shapes, out);
}

// ---- impulse blanker (include/dabgpu.h, "Impulse blanker"; the arithmetic is blanker_core.h's, shared with the kernel) ----
extern "C" dabgpu_blanker_stream dabgpu_blanker_defaults(void) { return dabgpu_blanker_stream{0, 3.0f, 8, 16, 1, 1, 0}; }

extern "C" size_t dabgpu_blanker_mask_words(size_t n_out) { return n_out / DABGPU_BLANKER_BLOCK + 2; }

int dabgpu_host_blanker_plan(const char* who, const dabgpu_blanker_stream* params, size_t n_streams, dabgpu_blanker_geometry* out) {
    if (out) *out = dabgpu_blanker_geometry{0, DABGPU_BLANKER_BLOCK, 0, 0};
    if (n_streams == 0 || n_streams > (size_t)(1 << 20)) { dabgpu_set_error("%s: %zu streams (1..1048576 are accepted)", who, n_streams); return DABGPU_ERR_INVALID_ARG; }
    if (!params) { dabgpu_set_error("%s: null parameters", who); return DABGPU_ERR_INVALID_ARG; }
    uint32_t reach = 0;
    for (size_t s = 0; s < n_streams; s++) {
        const dabgpu_blanker_stream& P = params[s];
        if (!std::isfinite(P.threshold)) { dabgpu_set_error("%s: stream %zu: threshold is not finite", who, s); return DABGPU_ERR_INVALID_ARG; }
        if (!(P.threshold > 1.0f && P.threshold <= DABGPU_BLANKER_MAX_THRESHOLD)) {
            dabgpu_set_error("%s: stream %zu: threshold %g (above 1, up to 1024)", who, s, (double)P.threshold); return DABGPU_ERR_INVALID_ARG;
        }
        if (P.window < 1 || P.window > DABGPU_BLANKER_MAX_WINDOW) {
            dabgpu_set_error("%s: stream %zu: window %d (1..%d are accepted)", who, s, P.window, DABGPU_BLANKER_MAX_WINDOW); return DABGPU_ERR_INVALID_ARG;
        }
        if (P.gap < 0 || P.gap > DABGPU_BLANKER_MAX_GAP) {
            dabgpu_set_error("%s: stream %zu: gap %d (0..%d are accepted)", who, s, P.gap, DABGPU_BLANKER_MAX_GAP); return DABGPU_ERR_INVALID_ARG;
        }
        if (P.guard < 0 || P.guard > DABGPU_BLANKER_MAX_GUARD) {
            dabgpu_set_error("%s: stream %zu: guard %d (0..%d are accepted)", who, s, P.guard, DABGPU_BLANKER_MAX_GUARD); return DABGPU_ERR_INVALID_ARG;
        }
        if (P.start > DABGPU_BLANKER_MAX_POSITION || P.start < -DABGPU_BLANKER_MAX_POSITION) {
            dabgpu_set_error("%s: stream %zu: start outside +-2^62", who, s); return DABGPU_ERR_INVALID_ARG;
        }
        reach = std::max(reach, (uint32_t)(P.gap + P.window + P.guard));
    }
    if (out) {
        out->reach_blocks = reach;
        out->lds_bytes = (DABGPU_BLANKER_BLOCK / DABGPU_BLANKER_POWER_BLOCK + 2u * reach) * 4u
                         + (DABGPU_BLANKER_BLOCK / DABGPU_BLANKER_POWER_BLOCK + 2u * DABGPU_BLANKER_MAX_GUARD) * 4u;
    }
    return DABGPU_OK;
}

int dabgpu_host_blanker_fits(const dabgpu_blanker_geometry& created, const dabgpu_blanker_geometry& wanted) {
    if (wanted.reach_blocks > created.reach_blocks) {
        dabgpu_set_error("blanker_bank_set_params: gap + window + guard reaches %u blocks, the bank was created for %u (create the bank with its "
                         "widest parameters)", wanted.reach_blocks, created.reach_blocks);
        return DABGPU_ERR_INVALID_ARG;
    }
    return DABGPU_OK;
}

int dabgpu_host_blanker_check_apply(const char* who, size_t n_streams, const void* in, size_t in_stride_samples, size_t n_in, size_t n_out,
                                    const void* out, size_t* out_stride_bytes, const void* mask, size_t* mask_stride_words, bool device_pointers) {
    const int st = dabgpu_host_channel_check_apply(who, n_streams, in, in_stride_samples, n_in, n_out, out, DABGPU_IQ_RAW_F32L, out_stride_bytes, 1.0f,
                                                   device_pointers);
    if (st) return st;
    if (in == out) { dabgpu_set_error("%s: in place is not defined (a tile reads its neighbours' input): d_out must not be d_in", who); return DABGPU_ERR_INVALID_ARG; }
    const size_t words = dabgpu_blanker_mask_words(n_out);
    if (*mask_stride_words == 0) *mask_stride_words = words;
    if (*mask_stride_words < words) {
        dabgpu_set_error("%s: mask_stride_words must be 0 or at least n_out / 1024 + 2 = %zu", who, words); return DABGPU_ERR_INVALID_ARG;
    }
    if (mask && ((uintptr_t)mask & 3)) { dabgpu_set_error("%s: the mask must be 4-byte aligned", who); return DABGPU_ERR_INVALID_ARG; }
    if (words * n_streams > 0x7FFFFFFFull) { dabgpu_set_error("%s: n_streams x n_out too large for one call", who); return DABGPU_ERR_INVALID_ARG; }
    return DABGPU_OK;
}

extern "C" int dabgpu_blanker_plan(const dabgpu_blanker_stream* params, size_t n_streams, dabgpu_blanker_geometry* out) {
    return dabgpu_host_blanker_plan("blanker_plan", params, n_streams, out);
}

extern "C" int dabgpu_blanker_input_needed(const dabgpu_blanker_stream* params, uint64_t position, size_t n_out, int64_t* first, uint64_t* count) {
    if (first) *first = 0;
    if (count) *count = 0;
    if (!first || !count) { dabgpu_set_error("blanker_input_needed: null result"); return DABGPU_ERR_INVALID_ARG; }
    const int st = dabgpu_host_blanker_plan("blanker_input_needed", params, 1, nullptr);
    if (st) return st;
    if (position > (uint64_t)DABGPU_BLANKER_MAX_POSITION) { dabgpu_set_error("blanker_input_needed: position above 2^62"); return DABGPU_ERR_INVALID_ARG; }
    if (n_out > ((size_t)1 << 31)) { dabgpu_set_error("blanker_input_needed: n_out = %zu (up to 2^31 per call)", n_out); return DABGPU_ERR_INVALID_ARG; }
    // position - start reaches 2^63 only where both stand at their caps: the index saturates there (no input is that long)
    auto index = [&](int64_t m) {
        const __int128 i = (__int128)m - (__int128)params->start;
        return i > (__int128)INT64_MAX ? INT64_MAX : (int64_t)i;
    };
    *first = index((int64_t)position);
    if (n_out == 0) return DABGPU_OK;
    if (!params->enabled) { *count = n_out; return DABGPU_OK; }
    const int64_t reach = params->gap + params->window + params->guard;
    const int64_t b0 = (int64_t)(position >> 5) - reach, b1 = (int64_t)((position + n_out - 1) >> 5) + reach;
    *first = index(b0 * DABGPU_BLANKER_POWER_BLOCK);
    *count = (uint64_t)(b1 - b0 + 1) * DABGPU_BLANKER_POWER_BLOCK;
    return DABGPU_OK;
}

// ---- IQ balance (include/dabgpu.h, "IQ balance"; the arithmetic is iqbal_core.h's, shared with the kernels) ----
#include "iqbal_core.h"

extern "C" float dabgpu_iqbal_forget(double time_constant_samples) {
    if (!(time_constant_samples >= (double)DABGPU_IQBAL_TILE)) return 0.0f;                  // (NaN too)
    if (std::isinf(time_constant_samples)) return 1.0f;
    return (float)std::exp(-(double)DABGPU_IQBAL_TILE / time_constant_samples);
}

// TRACK, identity, a memory of 16 mode-I frames, identity until 64 tiles are in (DESIGN.md 4.32 says why)
extern "C" dabgpu_iqbal_stream dabgpu_iqbal_defaults(void) {
    return dabgpu_iqbal_stream{DABGPU_IQBAL_TRACK, 0, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, dabgpu_iqbal_forget(16.0 * 196608.0), 65536.0f};
}

int dabgpu_host_iqbal_plan(const char* who, const dabgpu_iqbal_stream* params, size_t n_streams, size_t max_samples_per_call,
                           dabgpu_iqbal_geometry* out) {
    if (out) *out = dabgpu_iqbal_geometry{DABGPU_IQBAL_TILE, 0, 0};
    if (n_streams == 0 || n_streams > (size_t)(1 << 20)) { dabgpu_set_error("%s: %zu streams (1..1048576 are accepted)", who, n_streams); return DABGPU_ERR_INVALID_ARG; }
    if (!params) { dabgpu_set_error("%s: null parameters", who); return DABGPU_ERR_INVALID_ARG; }
    if (max_samples_per_call < DABGPU_IQBAL_TILE || max_samples_per_call > ((size_t)1 << 31) || (max_samples_per_call & (DABGPU_IQBAL_TILE - 1))) {
        dabgpu_set_error("%s: max_samples_per_call = %zu (a multiple of 1024 in 1024..2^31)", who, max_samples_per_call); return DABGPU_ERR_INVALID_ARG;
    }
    for (size_t s = 0; s < n_streams; s++) {
        const dabgpu_iqbal_stream& P = params[s];
        if (P.mode != DABGPU_IQBAL_OFF && P.mode != DABGPU_IQBAL_FIXED && P.mode != DABGPU_IQBAL_TRACK) {
            dabgpu_set_error("%s: stream %zu: mode %d (OFF 0, FIXED 1, TRACK 2)", who, s, P.mode); return DABGPU_ERR_INVALID_ARG;
        }
        const float k[6] = {P.a_re, P.a_im, P.b_re, P.b_im, P.c_re, P.c_im};
        static const char* const name[6] = {"a_re", "a_im", "b_re", "b_im", "c_re", "c_im"};
        for (int i = 0; i < 6; i++)
            if (!std::isfinite(k[i])) { dabgpu_set_error("%s: stream %zu: %s is not finite", who, s, name[i]); return DABGPU_ERR_INVALID_ARG; }
        if (!(P.forget > 0.0f && P.forget <= 1.0f)) {
            dabgpu_set_error("%s: stream %zu: forget %g (above 0, up to 1)", who, s, (double)P.forget); return DABGPU_ERR_INVALID_ARG;
        }
        if (!(std::isfinite(P.min_weight) && P.min_weight >= (float)DABGPU_IQBAL_TILE)) {
            dabgpu_set_error("%s: stream %zu: min_weight %g (finite, at least 1024)", who, s, (double)P.min_weight); return DABGPU_ERR_INVALID_ARG;
        }
    }
    const uint64_t tiles = max_samples_per_call / DABGPU_IQBAL_TILE;
    if (tiles * n_streams > 0x7FFFFFFFull) { dabgpu_set_error("%s: n_streams x max_samples_per_call too large for one call", who); return DABGPU_ERR_INVALID_ARG; }
    if (out) {
        out->tiles_per_call = (uint32_t)tiles;
        out->scratch_bytes = tiles * n_streams * 32u;
    }
    return DABGPU_OK;
}

int dabgpu_host_iqbal_check_apply(const char* who, size_t n_streams, const dabgpu_iqbal_geometry& geom, const void* in, size_t in_stride_samples,
                                  size_t n, const void* out, int out_format, size_t* out_stride_bytes, float u8_scale, uint32_t flags,
                                  bool device_pointers) {
    if (flags == 0 || (flags & ~(DABGPU_IQBAL_MEASURE | DABGPU_IQBAL_APPLY))) {
        dabgpu_set_error("%s: flags %u (DABGPU_IQBAL_MEASURE, DABGPU_IQBAL_APPLY or both)", who, flags); return DABGPU_ERR_INVALID_ARG;
    }
    const bool apply = (flags & DABGPU_IQBAL_APPLY) != 0;
    if (n == 0) { dabgpu_set_error("%s: n = 0 (1..2^31 are accepted)", who); return DABGPU_ERR_INVALID_ARG; }
    // without APPLY nothing is written: the output's rules are checked against the input, which satisfies them
    size_t no_stride = 0;
    const int st = dabgpu_host_channel_check_apply(who, n_streams, in, in_stride_samples, n, n, apply ? out : in, apply ? out_format : DABGPU_IQ_RAW_F32L,
                                                   apply ? out_stride_bytes : &no_stride, apply ? u8_scale : 1.0f, device_pointers);
    if (st) return st;
    if (apply && in == out && (out_format != DABGPU_IQ_RAW_F32L || (in_stride_samples != 0 && in_stride_samples * 8 != *out_stride_bytes) ||
                               (in_stride_samples == 0 && n_streams > 1))) {
        dabgpu_set_error("%s: in place needs complex float output and rows of the input's stride", who); return DABGPU_ERR_INVALID_ARG;
    }
    if (flags & DABGPU_IQBAL_MEASURE) {
        if (n & (DABGPU_IQBAL_TILE - 1)) { dabgpu_set_error("%s: MEASURE needs n to be a multiple of 1024 (n = %zu)", who, n); return DABGPU_ERR_INVALID_ARG; }
        if (n / DABGPU_IQBAL_TILE > geom.tiles_per_call) {
            dabgpu_set_error("%s: MEASURE of %zu samples, the bank was created for %zu per call", who, n, (size_t)geom.tiles_per_call * DABGPU_IQBAL_TILE);
            return DABGPU_ERR_INVALID_ARG;
        }
    }
    if ((n / DABGPU_IQBAL_TILE + 2) * n_streams > 0x7FFFFFFFull) { dabgpu_set_error("%s: n_streams x n too large for one call", who); return DABGPU_ERR_INVALID_ARG; }
    return DABGPU_OK;
}

extern "C" int dabgpu_iqbal_plan(const dabgpu_iqbal_stream* params, size_t n_streams, size_t max_samples_per_call, dabgpu_iqbal_geometry* out) {
    return dabgpu_host_iqbal_plan("iqbal_plan", params, n_streams, max_samples_per_call, out);
}

extern "C" int dabgpu_iqbal_impairment(double gain_db, double phase_deg, double dc_re, double dc_im, dabgpu_iqbal_stream* out) {
    if (!out) { dabgpu_set_error("iqbal_impairment: null result"); return DABGPU_ERR_INVALID_ARG; }
    *out = dabgpu_iqbal_defaults();
    out->mode = DABGPU_IQBAL_FIXED;
    if (!(std::fabs(gain_db) <= 20.0)) { dabgpu_set_error("iqbal_impairment: gain_db %g (-20..20 are accepted)", gain_db); return DABGPU_ERR_INVALID_ARG; }
    if (!(std::fabs(phase_deg) <= 45.0)) { dabgpu_set_error("iqbal_impairment: phase_deg %g (-45..45 are accepted)", phase_deg); return DABGPU_ERR_INVALID_ARG; }
    if (!std::isfinite(dc_re) || !std::isfinite(dc_im) || !std::isfinite((float)dc_re) || !std::isfinite((float)dc_im)) {
        dabgpu_set_error("iqbal_impairment: the DC term is not finite"); return DABGPU_ERR_INVALID_ARG;
    }
    const double g = std::pow(10.0, gain_db / 20.0), phi = phase_deg * (3.14159265358979323846 / 180.0);
    const double gc = g * std::cos(phi), gs = g * std::sin(phi);
    out->a_re = (float)(0.5 * (1.0 + gc)); out->a_im = (float)(-0.5 * gs);       // K1 = (1 + g e^{-j phi}) / 2
    out->b_re = (float)(0.5 * (1.0 - gc)); out->b_im = (float)(-0.5 * gs);       // K2 = (1 - g e^{+j phi}) / 2
    out->c_re = (float)dc_re; out->c_im = (float)dc_im;
    return DABGPU_OK;
}

extern "C" int dabgpu_iqbal_solve_host(const dabgpu_iqbal_stream* params, dabgpu_iqbal_record* record) {
    if (!params || !record) { dabgpu_set_error("iqbal_solve_host: null parameters / record"); return DABGPU_ERR_INVALID_ARG; }
    const int st = dabgpu_host_iqbal_plan("iqbal_solve_host", params, 1, DABGPU_IQBAL_TILE, nullptr);
    if (st) return st;
    dabgpu::iqb_fold_and_solve(*params, *record, 0, [](int) { return (const float*)nullptr; });
    return DABGPU_OK;
}

// ---- TII (include/dabgpu.h, "TII"; the table and the carrier rule are tii_core.h's, shared with the kernels) ----
#include "tii_core.h"

extern "C" void dabgpu_tii_cfg_default(dabgpu_tii_cfg* cfg) {
    if (!cfg) return;
    cfg->threshold = DABGPU_TII_DEFAULT_THRESHOLD;
    cfg->reserved = 0;
}
extern "C" int dabgpu_tii_pattern(int main_id) { return (main_id < 0 || main_id >= DABGPU_TII_NB_MAIN) ? -1 : (int)dabgpu::tii_pattern(main_id); }
extern "C" int dabgpu_tii_main_id(uint32_t mask) { return dabgpu::tii_main_id(mask); }
extern "C" int dabgpu_tii_carriers(int main_id, int sub_id, int out[32]) {
    if (!out) { dabgpu_set_error("tii_carriers: null output"); return DABGPU_ERR_INVALID_ARG; }
    if (main_id < 0 || main_id >= DABGPU_TII_NB_MAIN) { dabgpu_set_error("tii_carriers: main id %d outside 0..69", main_id); return DABGPU_ERR_INVALID_ARG; }
    if (sub_id < 0 || sub_id >= DABGPU_TII_COMBS) { dabgpu_set_error("tii_carriers: sub id %d outside 0..23", sub_id); return DABGPU_ERR_INVALID_ARG; }
    for (int q = 0; q < 32; q++) { int k0; out[q] = dabgpu::tii_carrier(main_id, sub_id, q, &k0); }
    return DABGPU_OK;
}
extern "C" int dabgpu_tii_validate(const dabgpu_tii_tx* tii, const uint8_t* tii_count, size_t n_frames) {
    if (!tii_count || n_frames == 0) return DABGPU_OK;
    if (!tii) { dabgpu_set_error("tii: counts without a transmitter list"); return DABGPU_ERR_INVALID_ARG; }
    for (size_t f = 0; f < n_frames; f++) {
        if (tii_count[f] > DABGPU_TII_MAX_TX) {
            dabgpu_set_error("tii: frame %zu: %u transmitters (at most %d)", f, (unsigned)tii_count[f], DABGPU_TII_MAX_TX); return DABGPU_ERR_INVALID_ARG;
        }
        for (unsigned i = 0; i < tii_count[f]; i++) {
            const dabgpu_tii_tx& t = tii[f * DABGPU_TII_MAX_TX + i];
            if (t.main_id >= DABGPU_TII_NB_MAIN) {
                dabgpu_set_error("tii: frame %zu: transmitter %u: main id %u outside 0..69", f, i, (unsigned)t.main_id); return DABGPU_ERR_INVALID_ARG;
            }
            if (t.sub_id >= DABGPU_TII_COMBS) {
                dabgpu_set_error("tii: frame %zu: transmitter %u: sub id %u outside 0..23", f, i, (unsigned)t.sub_id); return DABGPU_ERR_INVALID_ARG;
            }
            if (!std::isfinite(t.amp)) { dabgpu_set_error("tii: frame %zu: transmitter %u: amp is not finite", f, i); return DABGPU_ERR_INVALID_ARG; }
        }
    }
    return DABGPU_OK;
}
