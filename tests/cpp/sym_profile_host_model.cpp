// sym_profile_host_model.cpp -- csrc/sym_profile_core.h compiled for the host (tests/sym_profile_model.py builds it with
// -ffp-contract=off, together with the host half of the library): the row sums, the two figures, the medians and the weights of one
// frame's DQPSK products, and one frame of the symbol-weighted combiner, in the statements the kernels run.
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "sym_profile_core.h"

using namespace dabgpu;

extern "C" {

float sypm_k1536(void) { return SYP_K1536; }
float sypm_rsqrt2(void) { return SYP_RSQRT2; }
float sypm_median(const float* x) { return syp_median(x); }

// dq: [75][1536] complex float -> S1, SD, S2 [75]
void sypm_sums(const float* dq, float* S1, float* SD, float* S2) {
    for (int s = 0; s < SYP_SYMBOLS; s++) syp_row_sums(dq, s, &S1[s], &SD[s], &S2[s]);
}
// S1, SD, S2 [75] -> qa, R [75]
void sypm_figures(const float* S1, const float* SD, const float* S2, float* qa, float* R) {
    for (int s = 0; s < SYP_SYMBOLS; s++) { const syp_row r = syp_row_figures(S1[s], SD[s], S2[s]); qa[s] = r.qa; R[s] = r.R; }
}
// one frame as the device writes it; dq is not read when sync_ok is 0
int sypm_frame(const float* dq, int sync_ok, float* symbol_weight, float* symbol_noise, float* ref_noise) {
    return syp_frame(dq, sync_ok != 0, symbol_weight, symbol_noise, ref_noise) ? 1 : 0;
}

// One frame of the symbol-weighted combiner: npm_combine_frame of tests/cpp/noise_profile_host_model.cpp with sym[b] -> 75 symbol weights
// of branch b or null.  Symbol weights enter neither the live rule nor the scale; band and sym may be null arrays.
int sypm_combine_frame(const float* const* dq, const float* k, const float* w, const int* valid, const float* const* band, const float* const* sym,
                       int n, int classed, int8_t* bits, float* out_k, uint32_t* out_mask) {
    if (n < 1 || n > DV_MAX_BRANCHES) return -1;
    std::vector<int> mapper(1536);
    if (dabgpu_get_carrier_mapper(1, mapper.data())) return -2;
    float wb[DV_MAX_BRANCHES];
    dv_scale_state st = dv_scale_begin();
    for (int b = 0; b < n; b++) {
        wb[b] = (band && band[b]) ? np_branch_weight(band[b]) : (w ? w[b] : 1.0f);
        dv_scale_add(st, b, valid == nullptr || valid[b] != 0, k[b], wb[b]);
    }
    const float kk = dv_scale_end(st);
    const uint32_t mask = st.mask;
    *out_k = kk; *out_mask = mask;
    for (int row = 0; row < 75; row++) {
        for (int i = 0; i < 1536; i++) {
            const int c = mapper[i];                                  // soft bit i of the symbol sits on carrier c
            float re = 0.0f, im = 0.0f;
            bool first = true;
            for (int b = 0; b < n; b++) {
                if (!((mask >> b) & 1u) || kk == 0.0f) continue;      // (an erased frame reads nothing)
                const float* d = dq[b] + 2 * ((size_t)row * 1536 + (size_t)c);
                float wc = (band && band[b]) ? np_clean_weight(band[b][c / NP_BAND_CARRIERS]) : wb[b];
                if (sym && sym[b]) wc = wc * np_clean_weight(sym[b][row]);
                if (first) { re = dv_sum_first(wc, d[0]); im = dv_sum_first(wc, d[1]); first = false; }
                else { re = dv_sum_next(re, wc, d[0]); im = dv_sum_next(im, wc, d[1]); }
            }
            bits[dv_bit_offset(row, i, classed != 0)] = (int8_t)sb_soft_bit(re, kk);
            bits[dv_bit_offset(row, i + 1536, classed != 0)] = (int8_t)sb_soft_bit(-im, kk);
        }
    }
    return 0;
}

}  // extern "C"
