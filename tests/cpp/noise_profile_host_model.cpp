// noise_profile_host_model.cpp -- csrc/noise_profile_core.h compiled for the host (tests/noise_profile_model.py builds it with
// -ffp-contract=off, together with the host half of the library): the carrier powers of a float32 spectrum, bands, smoothing, mean and
// weights, and the banded combiner over one frame, in the statements the kernels run.
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "noise_profile_core.h"

using namespace dabgpu;

extern "C" {

float npm_count_reciprocal(int n) { return np_count_reciprocal(n); }
int npm_carrier_bin(int c) { return np_carrier_bin(c); }
uint32_t npm_band_mask(const uint32_t* exclude, int b) { return np_band_mask(exclude, b); }
float npm_mean128(const float* v) { return np_mean128(v); }
float npm_branch_weight(const float* band_weight) { return np_branch_weight(band_weight); }
float npm_weight(float n, float M) { return np_weight(n, M); }

// spectrum: 2048 complex float -> C[1536] in carrier order
void npm_carrier_powers(const float* spectrum, float* C) {
    for (int c = 0; c < NP_CARRIERS; c++) { const int k = np_carrier_bin(c); C[c] = tii_power(spectrum[2 * k], spectrum[2 * k + 1]); }
}

int npm_frame_bands(const float* C, const uint32_t* exclude, const float* profile_in, float alpha, float* profile_out, float* band_weight,
                    float* mean_noise) {
    return np_frame_bands(C, exclude, profile_in, alpha, profile_out, band_weight, mean_noise) ? 1 : 0;
}

// One frame of the banded combiner: dvm_combine_frame of tests/cpp/diversity_host_model.cpp with band[b] -> 128 band weights of branch
// b or null (then w[b], or 1 without w).  A branch with a table takes its tree mean for its weight; w[b] is not looked at.
int npm_combine_frame(const float* const* dq, const float* k, const float* w, const int* valid, const float* const* band, int n, int classed,
                      int8_t* bits, float* out_k, uint32_t* out_mask) {
    if (n < 1 || n > DV_MAX_BRANCHES) return -1;
    std::vector<int> mapper(1536);
    if (dabgpu_get_carrier_mapper(1, mapper.data())) return -2;
    float wb[DV_MAX_BRANCHES];
    dv_scale_state st = dv_scale_begin();
    for (int b = 0; b < n; b++) {
        wb[b] = band[b] ? np_branch_weight(band[b]) : (w ? w[b] : 1.0f);
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
                const float wc = band[b] ? np_clean_weight(band[b][c / NP_BAND_CARRIERS]) : wb[b];
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
