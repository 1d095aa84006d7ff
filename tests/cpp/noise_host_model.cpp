// noise_host_model.cpp -- csrc/noise_core.h compiled for the host (tests/noise_model.py builds it with -ffp-contract=off): the fold of a
// float32 spectrum, the floor, the frame power and the record, in the statements the kernel runs.
#include "noise_core.h"

using namespace dabgpu;

extern "C" {

float noise_host_unbias(void) { return NOISE_UNBIAS; }

// spectrum: 2048 complex float -> E[24][8]
void noise_host_fold(const float* spectrum, float* E) {
    float P[TII_FFT];
    for (int k = 0; k < TII_FFT; k++) P[k] = tii_power(spectrum[2 * k], spectrum[2 * k + 1]);
    for (int t = 0; t < TII_ACC; t++) E[t] = tii_fold([&](int bin) { return P[bin]; }, t >> 3, t & 7);
}

float noise_host_floor(const float* E) { return noise_floor(E); }
float noise_host_frame_power(const float* prs_useful) { return sb_frame_power(prs_useful); }
int noise_host_finish(float F, float P, dabgpu_noise_record* out) { return noise_finish(F, P, out) ? 1 : 0; }
float noise_host_reciprocal(float x) { return noise_reciprocal(x); }
float noise_host_scale(float level, float P) { return sb_scale(level, P); }

// every mantissa m in [1, 2) against the correctly rounded 1 / m (the double quotient of two floats, rounded once more, is the correctly
// rounded float quotient: 53 >= 2 * 24 + 2).  Returns the largest distance in units of the result's last place; *n_off: how many differ.
double noise_host_reciprocal_worst(uint32_t* n_off) {
    double worst = 0.0;
    uint32_t off = 0;
    for (uint32_t i = 0; i < (1u << 23); i++) {
        const float m = sb_bits_float(0x3F800000u | i);
        const float r = noise_reciprocal(m), exact = (float)(1.0 / (double)m);
        if (r != exact) {
            off++;
            const int32_t d = (int32_t)sb_float_bits(r) - (int32_t)sb_float_bits(exact);
            const double a = d < 0 ? -(double)d : (double)d;
            if (a > worst) worst = a;
        }
    }
    if (n_off) *n_off = off;
    return worst;
}

}  // extern "C"
