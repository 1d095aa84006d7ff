// tii_host_model.cpp -- csrc/tii_core.h compiled for the host (tests/tii_model.py builds it with -ffp-contract=off): the fold of a
// float32 spectrum and the decision on an accumulator, in the statements the kernel runs.
#include "tii_core.h"

using namespace dabgpu;

extern "C" {

int tii_host_pattern(int p) { return (p < 0 || p >= TII_NB_MAIN) ? -1 : (int)tii_pattern(p); }
int tii_host_main_id(uint32_t mask) { return tii_main_id(mask); }
void tii_host_sort8(const float* v, float* s) { tii_sort8(v, s); }

// spectrum: 2048 complex float -> E[24][8]
void tii_host_fold(const float* spectrum, float* E) {
    float P[TII_FFT];
    for (int k = 0; k < TII_FFT; k++) P[k] = tii_power(spectrum[2 * k], spectrum[2 * k + 1]);
    for (int t = 0; t < TII_ACC; t++) E[t] = tii_fold([&](int bin) { return P[bin]; }, t >> 3, t & 7);
}

// acc[24][8] -> records in ascending sub id; returns their count
int tii_host_decide(const float* acc, float threshold, dabgpu_tii_record* out) {
    float s[TII_COMBS][TII_GROUPS], share[TII_COMBS];
    for (int c = 0; c < TII_COMBS; c++) { tii_sort8(acc + TII_GROUPS * c, s[c]); share[c] = tii_comb_floor(s[c]); }
    const float n = tii_floor(share);
    if (!(n > 0.0f)) return 0;
    const float rn = tii_reciprocal(n);
    int count = 0;
    for (int c = 0; c < TII_COMBS; c++)
        if (tii_comb_decide(c, acc + TII_GROUPS * c, s[c], threshold * n, n, rn, out + count)) count++;
    return count;
}

}  // extern "C"
