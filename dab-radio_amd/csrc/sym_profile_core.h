// sym_profile_core.h -- the arithmetic of the symbol noise profile (include/dabgpu.h, "Symbol noise profile"), host and device: the kernel
// (sym_profile.hip), the host form (dabgpu_sym_profile_rows_host) and the host model of the tests (tests/cpp/sym_profile_host_model.cpp)
// compile these same statements, so the device is checked bit for bit against a CPU run of this file, and this file against an
// independent numpy model (tests/sym_profile_model.py).  The library's arithmetic contract holds: -ffp-contract=off, every fused step an
// explicit fmaf, sums in a written order, no `/` at run time (the reciprocal is diversity_core.h's), the correctly rounded square root
// (dd_profile_core.h says why both compilers give it).
//
// What is measured.  The decision-directed profile (dd_profile_core.h) averages a carrier over the frame's 75 products: a wideband burst
// that lasts a symbol or more raises every band alike and its weights stay flat.  Here the sums run the other way, over the 1536 carriers
// of one product row, and give one noise figure per row.  A product d of a carrier with channel power a and noise power q per bin, folded
// into the first quadrant (|re|, |im|), lies about the decision diagonal; its component across the diagonal, (|re| - |im|) / sqrt 2, has
// variance a q + q^2 / 2 whatever a is.  Summed over the carriers with P = S1 / sqrt 2 standing for sum a:
//     768 q^2 + P q - SD / 2 = 0,     qa = (sqrt(P^2 + 1536 SD) - P) / 1536
// in the units of "Noise profile" step 1 (white noise of power s2 per sample reads as 2048 s2).  Where decisions fail the folding hides
// noise and qa saturates; the rms R = sqrt(S2 / 1536) = a + q does not, so a row is also given the median figure plus its excess of R
// over the median R, and takes the larger of the two.  The weights are relative: the median row has weight 1, and so has every row that is
// no noisier.
//
// Order of the sums.  The row's 1536 carriers are dealt to 256 owners: owner t has the carrier pairs t, t + 256, t + 512 (carriers
// 2 p, 2 p + 1).  An owner chains its six carriers in that order from +0: s = s + term.  The 64 owners 64 w .. 64 w + 63 of wave w meet
// in the wavefront tree (a[i] + a[i + h] for i < h, h = 32 .. 1), and the four wave sums join as (p0 + p1) + (p2 + p3).  The order does
// not depend on launch geometry; syp_row_sums below is the definition.
//
// Limits.  Mode I only.  Product s mixes symbols s and s + 1, so a burst's edge weighs on one neighbour row.  A frame of which more than
// half is burst has a jammed reference and weights near 1.  The estimator keeps no state: bursts are not stationary.
#pragma once
#include <stdint.h>

#include "noise_profile_core.h"

namespace dabgpu {

constexpr int SYP_SYMBOLS = 75, SYP_CARRIERS = NP_CARRIERS, SYP_OWNERS = 256, SYP_WAVES = 4, SYP_MEDIAN_RANK = 37;   // the 38th smallest
constexpr float SYP_K1536 = 1.0f / 1536.0f;          // the float nearest 1 / 1536 (a constant of the compiler, correctly rounded)
constexpr float SYP_RSQRT2 = 0.70710678118654752f;   // the float nearest 1 / sqrt(2)
constexpr float SYP_WEIGHT_CAP = 0x1p-20f;           // v_s = q_ref / max(q_s, q_ref 2^-20)
static_assert(SYP_OWNERS * 6 == SYP_CARRIERS && SYP_WAVES * 64 == SYP_OWNERS, "six carriers an owner, four waves of owners");

// step 1: one carrier joins its owner's three chains
struct syp_sums { float s1, sd, s2; };
DABGPU_HD inline void syp_add(syp_sums& a, float re, float im) {
    const float ar = __builtin_fabsf(re), ai = __builtin_fabsf(im), d = ar - ai;
    a.s1 = a.s1 + (ar + ai);
    a.sd = a.sd + d * d;
    a.s2 = a.s2 + __builtin_fmaf(re, re, im * im);
}
DABGPU_HD inline float syp_join(float p0, float p1, float p2, float p3) { return (p0 + p1) + (p2 + p3); }

// steps 2 and 3 of one row from its sums: the quadrature figure qa and the rms R.  A row with a sum that is not finite (or whose
// discriminant is not) has qa = R = +infinity: it ranks last in every median and its weight is 0.
struct syp_row { float qa, R; };
DABGPU_HD inline syp_row syp_row_figures(float S1, float SD, float S2) {
    const float inf = sb_bits_float(0x7F800000u);
    const float P = S1 * SYP_RSQRT2;
    const float disc = __builtin_fmaf(1536.0f, SD, P * P);
    const float m2 = S2 * SYP_K1536;
    if (!(disc <= 3.40282347e+38f) || !(m2 <= 3.40282347e+38f)) return syp_row{inf, inf};      // (false for NaN)
    const float qa = (__builtin_sqrtf(disc) - P) * SYP_K1536;
    return syp_row{qa > 0.0f ? qa : 0.0f, __builtin_sqrtf(m2)};
}
DABGPU_HD inline bool syp_row_bad(float qa) { return !(qa <= 3.40282347e+38f); }

// the median of 75 values by rank counting: the rank of x[s] is the number of values below it, ties broken by row index; the median has
// rank 37.  X(j) -> float, no NaN among the values.
template <class Value>
DABGPU_HD inline int syp_rank(Value X, int s) {
    const float x = X(s);
    int r = 0;
    for (int j = 0; j < SYP_SYMBOLS; j++) {
        const float y = X(j);
        r += (y < x || (y == x && j < s)) ? 1 : 0;
    }
    return r;
}

// step 3: the row's noise figure from the two medians
DABGPU_HD inline float syp_noise(float qa, float R, float med_qa, float med_R) {
    if (syp_row_bad(qa)) return qa;
    const float lifted = med_qa + (R - med_R);
    return lifted > qa ? lifted : qa;                     // (a NaN compares false: qa)
}
// step 4
DABGPU_HD inline bool syp_ref_ok(float q_ref) { return np_mean_ok(q_ref); }
DABGPU_HD inline float syp_weight(float q, float q_ref) {
    if (syp_row_bad(q)) return 0.0f;
    if (q <= q_ref) return 1.0f;
    const float cap = q_ref * SYP_WEIGHT_CAP;
    const float v = q_ref * dv_reciprocal(q > cap ? q : cap);
    return v < 1.0f ? v : 1.0f;
}

// ---- the host forms ----
// the wavefront tree over 64 values (noise_profile_core.h's np_half_tree) of the owners' chains, then the join: the three sums of row s
// of one frame's products dq [75][1536] complex float
inline void syp_row_sums(const float* dq, int s, float* S1, float* SD, float* S2) {
    float part[3][SYP_WAVES];
    const float* const row = dq + 2 * (size_t)s * SYP_CARRIERS;
    for (int w = 0; w < SYP_WAVES; w++) {
        float a1[64], ad[64], a2[64];
        for (int l = 0; l < 64; l++) {
            syp_sums a{0.0f, 0.0f, 0.0f};
            for (int j = 0; j < 3; j++) {
                const int c = 2 * (64 * w + l + SYP_OWNERS * j);
                syp_add(a, row[2 * c], row[2 * c + 1]);
                syp_add(a, row[2 * c + 2], row[2 * c + 3]);
            }
            a1[l] = a.s1; ad[l] = a.sd; a2[l] = a.s2;
        }
        part[0][w] = np_half_tree(a1); part[1][w] = np_half_tree(ad); part[2][w] = np_half_tree(a2);
    }
    *S1 = syp_join(part[0][0], part[0][1], part[0][2], part[0][3]);
    *SD = syp_join(part[1][0], part[1][1], part[1][2], part[1][3]);
    *S2 = syp_join(part[2][0], part[2][1], part[2][2], part[2][3]);
}

inline float syp_median(const float* x) {
    for (int s = 0; s < SYP_SYMBOLS; s++)
        if (syp_rank([&](int j) { return x[j]; }, s) == SYP_MEDIAN_RANK) return x[s];
    return x[0];                                          // (not reached: the ranks are a permutation)
}

// steps 2 to 4 from the 75 rows' sums.  False: the frame is skipped -- weights, noise and reference 0.  Every output may be null.
inline bool syp_frame_rows(const float* S1, const float* SD, const float* S2, float* symbol_weight, float* symbol_noise, float* ref_noise) {
    float qa[SYP_SYMBOLS], R[SYP_SYMBOLS], q[SYP_SYMBOLS];
    for (int s = 0; s < SYP_SYMBOLS; s++) {
        const syp_row r = syp_row_figures(S1[s], SD[s], S2[s]);
        qa[s] = r.qa; R[s] = r.R;
    }
    const float med_qa = syp_median(qa), med_R = syp_median(R);
    for (int s = 0; s < SYP_SYMBOLS; s++) q[s] = syp_noise(qa[s], R[s], med_qa, med_R);
    const float q_ref = syp_median(q);
    const bool ok = syp_ref_ok(q_ref);
    for (int s = 0; s < SYP_SYMBOLS; s++) {
        if (symbol_weight) symbol_weight[s] = ok ? syp_weight(q[s], q_ref) : 0.0f;
        if (symbol_noise) symbol_noise[s] = ok ? q[s] : 0.0f;
    }
    if (ref_noise) *ref_noise = ok ? q_ref : 0.0f;
    return ok;
}

// one whole frame on the host.  sync_ok false: the frame is skipped and dq is not read.
inline bool syp_frame(const float* dq, bool sync_ok, float* symbol_weight, float* symbol_noise, float* ref_noise) {
    float S1[SYP_SYMBOLS], SD[SYP_SYMBOLS], S2[SYP_SYMBOLS];
    if (sync_ok) {
        for (int s = 0; s < SYP_SYMBOLS; s++) syp_row_sums(dq, s, &S1[s], &SD[s], &S2[s]);
        return syp_frame_rows(S1, SD, S2, symbol_weight, symbol_noise, ref_noise);
    }
    for (int s = 0; s < SYP_SYMBOLS; s++) {
        if (symbol_weight) symbol_weight[s] = 0.0f;
        if (symbol_noise) symbol_noise[s] = 0.0f;
    }
    if (ref_noise) *ref_noise = 0.0f;
    return false;
}

}  // namespace dabgpu
