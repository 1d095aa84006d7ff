// diversity_core.h -- every arithmetic step of receive diversity (include/dabgpu.h, "Receive diversity"), host and device: the combiner
// kernel (diversity.hip), dabgpu_diversity_scale_host and the host model of the tests (tests/cpp/diversity_host_model.cpp) compile these
// same functions, so the device is checked bit for bit against a CPU run of this file, and this file against an independent numpy model
// (tests/diversity_model.py).  The library's arithmetic contract holds: built with -ffp-contract=off, every fused operation an explicit
// fmaf, no `/` of either compiler (softbit_csi_core.h, channel_core.h say why).  Error bounds: DESIGN.md 4.24.
//
// What is combined.  A DQPSK product d = X_i conj(X_i+1) carries no channel phase: with the channel H of a carrier, d = |H|^2 s + noise,
// s the transmitted phase step.  The products of K receivers of one ensemble therefore add coherently, carrier by carrier, and the
// amplitude |H_b|^2 each of them keeps (the precondition: DABGPU_SOFT_CSI keeps it, the normalised policy divides it away) weighs a
// branch by its own channel state.  With noise of power N_b in branch b the maximal-ratio statistic is sum_b d_b / N_b: the weight
//     w_b = 1 / (noise power of branch b)
// is the maximal-ratio weight, and it does not change under a gain of the branch (a gain g scales d_b by g^2 and N_b by g^2; the
// soft-bit scale below divides the common factor out again).  Receivers with equal noise take weight 1: the plain sum is their
// maximal-ratio statistic.
//
// Scale.  Every branch was demodulated with one level L, k_b = L 1536 / (2048 P_b).  The combined factor
//     k = 1 / sum_live (w_b / k_b)        = L 1536 / (2048 sum w_b P_b)
// puts a component of mean size of the weighted sum at +-L again.
#pragma once
#include <stdint.h>

#include "softbit_csi_core.h"

namespace dabgpu {

constexpr int DV_MAX_BRANCHES = DABGPU_DIVERSITY_MAX_BRANCHES;

// finite and > 0 (false for NaN): what a scale and a weight of a live branch must be
DABGPU_HD inline bool dv_positive_finite(float x) { return x > 0.0f && x <= 3.40282347e+38f; }
// branch b of a frame takes part: its synchroniser accepted the frame (no record: it did), its scale and its weight are usable.  The
// products of a branch that is not live are never read.
DABGPU_HD inline bool dv_branch_live(bool sync_ok, float k, float w) { return sync_ok && dv_positive_finite(k) && dv_positive_finite(w); }

// ---- reciprocal ----
// 1 / x for a NORMAL positive x = m 2^e, m in [1, 2): the Newton iteration of sb_scale -- linear seed (within 1/17), three steps, one
// residual correction of the quotient 1 / m (within 1 ulp of the exact one) -- then the two powers of two, a = e / 2: the first product is
// exact, the second rounds once where the result is below the normal range (e = 127).  x below the normal range has no reciprocal a float
// holds for certain: +infinity, which the caller's test of its sum turns into an erasure.
DABGPU_HD inline float dv_reciprocal(float x) {
    if (!(x >= 1.17549435e-38f)) return sb_bits_float(0x7F800000u);
    const uint32_t b = sb_float_bits(x);
    const int e = (int)(b >> 23) - 127;                                            // -126 .. 127
    const float m = sb_bits_float((b & 0x007FFFFFu) | 0x3F800000u);
    float r = __builtin_fmaf(-0.470588235f, m, 1.41176471f);
    r = __builtin_fmaf(r, __builtin_fmaf(-m, r, 1.0f), r);
    r = __builtin_fmaf(r, __builtin_fmaf(-m, r, 1.0f), r);
    r = __builtin_fmaf(r, __builtin_fmaf(-m, r, 1.0f), r);
    const float q = __builtin_fmaf(__builtin_fmaf(-m, r, 1.0f), r, r);
    const int a = e / 2;
    return (q * sb_bits_float((uint32_t)(127 - a) << 23)) * sb_bits_float((uint32_t)(127 - (e - a)) << 23);
}

// ---- scale of a frame: the branches are offered in branch order ----
struct dv_scale_state {
    float sum;              // sum over the live branches so far of w_b / k_b, fmaf(w_b, 1 / k_b, sum) in branch order
    float k_only;           // scale of the first live branch
    uint32_t mask;          // bit b: branch b is live
    int n_live;
    bool unit;              // every live branch so far has weight exactly 1
};
DABGPU_HD inline dv_scale_state dv_scale_begin() { return dv_scale_state{0.0f, 0.0f, 0u, 0, true}; }
// returns whether the branch is live
DABGPU_HD inline bool dv_scale_add(dv_scale_state& s, int b, bool sync_ok, float k, float w) {
    if (!dv_branch_live(sync_ok, k, w)) return false;
    s.sum = __builtin_fmaf(w, dv_reciprocal(k), s.sum);
    if (s.n_live == 0) s.k_only = k;
    s.unit = s.unit && w == 1.0f;
    s.n_live++;
    s.mask |= 1u << b;
    return true;
}
// k of the frame.  0 -- the frame is erased -- without a live branch, for a sum that is not a normal number, for a result that is not
// finite.  The one exception to the formula: a single live branch of weight exactly 1 keeps its own scale unchanged, so that one branch
// reproduces the weighted soft bits of the demodulator bit for bit.
DABGPU_HD inline float dv_scale_end(const dv_scale_state& s) {
    if (s.n_live == 0) return 0.0f;
    if (s.n_live == 1 && s.unit) return s.k_only;
    if (!(s.sum >= 1.17549435e-38f) || !(s.sum <= 3.40282347e+38f)) return 0.0f;
    const float k = dv_reciprocal(s.sum);
    return (k <= 3.40282347e+38f) ? k : 0.0f;
}
// the whole rule over arrays: w (may be null: weight 1), valid (may be null: every record valid), n in 1 .. DV_MAX_BRANCHES
DABGPU_HD inline float dv_scale(const float* k, const float* w, const int* valid, int n, uint32_t* live_mask) {
    dv_scale_state s = dv_scale_begin();
    for (int b = 0; b < n; b++) dv_scale_add(s, b, valid == nullptr || valid[b] != 0, k[b], w ? w[b] : 1.0f);
    if (live_mask) *live_mask = s.mask;
    return dv_scale_end(s);
}

// ---- sum of the products: one component (re or im) of one carrier, the live branches in branch order ----
// (weight 1 leaves the first term exact; a product that is not finite propagates, and sb_quantise turns a NaN into 0)
DABGPU_HD inline float dv_sum_first(float w, float x) { return w * x; }
DABGPU_HD inline float dv_sum_next(float acc, float w, float x) { return __builtin_fmaf(w, x, acc); }

// ---- where a soft bit goes ----
// carrier c of a data symbol carries soft bit p = inv_map[c] (first bit) and p + 1536 (second bit) of the symbol's 3072.  Natural layout:
// symbol `row` (0 .. 74) starts at row * 3072.  Class order (DABGPU_BITS_MSC_CLASSED): the three FIC symbols as before; bit i of a CIF
// row of 55296 lies at (i mod 16) * 3456 + i / 16 of that row.
DABGPU_HD inline uint32_t dv_bit_offset(int row, int j /* bit of the symbol, 0 .. 3071 */, bool classed) {
    if (!classed || row < 3) return (uint32_t)row * 3072u + (uint32_t)j;
    const uint32_t q = (uint32_t)(row - 3) / 18u, i = ((uint32_t)(row - 3) % 18u) * 3072u + (uint32_t)j;
    return 9216u + q * 55296u + (i & 15u) * 3456u + (i >> 4);
}

}  // namespace dabgpu
