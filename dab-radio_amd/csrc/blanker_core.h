// blanker_core.h -- every arithmetic step of the impulse blanker (include/dabgpu.h, "Impulse blanker"), host and device: the kernel
// (blanker.hip) and the host model of the tests (tests/cpp/blanker_host_model.cpp) compile these same functions, so the device is checked
// bit for bit against a CPU run of this file, and this file against an independent numpy model (tests/blanker_model.py).
// The arithmetic contract is channel_core.h's: -ffp-contract=off, every fused operation an explicit fmaf, no division;
// a float addition is commutative bit for bit, so the tree below may be summed as a butterfly across lanes.  DESIGN.md 4.29.
#pragma once
#include <stdint.h>

#include "channel_core.h"

namespace dabgpu {

constexpr int BLK_SHIFT = 5;                          // log2 of DABGPU_BLANKER_POWER_BLOCK
constexpr int BLK_LEN = 1 << BLK_SHIFT;
static_assert(BLK_LEN == DABGPU_BLANKER_POWER_BLOCK, "block length");
constexpr float BLK_INV_LEN = 0.03125f;               // the mean as a product with 2^-5 (exact)

// |x|^2 of one sample
DABGPU_HD inline float blk_energy(chf2 x) { return __builtin_fmaf(x.im, x.im, x.re * x.re); }

// p of a block from the energies of its 32 samples: a pairwise tree (neighbours first), then the mean; e is overwritten
DABGPU_HD inline float blk_tree(float e[BLK_LEN]) {
    for (int step = 1; step < BLK_LEN; step <<= 1)
        for (int i = 0; i < BLK_LEN; i += 2 * step) e[i] = e[i] + e[i + step];
    return e[0] * BLK_INV_LEN;
}

DABGPU_HD inline bool blk_finite(float p) { return (ch_float_bits(p) & 0x7F800000u) != 0x7F800000u; }
DABGPU_HD inline float blk_q(float p) { return blk_finite(p) ? p : 0.0f; }

// the reach of a stream in blocks: what block b's decision reads either side of b
DABGPU_HD inline int blk_reach(const dabgpu_blanker_stream& P) { return P.gap + P.window + P.guard; }

// flag[b] from p(j) = the power of block b + j, |j| <= gap + window
template <class Power>
DABGPU_HD inline bool blk_flag(const dabgpu_blanker_stream& P, Power p) {
    const float pb = p(0);
    if (!blk_finite(pb)) return true;
    float before = 0.0f, after = 0.0f;
    for (int k = 1; k <= P.window; k++) before = before + blk_q(p(-P.gap - k));
    for (int k = 1; k <= P.window; k++) after = after + blk_q(p(P.gap + k));
    const float ref = before > after ? before : after;
    return ref > 0.0f && (float)P.window * pb > P.threshold * ref;
}

// blank[b] from flag(j) = the flag of block b + j, |j| <= guard
template <class Flag>
DABGPU_HD inline bool blk_blank(const dabgpu_blanker_stream& P, Flag flag) {
    bool any = false;
    for (int j = -P.guard; j <= P.guard; j++) any = any || flag(j);
    return any;
}

// input sample of absolute output sample m (signed: blocks before sample 0 exist and read what lies there, zeros as a rule)
DABGPU_HD inline chf2 blk_input(const chf2* x, int64_t n_in, int64_t start, int64_t m) {
    const int64_t i = m - start;
    return (i >= 0 && i < n_in) ? x[i] : chf2{0.0f, 0.0f};
}

// p of block b, one thread, straight from the definition (the host model; the kernel sums the tree across 16 lanes)
DABGPU_HD inline float blk_power(const chf2* x, int64_t n_in, int64_t start, int64_t b) {
    float e[BLK_LEN];
    for (int i = 0; i < BLK_LEN; i++) e[i] = blk_energy(blk_input(x, n_in, start, b * BLK_LEN + i));
    return blk_tree(e);
}

}  // namespace dabgpu
