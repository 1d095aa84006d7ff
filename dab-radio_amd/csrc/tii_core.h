// tii_core.h -- the arithmetic of the TII detector behind the transform (include/dabgpu.h, "TII": power, fold, accumulate, decision) and
// the carrier rule of both directions, host and device: the kernels (tii.hip, ofdm_mod.hip) and the host model of the tests
// (tests/cpp/tii_host_model.cpp) compile these same statements, so the device is checked bit for bit against a CPU run of this file, and
// this file against an independent float64 model (tests/tii_model.py).  The library's arithmetic contract holds: -ffp-contract=off, the
// one fused operation an explicit fmaf, sums in a written order, no `/`: the mean over 24 combs is a product with a constant and the
// one quotient (a record's strength) a reciprocal by Newton steps in fmaf, the same bits on both sides.
#pragma once
#include <stdint.h>

#include "dabgpu_host_logic.h"

namespace dabgpu {

constexpr int TII_COMBS = DABGPU_TII_COMBS, TII_GROUPS = DABGPU_TII_GROUPS, TII_ACC = TII_COMBS * TII_GROUPS;
constexpr int TII_NB_MAIN = DABGPU_TII_NB_MAIN, TII_PREFIX = 608, TII_FFT = 2048;

// T[p]: the 70 bytes with four bits set, ascending; group b of main id p is on when bit 7 - b is set
DABGPU_HD inline uint32_t tii_pattern(int p) {
    const uint8_t T[TII_NB_MAIN] = {
        0x0F, 0x17, 0x1B, 0x1D, 0x1E, 0x27, 0x2B, 0x2D, 0x2E, 0x33, 0x35, 0x36, 0x39, 0x3A, 0x3C, 0x47, 0x4B, 0x4D, 0x4E, 0x53, 0x55, 0x56, 0x59, 0x5A,
        0x5C, 0x63, 0x65, 0x66, 0x69, 0x6A, 0x6C, 0x71, 0x72, 0x74, 0x78, 0x87, 0x8B, 0x8D, 0x8E, 0x93, 0x95, 0x96, 0x99, 0x9A, 0x9C, 0xA3, 0xA5, 0xA6,
        0xA9, 0xAA, 0xAC, 0xB1, 0xB2, 0xB4, 0xB8, 0xC3, 0xC5, 0xC6, 0xC9, 0xCA, 0xCC, 0xD1, 0xD2, 0xD4, 0xD8, 0xE1, 0xE2, 0xE4, 0xE8, 0xF0};
    return T[p];
}
// the main id of a mask with four bits set (its rank among such bytes), -1 for any other mask
DABGPU_HD inline int tii_main_id(uint32_t mask) {
    if (mask > 0xFFu || __builtin_popcount(mask) != 4) return -1;
    int p = 0;
    for (uint32_t v = 0x0Fu; v < mask; v++) p += (__builtin_popcount(v) == 4);
    return p;
}

// carrier q (0 .. 31) of (main id p, sub id c): pair q >> 1 = (set bit number (q >> 3) of the pattern from b = 0 up, block (q >> 1) & 3),
// its second carrier when q is odd.  *k0 = the pair's first carrier, whose PRS phase both carry.  Carriers are numbered -768 .. 768.
DABGPU_HD inline int tii_carrier(int p, int c, int q, int* k0) {
    const uint32_t pat = tii_pattern(p);
    int b = 0;
    for (int seen = -1; b < 8; b++) {
        seen += (int)((pat >> (7 - b)) & 1u);
        if (seen == (q >> 3)) break;
    }
    const int blk = (q >> 1) & 3;
    const int B = (blk == 0) ? -768 : (blk == 1) ? -384 : (blk == 2) ? 1 : 385;
    *k0 = B + 2 * c + 48 * b;
    return *k0 + (q & 1);
}
DABGPU_HD inline int tii_bin(int k) { return k & (TII_FFT - 1); }

// step 4
DABGPU_HD inline float tii_power(float re, float im) { return __builtin_fmaf(re, re, im * im); }

// step 5: E[c][b] from the bin powers, P(bin) -> float
template <class Power>
DABGPU_HD inline float tii_fold(Power P, int c, int b) {
    const int o = 2 * c + 48 * b;
    const float q0 = P(tii_bin(-768 + o)) + P(tii_bin(-768 + o + 1));
    const float q1 = P(tii_bin(-384 + o)) + P(tii_bin(-384 + o + 1));
    const float q2 = P(tii_bin(1 + o)) + P(tii_bin(1 + o + 1));
    const float q3 = P(tii_bin(385 + o)) + P(tii_bin(385 + o + 1));
    return (q0 + q1) + (q2 + q3);
}

// step 7, one comb: its eight values in ascending order (Batcher's odd-even merge sort, 19 exchanges)
DABGPU_HD inline void tii_sort8(const float* v, float* s) {
    for (int i = 0; i < 8; i++) s[i] = v[i];
#define TII_CX(i, j) do { const float lo_ = s[i] < s[j] ? s[i] : s[j], hi_ = s[i] < s[j] ? s[j] : s[i]; s[i] = lo_; s[j] = hi_; } while (0)
    TII_CX(0, 1); TII_CX(2, 3); TII_CX(4, 5); TII_CX(6, 7);
    TII_CX(0, 2); TII_CX(1, 3); TII_CX(4, 6); TII_CX(5, 7);
    TII_CX(1, 2); TII_CX(5, 6);
    TII_CX(0, 4); TII_CX(1, 5); TII_CX(2, 6); TII_CX(3, 7);
    TII_CX(2, 4); TII_CX(3, 5);
    TII_CX(1, 2); TII_CX(3, 4); TII_CX(5, 6);
#undef TII_CX
}
// the comb's share of the floor: the mean of its four smallest
DABGPU_HD inline float tii_comb_floor(const float* s) { return ((s[0] + s[1]) + (s[2] + s[3])) * 0.25f; }
// N: the mean of the 24 shares, summed in order of c
DABGPU_HD inline float tii_floor(const float* share) {
    float n = share[0];
    for (int c = 1; c < TII_COMBS; c++) n = n + share[c];
    return n * (1.0f / 24.0f);
}

// 1 / x for a normal x > 0: the exponent mirrored about 1 as the seed (within 12.5 %), four Newton steps
DABGPU_HD inline float tii_reciprocal(float x) {
    uint32_t b;
    __builtin_memcpy(&b, &x, 4);
    b = 0x7EF311C7u - b;
    float r;
    __builtin_memcpy(&r, &b, 4);
    for (int i = 0; i < 4; i++) r = __builtin_fmaf(r, __builtin_fmaf(-x, r, 1.0f), r);
    return r;
}

// the decision of one comb from its values v (group order), their sorted copy s and the level threshold * N; rn = tii_reciprocal(N).
// true: the comb is active and *out its record
DABGPU_HD inline bool tii_comb_decide(int c, const float* v, const float* s, float level, float n, float rn, dabgpu_tii_record* out) {
    if (!(s[4] >= level)) return false;                     // the fourth largest
    uint32_t mask = 0;
    float sum = 0.0f;
    int cnt = 0;
    for (int b = 0; b < TII_GROUPS; b++)
        if (v[b] >= level) { mask |= 1u << (7 - b); sum = sum + v[b]; cnt++; }
    const float mean = sum * (cnt == 4 ? 0.25f : cnt == 5 ? 0.2f : cnt == 6 ? (1.0f / 6.0f) : cnt == 7 ? (1.0f / 7.0f) : 0.125f);
    const float q = mean * rn;
    out->sub_id = c;
    out->main_id = tii_main_id(mask);
    out->mask = mask;
    out->strength = __builtin_fmaf(__builtin_fmaf(-n, q, mean), rn, q);
    return true;
}

// an offset of the synchroniser's that a NULL window may be placed with (the range dabgpu_ofdm_sync_demod_frames documents)
DABGPU_HD inline bool tii_time_offset_ok(int fine_time_offset) { return fine_time_offset >= -504 && fine_time_offset <= 1543; }

}  // namespace dabgpu
