// iqbal_core.h -- every arithmetic step of the IQ balance bank (include/dabgpu.h, "IQ balance"), host and device: the kernels (iqbal.hip),
// dabgpu_iqbal_solve_host and the host model of the tests (tests/cpp/iqbal_host_model.cpp) compile these same functions, so the device is
// checked bit for bit against a CPU run of this file, and this file against an independent numpy model (tests/iqbal_model.py).
// The arithmetic contract is channel_core.h's: -ffp-contract=off, every fused operation an explicit fmaf, no division: the two reciprocals
// are dv_reciprocal (diversity_core.h).  A float addition is commutative bit for bit, so the tree below may be summed as a butterfly across
// lanes (blanker_core.h).  Derivation and bounds: DESIGN.md 4.32.
#pragma once
#include <stdint.h>

#include "channel_core.h"
#include "diversity_core.h"

namespace dabgpu {

constexpr int IQB_TILE = DABGPU_IQBAL_TILE;               // 1024 absolute samples
constexpr int IQB_MOMENTS = 5;
constexpr int IQB_TILE_FLOATS = 8;                        // a tile's record in the scratch: the five sums and three zeros (32 bytes)
constexpr float IQB_TILE_WEIGHT = 1024.0f;

// The tile tree: ten levels, each combining the partial sums whose sample index differs in ONE bit, in this order of bits.  Bit 0 first
// (the two samples of a 16-byte load), then bit 9 (the two passes of a thread: samples 2 t + j and 512 + 2 t + j), then bits 1 .. 6 (the
// lanes of a wave, t ^ 1 .. t ^ 32), then bits 7 and 8 (the four waves, through LDS).  iqb_tree is the definition; the kernel's in-lane
// sums, butterfly and LDS step are the same additions.
constexpr int IQB_TREE_BITS[10] = {0, 9, 1, 2, 3, 4, 5, 6, 7, 8};

// v[0 .. 1024) -> the tree's sum; v is overwritten
DABGPU_HD inline float iqb_tree(float* v) {
    uint32_t done = 0;                                    // bits already folded: live entries have them clear
    for (int l = 0; l < 10; l++) {
        const uint32_t bit = 1u << IQB_TREE_BITS[l];
        for (uint32_t i = 0; i < (uint32_t)IQB_TILE; i++)
            if (!(i & (done | bit))) v[i] = v[i] + v[i | bit];
        done |= bit;
    }
    return v[0];
}

struct iqb_coef { chf2 a, b, c; };
struct iqb_moments { float m[IQB_MOMENTS]; };             // sum re, sum im, sum |y|^2, sum (re^2 - im^2), sum 2 re im
struct iqb_state { float N, S[IQB_MOMENTS]; };

DABGPU_HD inline iqb_coef iqb_identity() { return iqb_coef{chf2{1.0f, 0.0f}, chf2{0.0f, 0.0f}, chf2{0.0f, 0.0f}}; }

// z = a y + b conj(y) + c: from c, then the terms of a, then the terms of b
DABGPU_HD inline chf2 iqb_map(const iqb_coef& K, chf2 y) {
    float re = __builtin_fmaf(K.a.re, y.re, K.c.re);
    re = __builtin_fmaf(-K.a.im, y.im, re);
    re = __builtin_fmaf(K.b.re, y.re, re);
    re = __builtin_fmaf(K.b.im, y.im, re);
    float im = __builtin_fmaf(K.a.re, y.im, K.c.im);
    im = __builtin_fmaf(K.a.im, y.re, im);
    im = __builtin_fmaf(K.b.im, y.re, im);
    im = __builtin_fmaf(-K.b.re, y.im, im);
    return chf2{re, im};
}

// the five terms of one raw sample
DABGPU_HD inline iqb_moments iqb_terms(chf2 y) {
    const float rr = y.re * y.re;
    return iqb_moments{{y.re, y.im, __builtin_fmaf(y.im, y.im, rr), __builtin_fmaf(-y.im, y.im, rr), (2.0f * y.re) * y.im}};
}
DABGPU_HD inline iqb_moments iqb_add(const iqb_moments& p, const iqb_moments& q) {
    return iqb_moments{{p.m[0] + q.m[0], p.m[1] + q.m[1], p.m[2] + q.m[2], p.m[3] + q.m[3], p.m[4] + q.m[4]}};
}

// the moments of one tile, one thread, straight from the definition (the host model; the kernel spreads the tree over 256 threads)
inline iqb_moments iqb_tile_moments(const chf2* y) {
    static thread_local float v[IQB_MOMENTS][IQB_TILE];
    for (int i = 0; i < IQB_TILE; i++) {
        const iqb_moments t = iqb_terms(y[i]);
        for (int k = 0; k < IQB_MOMENTS; k++) v[k][i] = t.m[k];
    }
    iqb_moments r;
    for (int k = 0; k < IQB_MOMENTS; k++) r.m[k] = iqb_tree(v[k]);
    return r;
}

DABGPU_HD inline bool iqb_finite(float p) { return (ch_float_bits(p) & 0x7F800000u) != 0x7F800000u; }

// one tile into the state; false: a moment is not finite, the tile is skipped and the state stays
DABGPU_HD inline bool iqb_fold(iqb_state& s, const float* m, float forget) {
    for (int k = 0; k < IQB_MOMENTS; k++)
        if (!iqb_finite(m[k])) return false;
    s.N = __builtin_fmaf(forget, s.N, IQB_TILE_WEIGHT);
    for (int k = 0; k < IQB_MOMENTS; k++) s.S[k] = __builtin_fmaf(forget, s.S[k], m[k]);
    return true;
}

// state -> what the record holds besides the state and the counters.  valid = 0: identity coefficients (d, P, C, w as far as they were
// formed, else 0)
struct iqb_solution { chf2 d; float P; chf2 C, w; iqb_coef K; uint32_t valid; };

DABGPU_HD inline iqb_solution iqb_solve(const iqb_state& s, float min_weight) {
    iqb_solution R;
    R.d = R.C = R.w = chf2{0.0f, 0.0f};
    R.P = 0.0f;
    R.K = iqb_identity();
    R.valid = 0;
    if (!(s.N >= min_weight) || !(s.N >= 1.17549435e-38f)) return R;
    const float r = dv_reciprocal(s.N);
    const chf2 d = chf2{s.S[0] * r, s.S[1] * r};
    R.d = d;
    float P = __builtin_fmaf(-d.re, d.re, s.S[2] * r);
    P = __builtin_fmaf(-d.im, d.im, P);
    R.P = P;
    if (!(P >= 1.17549435e-38f && P <= 3.40282347e+38f)) return R;          // not a normal positive float (zero input, NaN, overflow)
    float qr = __builtin_fmaf(-d.re, d.re, s.S[3] * r);
    qr = __builtin_fmaf(d.im, d.im, qr);
    const float qi = __builtin_fmaf(-2.0f * d.re, d.im, s.S[4] * r);
    const float ip = dv_reciprocal(P);
    const chf2 C = chf2{qr * ip, qi * ip};
    R.C = C;
    if (!(__builtin_fmaf(C.im, C.im, C.re * C.re) < 1.0f)) return R;
    const chf2 h = chf2{0.5f * C.re, 0.5f * C.im};
    chf2 w = h;
    for (int i = 0; i < 3; i++) {
        const float t = __builtin_fmaf(w.im, w.im, __builtin_fmaf(w.re, w.re, 1.0f));
        w = chf2{h.re * t, h.im * t};
    }
    R.w = w;
    const chf2 u = chf2{__builtin_fmaf(w.im, d.im, w.re * d.re), __builtin_fmaf(-w.re, d.im, w.im * d.re)};    // w conj(d)
    R.K.b = chf2{-w.re, -w.im};
    R.K.c = chf2{u.re - d.re, u.im - d.im};
    R.valid = 1;
    return R;
}

// the coefficients a stream's samples are mapped with: FIXED the caller's, TRACK the record's (OFF streams are copied, not mapped)
DABGPU_HD inline iqb_coef iqb_stream_coef(const dabgpu_iqbal_stream& P, const dabgpu_iqbal_record& R) {
    if (P.mode == DABGPU_IQBAL_FIXED) return iqb_coef{chf2{P.a_re, P.a_im}, chf2{P.b_re, P.b_im}, chf2{P.c_re, P.c_im}};
    return iqb_coef{chf2{R.a_re, R.a_im}, chf2{R.b_re, R.b_im}, chf2{R.c_re, R.c_im}};
}

DABGPU_HD inline void iqb_record_reset(dabgpu_iqbal_record& R) {
    R = dabgpu_iqbal_record{};
    R.a_re = 1.0f;
}

// the tiles of one MEASURE call folded into a TRACK stream's record, then the solve; moment(j) = the five sums of the call's tile j
template <class Moment>
DABGPU_HD inline void iqb_fold_and_solve(const dabgpu_iqbal_stream& P, dabgpu_iqbal_record& R, int tiles, Moment moment) {
    iqb_state s;
    s.N = R.N;
    for (int k = 0; k < IQB_MOMENTS; k++) s.S[k] = R.S[k];
    for (int j = 0; j < tiles; j++) {
        if (iqb_fold(s, moment(j), P.forget)) R.tiles_used++;
        else R.tiles_skipped++;
    }
    const iqb_solution Z = iqb_solve(s, P.min_weight);
    R.N = s.N;
    for (int k = 0; k < IQB_MOMENTS; k++) R.S[k] = s.S[k];
    R.d_re = Z.d.re; R.d_im = Z.d.im; R.P = Z.P; R.C_re = Z.C.re; R.C_im = Z.C.im; R.w_re = Z.w.re; R.w_im = Z.w.im;
    R.a_re = Z.K.a.re; R.a_im = Z.K.a.im; R.b_re = Z.K.b.re; R.b_im = Z.K.b.im; R.c_re = Z.K.c.re; R.c_im = Z.K.c.im;
    R.valid = Z.valid;
}

}  // namespace dabgpu
