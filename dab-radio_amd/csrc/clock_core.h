// clock_core.h -- the arithmetic of the sampling-clock tracker (include/dabgpu.h, "Sampling-clock tracker"), host and device: the kernels
// (clock.hip), the host forms (dabgpu_clock_estimate_host, dabgpu_clock_derotate_host) and the host model of the tests
// (tests/cpp/clock_host_model.cpp) compile these same statements, so the device is checked bit for bit against a CPU run of this file,
// and this file against an independent numpy model (tests/clock_model.py).  The library's arithmetic contract holds: -ffp-contract=off,
// every fused step an explicit fmaf, sums in a written order, no `/` at run time (the reciprocal is diversity_core.h's), no library
// transcendental (the oscillator is channel_core.h's, the arctangent a polynomial written out here).
//
// What is measured.  A sampling-clock error eps moves the sampling instant by eps * 2552 samples from one OFDM symbol to the next; in a
// DQPSK product of two neighbouring symbols that is a phase ramp over the carriers, theta * k cycles at carrier number k with
// theta = eps * 2552 / 2048.  The demodulator's products are d = X[s] conj(X[s + 1]), the later symbol conjugated, so the ramp on them
// is -theta * k.  The product of two products L carriers apart, p = d[c] conj(d[c + L]), has lost the channel (squared magnitudes only
// remain), the frame's common phase and every window offset; what is left is +theta * L plus the data's multiple of a quarter turn,
// which the fold into the sector |arg| <= 45 degrees removes.  The sum of the folded products points at theta * L.
//
// Order of the sum.  A row's 768 float4 (carrier pairs 2 j, 2 j + 1) are dealt to 256 owners: owner t has the positions j = t, t + 256,
// t + 512, of which those with j in 0 .. 367 or 384 .. 751 have their lag partner j + 16 in the same half of the block.  An owner chains
// from +0, row after row (s = 0 .. 74), in each row its positions in that order, in each position carrier 2 j before 2 j + 1:
// a = a + folded, re and im apart.  The 64 owners 64 w .. 64 w + 63 of wave w meet in the wavefront tree (a[i] + a[i + h] for i < h,
// h = 32 .. 1), and the four wave sums join as (p0 + p1) + (p2 + p3).  The order does not depend on launch geometry; clk_frame_sum
// below is the definition.  A chain holds at most 450 terms, so one tree per frame serves and no row needs a barrier.
#pragma once
#include <stdint.h>

#include "channel_core.h"
#include "noise_profile_core.h"

namespace dabgpu {

constexpr int CLK_SYMBOLS = 75, CLK_CARRIERS = NP_CARRIERS, CLK_LAG = DABGPU_CLOCK_LAG, CLK_OWNERS = 256, CLK_WAVES = 4;
constexpr int CLK_ROW_F4 = CLK_CARRIERS / 2, CLK_LAG_F4 = CLK_LAG / 2, CLK_HALF_F4 = CLK_ROW_F4 / 2;
constexpr int CLK_PAIRS = CLK_SYMBOLS * 2 * (CLK_CARRIERS / 2 - CLK_LAG);                      // 75 x 1472
constexpr int64_t CLK_MAX_SLOPE = DABGPU_CLOCK_MAX_SLOPE;
static_assert(CLK_LAG == 32 && CLK_LAG_F4 == 16 && CLK_PAIRS == 110400, "lag 32: the partner of float4 j is float4 j + 16");
static_assert(CLK_OWNERS * 3 == CLK_ROW_F4 && CLK_WAVES * 64 == CLK_OWNERS, "three positions an owner, four waves of owners");

// carrier number of carrier index c: -768 .. -1, 1 .. 768
DABGPU_HD inline int clk_carrier_number(int c) { return c < CLK_CARRIERS / 2 ? c - 768 : c - 767; }
// float4 position j of a row has a lag partner in its own half
DABGPU_HD inline bool clk_position_pairs(int j) { return (j < CLK_HALF_F4 ? j : j - CLK_HALF_F4) < CLK_HALF_F4 - CLK_LAG_F4; }

DABGPU_HD inline int64_t clk_clamp(int64_t s) { return s > CLK_MAX_SLOPE ? CLK_MAX_SLOPE : (s < -CLK_MAX_SLOPE ? -CLK_MAX_SLOPE : s); }

// (cos, sin)(k * slope), which takes the ramp -k * slope off a product: the ramp of carrier number k is the exact product k * slope
// mod 2^64, its angle the top 24 bits
DABGPU_HD inline chf2 clk_rotation(int64_t slope_q64, int k) {
    return ch_cos_sin(ch_osc_cycles(0u, (uint64_t)slope_q64, (uint64_t)(int64_t)k));
}
// (cos, -sin)(L * slope): what de-rotating every product by `slope` does to a lag product
DABGPU_HD inline chf2 clk_prior(int64_t slope_q64) {
    const chf2 cs = clk_rotation(slope_q64, CLK_LAG);
    return chf2{cs.re, -cs.im};
}
// y * rot in the product order of ch_finish
DABGPU_HD inline chf2 clk_rotate(chf2 rot, chf2 y) {
    const float b0 = rot.im * y.im, b1 = rot.im * y.re;
    return chf2{__builtin_fmaf(rot.re, y.re, -b0), __builtin_fmaf(rot.re, y.im, b1)};
}

// step 1: p = lo conj(hi)
DABGPU_HD inline chf2 clk_lag_product(chf2 lo, chf2 hi) {
    return chf2{__builtin_fmaf(lo.re, hi.re, lo.im * hi.im), __builtin_fmaf(lo.im, hi.re, -(lo.re * hi.im))};
}
DABGPU_HD inline bool clk_finite(float x) { return __builtin_fabsf(x) <= 3.40282347e+38f; }       // (false for NaN)
// step 3: one of p, -p, -i p, i p with |im| <= re
DABGPU_HD inline chf2 clk_fold(chf2 p) {
    if (__builtin_fabsf(p.re) >= __builtin_fabsf(p.im)) return p.re >= 0.0f ? p : chf2{-p.re, -p.im};
    return p.im > 0.0f ? chf2{p.im, -p.re} : chf2{-p.im, p.re};
}

// steps 1 to 3 and one link of an owner's chain
struct clk_sum { float re, im; uint32_t dropped; };
DABGPU_HD inline void clk_add(clk_sum& a, bool prior, chf2 rot, chf2 lo, chf2 hi) {
    chf2 p = clk_lag_product(lo, hi);
    if (prior) p = clk_rotate(rot, p);
    if (!clk_finite(p.re) || !clk_finite(p.im)) { a.dropped++; return; }
    const chf2 f = clk_fold(p);
    a.re = a.re + f.re;
    a.im = a.im + f.im;
}
DABGPU_HD inline float clk_join(float p0, float p1, float p2, float p3) { return (p0 + p1) + (p2 + p3); }

// step 5: atan(t) / (2 pi) for |t| <= 1 (and the ulp beyond that the quotient can reach), an odd polynomial by Horner in fmaf.  The
// coefficients are a minimax fit of degree 11: approximation 2.7e-7 cycles, eight float32 roundings of values below 0.272 another 1.3e-7,
// together within 4.0e-7 cycles = 2.5e-6 rad of float64 atan (tests/test_clock_model.py shows it), the equivalent of 0.01 ppm at lag 32.
DABGPU_HD inline float clk_atan_cycles(float t) {
    const float z = t * t;
    float p = __builtin_fmaf(-0.001865148195065558f, z, 0.008379058912396431f);
    p = __builtin_fmaf(p, z, -0.018529823049902916f);
    p = __builtin_fmaf(p, z, 0.03080289624631405f);
    p = __builtin_fmaf(p, z, -0.052938565611839294f);
    p = __builtin_fmaf(p, z, 0.15915131568908691f);
    return p * t;
}
DABGPU_HD inline bool clk_sum_valid(float re, float im, uint32_t dropped) {
    return re >= 1.17549435e-38f && re <= 3.40282347e+38f && __builtin_fabsf(im) <= re && 2u * dropped < (uint32_t)CLK_PAIRS;
}
// a float of cycles over the lag as a slope word: cycles * 2^59, rounded to nearest (exact from 2^-36 cycles up)
DABGPU_HD inline int64_t clk_cycles_q59(float cycles) { return (int64_t)__builtin_rintf(cycles * 0x1p59f); }

// steps 5 and 6 from the frame's sum
struct clk_update { int64_t slope, residual; bool valid; };
DABGPU_HD inline clk_update clk_frame_update(float re, float im, uint32_t dropped, int64_t slope_in, float gain) {
    if (!clk_sum_valid(re, im, dropped)) return clk_update{slope_in, 0, false};
    const float cycles = clk_atan_cycles(im * dv_reciprocal(re));
    const int64_t step = gain == 1.0f ? clk_cycles_q59(cycles) : clk_cycles_q59(gain * cycles);
    return clk_update{clk_clamp(clk_clamp(slope_in) + step), clk_cycles_q59(cycles), true};
}
DABGPU_HD inline bool clk_gain_ok(float gain) { return gain > 0.0f && gain <= 1.0f; }             // (false for NaN)

// ---- the host forms ----
// steps 1 to 4 of one frame's products dq [75][1536] complex float
inline void clk_frame_sum(const float* dq, int64_t slope_in, float* re, float* im, uint32_t* dropped) {
    const int64_t prior_slope = clk_clamp(slope_in);
    const bool prior = prior_slope != 0;
    const chf2 rot = prior ? clk_prior(prior_slope) : chf2{1.0f, 0.0f};
    float part[2][CLK_WAVES];
    uint32_t n = 0;
    for (int w = 0; w < CLK_WAVES; w++) {
        float ar[64], ai[64];
        for (int l = 0; l < 64; l++) {
            clk_sum a{0.0f, 0.0f, 0u};
            for (int s = 0; s < CLK_SYMBOLS; s++) {
                const float* const row = dq + 2 * (size_t)s * CLK_CARRIERS;
                for (int i = 0; i < 3; i++) {
                    const int j = 64 * w + l + CLK_OWNERS * i;
                    if (!clk_position_pairs(j)) continue;
                    const float *lo = row + 4 * j, *hi = lo + 4 * CLK_LAG_F4;
                    clk_add(a, prior, rot, chf2{lo[0], lo[1]}, chf2{hi[0], hi[1]});
                    clk_add(a, prior, rot, chf2{lo[2], lo[3]}, chf2{hi[2], hi[3]});
                }
            }
            ar[l] = a.re; ai[l] = a.im; n += a.dropped;
        }
        part[0][w] = np_half_tree(ar); part[1][w] = np_half_tree(ai);
    }
    *re = clk_join(part[0][0], part[0][1], part[0][2], part[0][3]);
    *im = clk_join(part[1][0], part[1][1], part[1][2], part[1][3]);
    *dropped = n;
}

// one whole frame of the estimator on the host.  sync_ok false: the frame is skipped and dq is not read.  corr [2] may be null.
inline clk_update clk_estimate_frame(const float* dq, bool sync_ok, int64_t slope_in, float gain, float* corr) {
    clk_update u{slope_in, 0, false};
    float re = 0.0f, im = 0.0f;
    if (sync_ok) {
        uint32_t dropped;
        clk_frame_sum(dq, slope_in, &re, &im, &dropped);
        u = clk_frame_update(re, im, dropped, slope_in, gain);
    }
    if (corr) { corr[0] = u.valid ? re : 0.0f; corr[1] = u.valid ? im : 0.0f; }
    return u;
}

// step 7 of one frame on the host; out may be in.  slope 0: a copy (in place: nothing).
inline void clk_derotate_frame(const float* in, float* out, int64_t slope_q64) {
    const size_t n = (size_t)CLK_SYMBOLS * CLK_CARRIERS;
    if (slope_q64 == 0) {
        if (out != in) for (size_t i = 0; i < 2 * n; i++) out[i] = in[i];
        return;
    }
    for (int c = 0; c < CLK_CARRIERS; c++) {
        const chf2 rot = clk_rotation(slope_q64, clk_carrier_number(c));
        for (int s = 0; s < CLK_SYMBOLS; s++) {
            const size_t i = 2 * ((size_t)s * CLK_CARRIERS + (size_t)c);
            const chf2 v = clk_rotate(rot, chf2{in[i], in[i + 1]});
            out[i] = v.re; out[i + 1] = v.im;
        }
    }
}

}  // namespace dabgpu
