// channel_core.h -- every arithmetic step of the channel model (include/dabgpu.h, "Channel model"), host and device: the kernel
// (channel.hip) and the host model of the tests (tests/cpp/channel_host_model.cpp) compile these same functions, so the device is
// checked bit for bit against a CPU run of this file, and this file against an independent numpy model (tests/channel_model.py).
// The library's arithmetic contract holds: built with -ffp-contract=off, every fused operation an explicit fmaf, no library
// transcendental (logf / sincosf differ between host and device): the logarithm is exponent * ln 2 + an explicit series on the
// mantissa, sine and cosine are the Chebyshev form of ofdm_device.h restated with fmaf.  The one quotient and the one square root of
// Box-Muller are Newton iterations written out in fmaf as well: with the `/` and sqrtf of the two compilers the noise differed in its
// last bit between an MI355X and the host (measured; the signal path, which has neither, was equal).  Error bounds: DESIGN.md 4.16.
#pragma once
#include <stdint.h>

#include "dabgpu_host_logic.h"

namespace dabgpu {

struct chf2 { float re, im; };

// ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) ----
DABGPU_HD inline void ch_philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out[4]) {
#if defined(__HIPCC__)                 // (the planner's plain C++ build of this header does not know the pragma)
#pragma unroll
#endif
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the four words shared by samples 2 p and 2 p + 1 of stream s
DABGPU_HD inline void ch_noise_words(uint64_t seed, uint32_t s, uint64_t pair, uint32_t w[4]) {
    ch_philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)pair, (uint32_t)(pair >> 32), s, 0u, w);
}

// A uniform is ((w >> 8) + 0.5) * 2^-24 = n * 2^-25 with n = 2 (w >> 8) + 1 odd, in [2^-25, 1 - 2^-25]: never 0.  n has 25 bits, one more
// than a float holds, so the two places that use a uniform take what they need from the INTEGER, exactly: the logarithm its normalised
// mantissa minus one, the angle n - 2^24.
DABGPU_HD inline uint32_t ch_uniform_n(uint32_t w) { return ((w >> 8) << 1) | 1u; }

// ln(n * 2^-25), n odd below 2^25: n = 2^E' * m with m in [sqrt(1/2), sqrt(2)), f = m - 1 formed exactly from the integer (at most 24
// significant bits), ln m = 2 atanh(s), s = f / (2 + f), |s| <= 0.1716, as 2 s (1 + z / 3 + z^2 / 5 + z^3 / 7 + z^4 / 9), z = s^2 (the
// series' next term is below 2.1e-9 of the sum); the result is E ln 2 + ln m with E = E' - 25.  < 0.
DABGPU_HD inline uint32_t ch_float_bits(float x) { uint32_t b; __builtin_memcpy(&b, &x, 4); return b; }
DABGPU_HD inline float ch_bits_float(uint32_t b) { float x; __builtin_memcpy(&x, &b, 4); return x; }

// f / a for a in [1.29, 2.42]: 1 / a from a linear seed (within 7 %) by three Newton steps, the quotient and one residual correction
DABGPU_HD inline float ch_quotient(float f, float a) {
    float r = __builtin_fmaf(-0.3125f, a, 1.171875f);
    r = __builtin_fmaf(r, __builtin_fmaf(-a, r, 1.0f), r);
    r = __builtin_fmaf(r, __builtin_fmaf(-a, r, 1.0f), r);
    r = __builtin_fmaf(r, __builtin_fmaf(-a, r, 1.0f), r);
    const float q = f * r;
    return __builtin_fmaf(__builtin_fmaf(-a, q, f), r, q);
}

// sqrt(v) for a normal v > 0: v = 4^k q with q in [1, 4) through the exponent field (exact), 1 / sqrt(q) from a linear seed (within 12 %)
// by four Newton steps, the root q y and one residual correction, scaled back by 2^k
DABGPU_HD inline float ch_sqrt(float v) {
    const uint32_t b = ch_float_bits(v);
    const int k = (((int)(b >> 23) - 127) >> 1);                          // floor(exponent / 2)
    const float q = ch_bits_float(b - ((uint32_t)(2 * k) << 23));
    float y = __builtin_fmaf(-0.1666666716f, q, 1.12f);
    for (int i = 0; i < 4; i++) y = y * __builtin_fmaf(-0.5f * q, y * y, 1.5f);
    const float r = q * y;
    const float root = __builtin_fmaf(__builtin_fmaf(-r, r, q), 0.5f * y, r);
    return root * ch_bits_float((uint32_t)(127 + k) << 23);
}

DABGPU_HD inline float ch_log_n25(uint32_t n) {
    const int lz = __builtin_clz(n);
    const uint32_t nn = n << lz;                               // bit 31 set: m = nn * 2^-31 in [1, 2)
    int e = (31 - lz) - 25;
    float f;
    if (nn > 0xB504F333u) { f = -((float)(0u - nn) * 0x1p-32f); e += 1; }      // above sqrt(2): m / 2 - 1 = -(2^32 - nn) * 2^-32
    else f = (float)(nn - 0x80000000u) * 0x1p-31f;
    const float s = ch_quotient(f, 2.0f + f);
    const float z = s * s;
    float p = __builtin_fmaf(z, 0.111111111f, 0.142857143f);
    p = __builtin_fmaf(p, z, 0.2f);
    p = __builtin_fmaf(p, z, 0.333333333f);
    p = __builtin_fmaf(p, z, 1.0f);
    const float lnm = (2.0f * s) * p;
    return __builtin_fmaf((float)e, 0.693147182f, lnm);
}

// sin(2 pi x) for x in [-0.5, 0.5]: the Chebyshev form of ofdm_device.h (cheb2), Horner with fmaf
DABGPU_HD inline float ch_sin_cycles(float x) {
    const float z = x * x;
    float b = __builtin_fmaf(3.20396066f, z, -14.07150173f);
    b = __builtin_fmaf(b, z, 38.50016403f);
    b = __builtin_fmaf(b, z, -67.07687378f);
    b = __builtin_fmaf(b, z, 64.83583069f);
    b = __builtin_fmaf(b, z, -25.13274193f);
    return (b * (z - 0.25f)) * x;
}
// (cos, sin)(2 pi t) for t in [-0.5, 0.5]: the cosine is the sine a quarter cycle on, wrapped back into the range
DABGPU_HD inline chf2 ch_cos_sin(float t) {
    float d = t + 0.25f;
    d = d - __builtin_rintf(d);
    return chf2{ch_sin_cycles(d), ch_sin_cycles(t)};
}

// Box-Muller on two words: r = sqrt(-2 ln u1), angle u2 - 1/2 of a cycle (as uniform as u2 itself)
DABGPU_HD inline chf2 ch_gauss_pair(uint32_t w0, uint32_t w1) {
    const float r = ch_sqrt(-2.0f * ch_log_n25(ch_uniform_n(w0)));
    const chf2 cs = ch_cos_sin((float)((int32_t)ch_uniform_n(w1) - (1 << 24)) * 0x1p-25f);
    return chf2{r * cs.re, r * cs.im};
}

// the oscillator's angle at sample m: the top 24 bits of the 64-bit phase, as cycles in [-0.5, 0.5) (exact)
DABGPU_HD inline float ch_osc_cycles(uint64_t phase0_q64, uint64_t freq_q64, uint64_t m) {
    const uint64_t ph = phase0_q64 + m * freq_q64;
    return (float)(int32_t)((int64_t)ph >> 40) * 0x1p-24f;
}

// input index of (output sample m, tap delay d); wrap: modulo n_in, else -1 outside the input (the sample is zero)
DABGPU_HD inline int64_t ch_src_index(uint64_t m, int64_t start, int32_t delay, int64_t n_in, bool wrap) {
    // (m, start: any 64-bit values; the unsigned difference wraps like the stream position)
    int64_t i = (int64_t)(m - (uint64_t)start - (uint64_t)(int64_t)delay);
    if (wrap) { i %= n_in; return i < 0 ? i + n_in : i; }
    return (i < 0 || i >= n_in) ? -1 : i;
}

// z += h * x in the order of the definition (the first tap starts from the products, so that a tap of 1 passes x through unchanged)
DABGPU_HD inline chf2 ch_tap_first(float hr, float hi, chf2 x) {
    return chf2{__builtin_fmaf(-hi, x.im, hr * x.re), __builtin_fmaf(hi, x.re, hr * x.im)};
}
DABGPU_HD inline chf2 ch_tap_add(chf2 z, float hr, float hi, chf2 x) {
    float re = __builtin_fmaf(hr, x.re, z.re);
    re = __builtin_fmaf(-hi, x.im, re);
    float im = __builtin_fmaf(hr, x.im, z.im);
    im = __builtin_fmaf(hi, x.re, im);
    return chf2{re, im};
}

// the paths of one sample; fetch(k) = x[src_k] (zero where the definition says so)
template <class Fetch>
DABGPU_HD inline chf2 ch_paths(const dabgpu_channel_stream& P, Fetch fetch) {
    chf2 z = ch_tap_first(P.tap_re[0], P.tap_im[0], fetch(0));
    for (int k = 1; k < P.n_taps; k++) z = ch_tap_add(z, P.tap_re[k], P.tap_im[k], fetch(k));
    return z;
}

// gain, rotation and noise of sample m from its path sum z; w = the noise words of the sample's pair (read only when noise_sigma != 0)
DABGPU_HD inline chf2 ch_finish(const dabgpu_channel_stream& P, uint64_t m, chf2 z, const uint32_t w[4]) {
    chf2 y = chf2{P.gain * z.re, P.gain * z.im};
    if ((P.freq_q64 | P.phase0_q64) != 0) {
        const chf2 cs = ch_cos_sin(ch_osc_cycles(P.phase0_q64, P.freq_q64, m));
        const float b0 = cs.im * y.im, b1 = cs.im * y.re;
        y = chf2{__builtin_fmaf(cs.re, y.re, -b0), __builtin_fmaf(cs.re, y.im, b1)};
    }
    if (P.noise_sigma != 0.0f) {
        const int h = (int)(m & 1u) * 2;
        const chf2 g = ch_gauss_pair(w[h], w[h + 1]);
        y = chf2{__builtin_fmaf(P.noise_sigma, g.re, y.re), __builtin_fmaf(P.noise_sigma, g.im, y.im)};
    }
    return y;
}

// ---- fading taps (include/dabgpu.h, "Channel model, fading taps"; bounds: DESIGN.md 4.18) ----
constexpr int CH_FADE_GRID_SHIFT = 6;                                        // DABGPU_FADING_GRID = 64
constexpr int CH_FADE_MAX_POINTS = 18;                                       // grid points a tile of 1024 samples aligned to 4 can touch
static_assert((1 << CH_FADE_GRID_SHIFT) == DABGPU_FADING_GRID, "grid");

// bit k set: tap k of the stream fades
DABGPU_HD inline uint32_t ch_fading_mask(const dabgpu_channel_fading_stream& F, int n_taps) {
    uint32_t mask = 0;
    for (int k = 0; k < n_taps; k++) mask |= (F.kind[k] == DABGPU_TAP_FADING ? 1u : 0u) << k;
    return mask;
}
// (cos, sin) of oscillator n of a tap at grid point j (absolute sample 64 j)
DABGPU_HD inline chf2 ch_fading_osc(const dabgpu_channel_fading_tap& T, int n, uint64_t j) {
    return ch_cos_sin(ch_osc_cycles(T.phase_q64[n], T.freq_q64[n], j << CH_FADE_GRID_SHIFT));
}
// the 16 diffuse terms as the fixed pairwise tree v[i] += v[i ^ 1], v[i ^ 2], v[i ^ 4], v[i ^ 8]: every level adds partners both ways
// round (the sum of two floats does not depend on their order), which is what 16 lanes exchanging registers do; v[0] is the sum
DABGPU_HD inline float ch_fading_tree16(float v[16]) {
    for (int stride = 1; stride < 16; stride <<= 1) {
        float t[16];
        for (int i = 0; i < 16; i++) t[i] = v[i] + v[i ^ stride];
        for (int i = 0; i < 16; i++) v[i] = t[i];
    }
    return v[0];
}
// G_j from the tree's sums and the line of sight (los is not read when amp_los == 0)
DABGPU_HD inline chf2 ch_fading_combine(float amp_diffuse, float amp_los, chf2 sum, chf2 los) {
    const chf2 d = chf2{amp_diffuse * sum.re, amp_diffuse * sum.im};
    if (amp_los == 0.0f) return d;
    return chf2{__builtin_fmaf(amp_los, los.re, d.re), __builtin_fmaf(amp_los, los.im, d.im)};
}
// G_j of one tap, one thread (the kernel spreads the same operations over 16 lanes)
DABGPU_HD inline chf2 ch_fading_grid_gain(const dabgpu_channel_fading_tap& T, uint64_t j) {
    float c[16], s[16];
    for (int n = 0; n < 16; n++) { const chf2 cs = ch_fading_osc(T, n, j); c[n] = cs.re; s[n] = cs.im; }
    const chf2 sum = chf2{ch_fading_tree16(c), ch_fading_tree16(s)};
    const chf2 los = (T.amp_los != 0.0f) ? ch_fading_osc(T, 16, j) : chf2{0.0f, 0.0f};
    return ch_fading_combine(T.amp_diffuse, T.amp_los, sum, los);
}
// g(m) between the grid points j = m >> 6 and j + 1
DABGPU_HD inline chf2 ch_fading_interp(chf2 g0, chf2 g1, uint64_t m) {
    const float w = (float)(uint32_t)(m & (uint64_t)(DABGPU_FADING_GRID - 1)) * 0x1p-6f;
    return chf2{__builtin_fmaf(w, g1.re - g0.re, g0.re), __builtin_fmaf(w, g1.im - g0.im, g0.im)};
}
// the paths of one sample of a fading stream; gain(k) = g_k(m) (called for the taps of `mask` only), fetch(k) as in ch_paths
template <class Gain, class Fetch>
DABGPU_HD inline chf2 ch_paths_fading(const dabgpu_channel_stream& P, uint32_t mask, Gain gain, Fetch fetch) {
    chf2 z = chf2{0.0f, 0.0f};
    for (int k = 0; k < P.n_taps; k++) {
        float hr = P.tap_re[k], hi = P.tap_im[k];
        if ((mask >> k) & 1u) { const chf2 e = ch_tap_first(hr, hi, gain(k)); hr = e.re; hi = e.im; }
        z = (k == 0) ? ch_tap_first(hr, hi, fetch(0)) : ch_tap_add(z, hr, hi, fetch(k));
    }
    return z;
}

// the modulator's quantiser (ofdm_mod.hip, tx_u8): x * scale + 127.5, clamped to [0, 255] (NaN -> 0), truncated
DABGPU_HD inline uint32_t ch_u8(float x, float scale) {
    float v = x * scale;
    v = v + 127.5f;
    v = (v > 0.0f) ? v : 0.0f;
    v = (v > 255.0f) ? 255.0f : v;
    return (uint32_t)v;
}

// largest tap delay of a stream, rounded up to an even count
DABGPU_HD inline int ch_stream_halo(const dabgpu_channel_stream& P) {
    int h = 0;
    for (int k = 0; k < P.n_taps; k++) h = P.tap_delay[k] > h ? P.tap_delay[k] : h;
    return (h + 1) & ~1;
}
DABGPU_HD inline bool ch_stream_direct(const dabgpu_channel_stream& P) { return P.n_taps == 1 && P.tap_delay[0] == 0; }

}  // namespace dabgpu
