// dd_profile_core.h -- the arithmetic of the decision-directed noise profile (include/dabgpu.h, "Decision-directed noise profile"), host and
// device: the kernel (dd_profile.hip), the host form (dabgpu_dd_profile_carriers_host) and the host model of the tests
// (tests/cpp/dd_profile_host_model.cpp) compile these same statements, so the device is checked bit for bit against a CPU run of this
// file, and this file against an independent numpy model (tests/dd_profile_model.py).  The library's arithmetic contract holds:
// -ffp-contract=off, the one fused step an explicit fmaf, sums in a written order, no `/` at run time.  Bands, exclusion, smoothing, mean
// and weights are noise_profile_core.h's, called with Q in the place of C; nothing of them is restated here.
//
// What is measured.  A DQPSK product d = X_i conj(X_i+1) of a carrier with channel power a = |H|^2 and noise power q per bin (in the
// units of the unnormalised transform, where white noise of power s2 per sample has q = 2048 s2) has E|d|^2 = (a + q)^2, and while
// the decisions are right the mean of (|re d| + |im d|) / sqrt(2) is a.  So over the 75 products of a frame
//     q = rms(d) - mean projected amplitude
// with no division, in the units of "Noise profile" step 1.
//
// Order of the sums.  S2 and S1 of a carrier are sequential chains over its 75 products in symbol order, symbol 0 first, each begun
// at +0: s = s + term.  The order does not depend on launch geometry; ddp_carrier below is the definition.
//
// The square root is the IEEE one on both sides: g++ emits the correctly rounded instruction, and hipcc with the library's flags
// (no fast-math, correctly rounded divide/sqrt left at its default) expands __builtin_sqrtf to v_sqrt_f32 with the two fused
// residual tests of its neighbours and the scaling of small arguments, which is the correctly rounded root, denormals included.
//
// Limits.  The estimate under-reads where decisions fail (DESIGN 4.30 has the table: 0.98 of q at 12 dB carrier SNR and above, 0.8 at
// 6 dB, 0.5 at 0 dB, 0.3 at -10 dB), but stays monotone.  Amplitude that changes within the frame (fast fading) reads as noise.  The
// frame scale still rests on the power of the phase reference symbol; under a jammed band A is inflated, so A is no cure for the
// scale.  Mode I only.
#pragma once
#include <stdint.h>

#include "noise_profile_core.h"

namespace dabgpu {

constexpr int DDP_SYMBOLS = 75, DDP_CARRIERS = NP_CARRIERS;
constexpr float DDP_K1 = 0.009428090415820634f;       // the float nearest 1 / (75 sqrt(2))
constexpr float DDP_K75 = 1.0f / 75.0f;              // the float nearest 1 / 75 (a constant of the compiler, correctly rounded)

// step 1: one product joins the chains
DABGPU_HD inline float ddp_sum2(float s2, float re, float im) { return s2 + __builtin_fmaf(re, re, im * im); }
DABGPU_HD inline float ddp_sum1(float s1, float re, float im) { return s1 + (__builtin_fabsf(re) + __builtin_fabsf(im)); }

// step 2: A and Q of a carrier from its sums.  Q is 0 for a NaN and for a difference that is not positive.
DABGPU_HD inline float ddp_amplitude(float s1) { return s1 * DDP_K1; }
DABGPU_HD inline float ddp_noise(float s2, float a) {
    const float q = __builtin_sqrtf(s2 * DDP_K75) - a;
    return q > 0.0f ? q : 0.0f;
}

// steps 1 and 2 of carrier c of one frame on the host: dq = the frame's products [75][1536] complex float
inline void ddp_carrier(const float* dq, int c, float* Q, float* A) {
    float s2 = 0.0f, s1 = 0.0f;
    for (int s = 0; s < DDP_SYMBOLS; s++) {
        const float re = dq[2 * ((size_t)s * DDP_CARRIERS + c)], im = dq[2 * ((size_t)s * DDP_CARRIERS + c) + 1];
        s2 = ddp_sum2(s2, re, im);
        s1 = ddp_sum1(s1, re, im);
    }
    *A = ddp_amplitude(s1);
    *Q = ddp_noise(s2, *A);
}
inline void ddp_frame_carriers(const float* dq, float* Q, float* A) {
    for (int c = 0; c < DDP_CARRIERS; c++) {
        float q, a;
        ddp_carrier(dq, c, &q, &a);
        if (Q) Q[c] = q;
        if (A) A[c] = a;
    }
}

// one whole frame on the host.  sync_ok false: the frame is skipped and dq is not read.  False: skipped -- weights, mean, Q and A 0,
// the profile unchanged (0 without a previous one).  Every output may be null, profile_out may be profile_in.
inline bool ddp_frame(const float* dq, bool sync_ok, const uint32_t* exclude, const float* profile_in, float alpha, float* profile_out,
                      float* band_weight, float* mean_noise, float* carrier_noise, float* carrier_amplitude) {
    float Q[DDP_CARRIERS], A[DDP_CARRIERS];
    bool ok = false;
    if (sync_ok) {
        ddp_frame_carriers(dq, Q, A);
        ok = np_frame_bands(Q, exclude, profile_in, alpha, profile_out, band_weight, mean_noise);
    } else {
        for (int b = 0; b < NP_BANDS; b++) {
            if (profile_out) profile_out[b] = profile_in ? profile_in[b] : 0.0f;
            if (band_weight) band_weight[b] = 0.0f;
        }
        if (mean_noise) *mean_noise = 0.0f;
    }
    for (int c = 0; c < DDP_CARRIERS; c++) {
        if (carrier_noise) carrier_noise[c] = ok ? Q[c] : 0.0f;
        if (carrier_amplitude) carrier_amplitude[c] = ok ? A[c] : 0.0f;
    }
    return ok;
}

}  // namespace dabgpu
