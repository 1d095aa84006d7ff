// noise_profile.hip -- the noise profile on the device (include/dabgpu.h, "Noise profile"): one frame's NULL window turned into the noise
// power of 128 bands of 12 carriers, smoothed against the caller's previous profile, and the bands' maximal-ratio weights.  The arithmetic
// behind the transform is noise_profile_core.h's (shared with the host forms and the tests' host model); the window's place, rotation,
// transform and powers are null_window.h's, the TII detector's and the noise estimator's front half; the band tail behind the powers is
// noise_profile_device.h's, shared with dd_profile.hip.  The single-frame host form is host_round_trip.h's over this file's launch and
// layout of the small block, its window check plan_prelude.h's.
//
// One 256-thread workgroup per frame.  Threads 0 .. 127 own one band each: they request the band's previous value before the window is
// transformed, so that it travels meanwhile, chain the band's twelve powers out of LDS, smooth, and fold the 128 values in the
// demodulator's wavefront tree; the two wave sums meet in LDS and every thread forms the same mean.  A band's thread reads its previous
// value before it writes the new one, so the profile may be updated in place.  Thread t copies the carrier powers t + 256 j.
// LDS: 18432 + 8192 + 8 bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "host_round_trip.h"
#include "noise_profile_device.h"
#include "null_window.h"
#include "plan_prelude.h"

namespace dabgpu {

struct profile_out { float *profile, *band_weight, *mean_noise, *carrier_power; uint32_t* valid; };

// a skipped frame: zeros everywhere, the profile kept (keep: this thread's band's previous value, 0 without one)
__device__ __forceinline__ void profile_skip(const profile_out& o, size_t k, int t, float keep) {
    np_band_skip(o, k, t, keep);
    if (o.carrier_power) {
#pragma unroll
        for (int j = 0; j < NP_CARRIERS / 256; j++) o.carrier_power[k * NP_CARRIERS + t + 256 * j] = 0.0f;
    }
    np_frame_store(o, k, t, 0.0f, 0u);
}

__global__ __launch_bounds__(256)
void noise_profile_kernel(const f2* __restrict__ iq, size_t stride, long long null_offset, const dabgpu_sync_state* __restrict__ states,
                          const float* __restrict__ freq, float freq_all, const f2* __restrict__ tw, const uint32_t* __restrict__ exclude,
                          const float* profile_in, float alpha, profile_out out)
{
    __shared__ __attribute__((aligned(16))) f2 A[4 * WAVE_PATCH];
    __shared__ float Pw[TII_FFT];
    __shared__ float sumS[2];
    const int t = threadIdx.x;
    const size_t k = blockIdx.x;
    const float prev = np_band_prev(profile_in, k, t);

    float f = freq_all;
    int fto = 0;
    if (!null_window_place(states, freq, k, null_offset, true, &f, &fto)) {             // refused: none of its samples is read
        profile_skip(out, k, t, prev);
        return;
    }
    const f2* const null0 = iq + k * stride + (null_offset + fto);
    const Fft2048Tw w = fft2048_twiddles(tw);

    null_window_powers(null0 + TII_PREFIX, f, w, A, Pw, t);

    float M;
    if (!np_band_finish([&](int c) { return Pw[np_carrier_bin(c)]; }, exclude, profile_in, prev, alpha, sumS, out, k, t, &M)) {      // (uniform)
        profile_skip(out, k, t, prev);
        return;
    }
    if (out.carrier_power) {
#pragma unroll
        for (int j = 0; j < NP_CARRIERS / 256; j++) {
            const int c = t + 256 * j;
            out.carrier_power[k * NP_CARRIERS + c] = Pw[np_carrier_bin(c)];
        }
    }
    np_frame_store(out, k, t, M, 1u);
}

}  // namespace dabgpu

using namespace dabgpu;

static int profile_launch(dabgpu_ctx* c, const float* d_iq, size_t n, size_t stride, long long null_offset, const dabgpu_sync_state* d_states,
                          const float* d_freq, float freq_all, const uint32_t* d_exclude, const float* d_profile_in, float alpha,
                          const profile_out& out, hipStream_t s) {
    hipLaunchKernelGGL(noise_profile_kernel, dim3((unsigned)n), dim3(DABGPU_NOISE_PROFILE_THREADS), 0, s, reinterpret_cast<const f2*>(d_iq), stride,
                       null_offset, d_states, d_freq, freq_all, reinterpret_cast<const f2*>(c->d_tw), d_exclude, d_profile_in, alpha, out);
    return dabgpu_check_hip(hipGetLastError(), "noise_profile_kernel launch");
}

extern "C" {

int dabgpu_noise_profile_frames(dabgpu_ctx* c, const float* d_iq, size_t n_frames, size_t stream_stride_samples, size_t null_offset_samples,
                                const dabgpu_sync_state* d_states, const float* d_freq_offset, const uint32_t* d_exclude, const float* d_profile_in,
                                float alpha, float* d_profile_out, float* d_band_weight, float* d_mean_noise, float* d_carrier_power,
                                uint32_t* d_valid, void* stream) {
    if (!c) { dabgpu_set_error("noise_profile_frames: null context"); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_noise_geometry g;
    const int st = dabgpu_noise_profile_plan(1, d_iq, n_frames, stream_stride_samples, null_offset_samples, d_states, d_freq_offset, d_exclude,
                                             d_profile_in, alpha, d_profile_out, d_band_weight, d_mean_noise, d_carrier_power, d_valid, &g);
    if (st) return st;
    DABGPU_BIND(c);
    return profile_launch(c, d_iq, g.grid, stream_stride_samples, (long long)null_offset_samples, d_states, d_freq_offset, 0.0f, d_exclude,
                          d_profile_in, alpha, profile_out{d_profile_out, d_band_weight, d_mean_noise, d_carrier_power, d_valid}, (hipStream_t)stream);
}

int dabgpu_noise_profile_host_sync(dabgpu_ctx* c, const float* h_iq, size_t n_samples, size_t null_offset_samples, float freq_offset,
                                   int fine_time_offset, const uint32_t* h_exclude, float* h_profile, float alpha, float* h_band_weight,
                                   float* h_mean_noise, float* h_carrier_power, uint32_t* h_valid) {
    if (!c || !h_iq) { dabgpu_set_error("noise_profile_host_sync: null argument"); return DABGPU_ERR_INVALID_ARG; }
    if (h_valid) *h_valid = 0u;
    if (!np_alpha_ok(alpha)) { dabgpu_set_error("noise_profile_host_sync: alpha %g outside (0, 1]", (double)alpha); return DABGPU_ERR_INVALID_ARG; }
    const char* const who = "noise_profile_host_sync";
    const long long first = host_window_first(who, n_samples, null_offset_samples, fine_time_offset, true, 0, NP_NULL, "the NULL at", "leaves");
    if (first < 0) return DABGPU_ERR_INVALID_ARG;
    // only the frame's NULL travels; behind it one block of small words: exclusion, profile, weights, mean, valid, carrier powers
    constexpr size_t W_EX = 0, W_PROF = W_EX + NP_EXCLUDE_WORDS, W_BW = W_PROF + NP_BANDS, W_MEAN = W_BW + NP_BANDS, W_VALID = W_MEAN + 1,
                     W_CP = W_VALID + 1, W_END = W_CP + NP_CARRIERS;
    const HostField fields[] = {{W_EX, NP_EXCLUDE_WORDS, const_cast<uint32_t*>(h_exclude), HOST_IN}, {W_PROF, NP_BANDS, h_profile, HOST_IN | HOST_OUT},
                                {W_BW, NP_BANDS, h_band_weight, HOST_OUT},                         {W_CP, NP_CARRIERS, h_carrier_power, HOST_OUT},
                                {W_MEAN, 1, h_mean_noise, HOST_LATE},                              {W_VALID, 1, h_valid, HOST_LATE}};
    return host_round_trip(c, who, HostPayload{SCR_HOST_IQ, h_iq + 2 * (size_t)first, (size_t)NP_NULL * 8, nullptr}, W_END, fields,
                           [&](float* d_iq, float* d_small, hipStream_t s) {
                               return profile_launch(c, d_iq, 1, NP_NULL, 0, nullptr, nullptr, freq_offset,
                                                     h_exclude ? reinterpret_cast<const uint32_t*>(d_small + W_EX) : nullptr,
                                                     h_profile ? d_small + W_PROF : nullptr, alpha,
                                                     profile_out{d_small + W_PROF, d_small + W_BW, d_small + W_MEAN, h_carrier_power ? d_small + W_CP : nullptr,
                                                                 reinterpret_cast<uint32_t*>(d_small + W_VALID)}, s);
                           });
}

}  // extern "C"
