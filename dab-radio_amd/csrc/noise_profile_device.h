// noise_profile_device.h -- the band tail that the noise profile (noise_profile.hip) and the decision-directed profile (dd_profile.hip)
// share on the device: 1536 carrier values in LDS turned into 128 band values, smoothed against the caller's previous profile, their mean
// and the bands' weights (steps 3 to 5 of include/dabgpu.h, "Noise profile"; the arithmetic is noise_profile_core.h's).  One 256-thread
// workgroup per frame, threads 0 .. 127 own one band each.  Out is the kernel's output record: profile, band_weight, mean_noise, valid
// are read here, the carrier outputs stay with the kernel.
#pragma once
#include "noise_profile_core.h"
#include "ofdm_device.h"

namespace dabgpu {

// the band's previous value, requested before the kernel's long loads (profile_in may be out.profile: read here, written at the end by
// the same thread); 0 without one
__device__ __forceinline__ float np_band_prev(const float* profile_in, size_t k, int t) {
    return (profile_in != nullptr && t < NP_BANDS) ? profile_in[k * NP_BANDS + t] : 0.0f;
}

// the frame's two words (thread 0)
template <class Out> __device__ __forceinline__ void np_frame_store(const Out& o, size_t k, int t, float mean, uint32_t valid) {
    if (t == 0) {
        if (o.mean_noise) o.mean_noise[k] = mean;
        if (o.valid) o.valid[k] = valid;
    }
}

// the band half of a skipped frame: the profile kept (keep: np_band_prev), weight 0.  The kernel zeroes its carrier outputs behind it and
// ends with np_frame_store(.., 0, 0)
template <class Out> __device__ __forceinline__ void np_band_skip(const Out& o, size_t k, int t, float keep) {
    if (t < NP_BANDS) {
        if (o.profile) o.profile[k * NP_BANDS + t] = keep;
        if (o.band_weight) o.band_weight[k * NP_BANDS + t] = 0.0f;
    }
}

// power(c): carrier c's value, complete in LDS; sumS: two floats in LDS.  The band's twelve values chained, smoothed, the 128 folded in the
// demodulator's wavefront tree, the two wave sums joined by every thread alike.  False (uniform): the mean is not usable, nothing is
// written (the kernel skips the frame).  True: profile and weights are stored, *mean is the frame's; the kernel stores its carrier outputs
// and ends with np_frame_store(.., *mean, 1)
template <class Power, class Out>
__device__ __forceinline__ bool np_band_finish(Power power, const uint32_t* __restrict__ exclude, const float* profile_in, float prev, float alpha,
                                               float* sumS, const Out& o, size_t k, int t, float* mean) {
    const int lane = t & 63, wave = t >> 6;
    float n = 0.0f;
    if (t < NP_BANDS) {
        const float m = np_band_measure(power, t, np_band_mask(exclude, t));
        n = np_smooth(m, profile_in != nullptr, prev, alpha);
    }
    if (wave < 2) {                                                                    // (uniform per wave)
        const float s = wave_tree_sum(n, lane);
        if (lane == 0) sumS[wave] = s;
    }
    __syncthreads();
    const float M = np_mean_join(sumS[0], sumS[1]);
    *mean = M;
    if (!np_mean_ok(M)) return false;
    if (t < NP_BANDS) {
        if (o.profile) o.profile[k * NP_BANDS + t] = n;
        if (o.band_weight) o.band_weight[k * NP_BANDS + t] = np_weight(n, M);
    }
    return true;
}

}  // namespace dabgpu
