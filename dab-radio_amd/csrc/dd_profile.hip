// dd_profile.hip -- the decision-directed noise profile on the device (include/dabgpu.h, "Decision-directed noise profile"): one frame's
// 75 x 1536 DQPSK products turned into a noise power per carrier (rms of the products minus their mean projected amplitude), that into
// the noise power of 128 bands of 12 carriers, smoothed against the caller's previous profile, and the bands' maximal-ratio weights.
// The carrier arithmetic is dd_profile_core.h's, everything behind it noise_profile_core.h's (both shared with the host forms and the
// tests' host model), on the device through noise_profile_device.h, the band tail shared with noise_profile.hip.  The single-frame host
// form is host_round_trip.h's over this file's launch and layout of the small block.
//
// One 256-thread workgroup per frame; the call is one pass over the products (921,600 bytes a frame) and writes about 0.5 kB.  Thread t
// owns the carrier pairs t, t + 256 and t + 512 (carriers 2 p, 2 p + 1; a pair never straddles a band): one 16-byte load per pair and
// symbol, adjacent lanes adjacent addresses, five symbols = fifteen loads in flight per thread.  The two sums of a carrier are chains in
// symbol order held in registers.  Q goes to LDS once; threads 0 .. 127 own one band each as in noise_profile.hip: they request the
// band's previous value before the products are read, chain the band's twelve values out of LDS, smooth, and fold the 128 values in the
// demodulator's wavefront tree; the two wave sums meet in LDS and every thread forms the same mean.  A band's thread reads its
// previous value before it writes the new one, so the profile may be updated in place.  LDS: 6144 + 8 bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "dd_profile_core.h"
#include "host_round_trip.h"
#include "noise_profile_device.h"

namespace dabgpu {

typedef float ddp_f4 __attribute__((ext_vector_type(4)));
typedef float ddp_f2 __attribute__((ext_vector_type(2)));
constexpr int DDP_THREADS = (int)DABGPU_DD_PROFILE_THREADS, DDP_PAIRS = DDP_CARRIERS / 2, DDP_OWN = DDP_PAIRS / DDP_THREADS, DDP_RUN = 5;
static_assert(DDP_OWN * DDP_THREADS == DDP_PAIRS && DDP_SYMBOLS % DDP_RUN == 0 && NP_BAND_CARRIERS % 2 == 0, "three pairs a thread, runs of five symbols");

struct ddp_out { float *profile, *band_weight, *mean_noise, *carrier_noise, *carrier_amplitude; uint32_t* valid; };

// a skipped frame: zeros everywhere, the profile kept (keep: this thread's band's previous value, 0 without one)
__device__ __forceinline__ void ddp_skip(const ddp_out& o, size_t k, int t, float keep) {
    np_band_skip(o, k, t, keep);
#pragma unroll
    for (int j = 0; j < DDP_OWN; j++) {
        const size_t at = k * DDP_PAIRS + t + DDP_THREADS * j;
        if (o.carrier_noise) reinterpret_cast<ddp_f2*>(o.carrier_noise)[at] = ddp_f2{0.0f, 0.0f};
        if (o.carrier_amplitude) reinterpret_cast<ddp_f2*>(o.carrier_amplitude)[at] = ddp_f2{0.0f, 0.0f};
    }
    np_frame_store(o, k, t, 0.0f, 0u);
}

__global__ __launch_bounds__(256)
void dd_profile_kernel(const ddp_f4* __restrict__ dq, const dabgpu_sync_state* __restrict__ sync, const uint32_t* __restrict__ exclude,
                       const float* profile_in, float alpha, ddp_out out)
{
    __shared__ __attribute__((aligned(8))) float Qs[DDP_CARRIERS];
    __shared__ float sumS[2];
    const int t = threadIdx.x;
    const size_t k = blockIdx.x;
    const float prev = np_band_prev(profile_in, k, t);

    // a frame the synchroniser refused left stale products behind: none is read (the same for the whole workgroup)
    if (sync && !sync[k].sync_valid) {
        ddp_skip(out, k, t, prev);
        return;
    }

    // steps 1 and 2: the chains of this thread's six carriers
    const ddp_f4* const p = dq + k * ((size_t)DDP_SYMBOLS * DDP_PAIRS) + t;
    float s2[2 * DDP_OWN], s1[2 * DDP_OWN];
#pragma unroll
    for (int i = 0; i < 2 * DDP_OWN; i++) s2[i] = s1[i] = 0.0f;
    for (int s0 = 0; s0 < DDP_SYMBOLS; s0 += DDP_RUN) {
        ddp_f4 v[DDP_RUN][DDP_OWN];
#pragma unroll
        for (int r = 0; r < DDP_RUN; r++)
#pragma unroll
            for (int j = 0; j < DDP_OWN; j++) v[r][j] = p[(size_t)(s0 + r) * DDP_PAIRS + DDP_THREADS * j];
#pragma unroll
        for (int r = 0; r < DDP_RUN; r++)
#pragma unroll
            for (int j = 0; j < DDP_OWN; j++) {
                s2[2 * j] = ddp_sum2(s2[2 * j], v[r][j].x, v[r][j].y);
                s1[2 * j] = ddp_sum1(s1[2 * j], v[r][j].x, v[r][j].y);
                s2[2 * j + 1] = ddp_sum2(s2[2 * j + 1], v[r][j].z, v[r][j].w);
                s1[2 * j + 1] = ddp_sum1(s1[2 * j + 1], v[r][j].z, v[r][j].w);
            }
    }
    float Q[2 * DDP_OWN], A[2 * DDP_OWN];
#pragma unroll
    for (int i = 0; i < 2 * DDP_OWN; i++) {
        A[i] = ddp_amplitude(s1[i]);
        Q[i] = ddp_noise(s2[i], A[i]);
    }
#pragma unroll
    for (int j = 0; j < DDP_OWN; j++) reinterpret_cast<ddp_f2*>(Qs)[t + DDP_THREADS * j] = ddp_f2{Q[2 * j], Q[2 * j + 1]};
    __syncthreads();

    // steps 3 to 5: noise_profile_core.h over Q
    float M;
    if (!np_band_finish([&](int c) { return Qs[c]; }, exclude, profile_in, prev, alpha, sumS, out, k, t, &M)) {                        // (uniform)
        ddp_skip(out, k, t, prev);
        return;
    }
#pragma unroll
    for (int j = 0; j < DDP_OWN; j++) {
        const size_t at = k * DDP_PAIRS + t + DDP_THREADS * j;
        if (out.carrier_noise) reinterpret_cast<ddp_f2*>(out.carrier_noise)[at] = ddp_f2{Q[2 * j], Q[2 * j + 1]};
        if (out.carrier_amplitude) reinterpret_cast<ddp_f2*>(out.carrier_amplitude)[at] = ddp_f2{A[2 * j], A[2 * j + 1]};
    }
    np_frame_store(out, k, t, M, 1u);
}

}  // namespace dabgpu

using namespace dabgpu;

static int ddp_launch(const float* d_dqpsk, size_t n, const dabgpu_sync_state* d_sync, const uint32_t* d_exclude, const float* d_profile_in,
                      float alpha, const ddp_out& out, hipStream_t s) {
    hipLaunchKernelGGL(dd_profile_kernel, dim3((unsigned)n), dim3(DABGPU_DD_PROFILE_THREADS), 0, s, reinterpret_cast<const ddp_f4*>(d_dqpsk), d_sync,
                       d_exclude, d_profile_in, alpha, out);
    return dabgpu_check_hip(hipGetLastError(), "dd_profile_kernel launch");
}

extern "C" {

int dabgpu_dd_profile_frames(dabgpu_ctx* c, const float* d_dqpsk, size_t n_frames, const dabgpu_sync_state* d_sync, const uint32_t* d_exclude,
                             const float* d_profile_in, float alpha, float* d_profile_out, float* d_band_weight, float* d_mean_noise,
                             float* d_carrier_noise, float* d_carrier_amplitude, uint32_t* d_valid, void* stream) {
    if (!c) { dabgpu_set_error("dd_profile_frames: null context"); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_noise_geometry g;
    const int st = dabgpu_dd_profile_plan(1, d_dqpsk, n_frames, d_sync, d_exclude, d_profile_in, alpha, d_profile_out, d_band_weight, d_mean_noise,
                                          d_carrier_noise, d_carrier_amplitude, d_valid, &g);
    if (st) return st;
    DABGPU_BIND(c);
    return ddp_launch(d_dqpsk, g.grid, d_sync, d_exclude, d_profile_in, alpha,
                      ddp_out{d_profile_out, d_band_weight, d_mean_noise, d_carrier_noise, d_carrier_amplitude, d_valid}, (hipStream_t)stream);
}

int dabgpu_dd_profile_host_sync(dabgpu_ctx* c, const float* h_dqpsk, const uint32_t* h_exclude, float* h_profile, float alpha, float* h_band_weight,
                                float* h_mean_noise, float* h_carrier_noise, float* h_carrier_amplitude, uint32_t* h_valid) {
    if (!c || !h_dqpsk) { dabgpu_set_error("dd_profile_host_sync: null argument"); return DABGPU_ERR_INVALID_ARG; }
    if (h_valid) *h_valid = 0u;
    if (!np_alpha_ok(alpha)) { dabgpu_set_error("dd_profile_host_sync: alpha %g outside (0, 1]", (double)alpha); return DABGPU_ERR_INVALID_ARG; }
    // the frame's products, and one block of small words: exclusion, profile, weights, mean, valid, carrier noise, carrier amplitude
    constexpr size_t W_EX = 0, W_PROF = W_EX + NP_EXCLUDE_WORDS, W_BW = W_PROF + NP_BANDS, W_MEAN = W_BW + NP_BANDS, W_VALID = W_MEAN + 1,
                     W_Q = W_VALID + 1, W_A = W_Q + DDP_CARRIERS, W_END = W_A + DDP_CARRIERS;
    static_assert(W_Q % 2 == 0 && W_A % 2 == 0, "carrier outputs are stored in pairs");
    const HostField fields[] = {{W_EX, NP_EXCLUDE_WORDS, const_cast<uint32_t*>(h_exclude), HOST_IN}, {W_PROF, NP_BANDS, h_profile, HOST_IN | HOST_OUT},
                                {W_BW, NP_BANDS, h_band_weight, HOST_OUT},                         {W_Q, DDP_CARRIERS, h_carrier_noise, HOST_OUT},
                                {W_A, DDP_CARRIERS, h_carrier_amplitude, HOST_OUT},                {W_MEAN, 1, h_mean_noise, HOST_LATE},
                                {W_VALID, 1, h_valid, HOST_LATE}};
    return host_round_trip(c, "dd_profile_host_sync", HostPayload{SCR_HOST_DQPSK, h_dqpsk, (size_t)DDP_SYMBOLS * DDP_CARRIERS * 2 * sizeof(float), nullptr},
                           W_END, fields, [&](float* d_dq, float* d_small, hipStream_t s) {
                               return ddp_launch(d_dq, 1, nullptr, h_exclude ? reinterpret_cast<const uint32_t*>(d_small + W_EX) : nullptr,
                                                 h_profile ? d_small + W_PROF : nullptr, alpha,
                                                 ddp_out{d_small + W_PROF, d_small + W_BW, d_small + W_MEAN, h_carrier_noise ? d_small + W_Q : nullptr,
                                                         h_carrier_amplitude ? d_small + W_A : nullptr, reinterpret_cast<uint32_t*>(d_small + W_VALID)}, s);
                           });
}

}  // extern "C"
