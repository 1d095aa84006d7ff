// noise.hip -- the noise estimator on the device (include/dabgpu.h, "Noise estimate"): one frame's NULL window folded into 24 x 8 group
// energies, their floor calibrated into a noise power, the frame power of the phase reference symbol behind it, and the maximal-ratio
// weight of the two.  The arithmetic behind the transform is noise_core.h's (shared with the host forms and the tests' host model); the
// window's place, rotation, transform and powers are null_window.h's, the TII detector's front half.  The single-frame host form is
// host_round_trip.h's over this file's launch, its window check plan_prelude.h's.
//
// One 256-thread workgroup per frame.  Every thread first requests its eight samples of the phase reference symbol (sb_lane_sample order:
// the same four 16-byte or eight 8-byte loads as the window's), so that they travel while the window is transformed; its chain of eight
// fused steps and the wave's tree are the demodulator's, the four wave sums meet in LDS.  Threads 0 .. 191 own one (comb, group) each for
// the fold; wave 0 decides: lane c < 24 sorts comb c in registers, the 24 floor shares meet in LDS and every lane sums them in the same
// order, lane 0 writes the frame's words.  The group energies leave behind one more barrier, because a skipped frame writes zeros there too.
// LDS: 18432 + 8192 + 768 + 96 + 16 + 4 bytes; 84 VGPRs: five workgroups per CU, bounded by LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "host_round_trip.h"
#include "noise_core.h"
#include "null_window.h"
#include "plan_prelude.h"

namespace dabgpu {

struct noise_out { float *noise_power, *signal_power, *weight, *snr, *group_energy; uint32_t* valid; };

__device__ __forceinline__ void noise_store(const noise_out& o, size_t k, const dabgpu_noise_record& r) {
    if (o.noise_power) o.noise_power[k] = r.noise_power;
    if (o.signal_power) o.signal_power[k] = r.signal_power;
    if (o.weight) o.weight[k] = r.weight;
    if (o.snr) o.snr[k] = r.snr;
    if (o.valid) o.valid[k] = r.valid;
}

__global__ __launch_bounds__(256)
void noise_kernel(const f2* __restrict__ iq, size_t stride, long long null_offset, const dabgpu_sync_state* __restrict__ states,
                  const float* __restrict__ freq, float freq_all, const f2* __restrict__ tw, noise_out out)
{
    __shared__ __attribute__((aligned(16))) f2 A[4 * WAVE_PATCH];
    __shared__ float Pw[TII_FFT];
    __shared__ float ES[TII_ACC];
    __shared__ float shareS[TII_COMBS];
    __shared__ float sumS[4];
    __shared__ uint32_t okS;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t k = blockIdx.x;

    float f = freq_all;
    int fto = 0;
    if (!null_window_place(states, freq, k, null_offset, true, &f, &fto)) {             // refused: none of its samples is read
        if (t == 0) noise_store(out, k, dabgpu_noise_record{0.0f, 0.0f, 0.0f, 0.0f, 0u});
        if (out.group_energy && t < TII_ACC) out.group_energy[k * TII_ACC + t] = 0.0f;
        return;
    }
    const f2* const null0 = iq + k * stride + (null_offset + fto);
    const Fft2048Tw w = fft2048_twiddles(tw);

    // the phase reference symbol's useful part, not rotated
    const f2* const prs = null0 + NOISE_PRS_USEFUL;
    f4 q[4];
    if (((uintptr_t)prs & 15) == 0) {
#pragma unroll
        for (int j = 0; j < 4; j++) q[j] = *reinterpret_cast<const f4*>(prs + 2 * t + 512 * j);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) { const f2 a = prs[2 * t + 512 * j], b = prs[2 * t + 512 * j + 1]; q[j] = f4{a.x, a.y, b.x, b.y}; }
    }

    null_window_powers(null0 + TII_PREFIX, f, w, A, Pw, t);

    float acc = sb_power_first(q[0].x, q[0].y);
    acc = sb_power_next(acc, q[0].z, q[0].w);
#pragma unroll
    for (int j = 1; j < 4; j++) { acc = sb_power_next(acc, q[j].x, q[j].y); acc = sb_power_next(acc, q[j].z, q[j].w); }
    acc = wave_tree_sum(acc, lane);
    if (lane == 0) sumS[wave] = acc;
    if (t < TII_ACC) ES[t] = tii_fold([&](int bin) { return Pw[bin]; }, t >> 3, t & 7);
    __syncthreads();

    if (t < 64) {
        const int c = t < TII_COMBS ? t : 0;
        float v[TII_GROUPS], s[TII_GROUPS];
#pragma unroll
        for (int b = 0; b < TII_GROUPS; b++) v[b] = ES[TII_GROUPS * c + b];
        tii_sort8(v, s);
        if (t < TII_COMBS) shareS[t] = tii_comb_floor(s);
        wave_lds_fence();
        dabgpu_noise_record rec;
        const bool ok = noise_finish(tii_floor(shareS), sb_power_join(sumS[0], sumS[1], sumS[2], sumS[3]), &rec);
        if (t == 0) { noise_store(out, k, rec); okS = ok ? 1u : 0u; }
    }
    if (!out.group_energy) return;                                                    // (uniform)
    __syncthreads();
    if (t < TII_ACC) out.group_energy[k * TII_ACC + t] = okS ? ES[t] : 0.0f;
}

}  // namespace dabgpu

using namespace dabgpu;

static int noise_launch(dabgpu_ctx* c, const float* d_iq, size_t n, size_t stride, long long null_offset, const dabgpu_sync_state* d_states,
                        const float* d_freq, float freq_all, const noise_out& out, hipStream_t s) {
    hipLaunchKernelGGL(noise_kernel, dim3((unsigned)n), dim3(DABGPU_NOISE_THREADS), 0, s, reinterpret_cast<const f2*>(d_iq), stride, null_offset, d_states,
                       d_freq, freq_all, reinterpret_cast<const f2*>(c->d_tw), out);
    return dabgpu_check_hip(hipGetLastError(), "noise_kernel launch");
}

extern "C" {

int dabgpu_noise_estimate_frames(dabgpu_ctx* c, const float* d_iq, size_t n_frames, size_t stream_stride_samples, size_t null_offset_samples,
                                 const dabgpu_sync_state* d_states, const float* d_freq_offset, float* d_noise_power, float* d_signal_power,
                                 float* d_weight, float* d_snr, float* d_group_energy, uint32_t* d_valid, void* stream) {
    if (!c) { dabgpu_set_error("noise_estimate_frames: null context"); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_noise_geometry g;
    const int st = dabgpu_noise_plan(1, d_iq, n_frames, stream_stride_samples, null_offset_samples, d_states, d_freq_offset, d_noise_power,
                                     d_signal_power, d_weight, d_snr, d_group_energy, d_valid, &g);
    if (st) return st;
    DABGPU_BIND(c);
    return noise_launch(c, d_iq, g.grid, stream_stride_samples, (long long)null_offset_samples, d_states, d_freq_offset, 0.0f,
                        noise_out{d_noise_power, d_signal_power, d_weight, d_snr, d_group_energy, d_valid}, (hipStream_t)stream);
}

int dabgpu_noise_estimate_host_sync(dabgpu_ctx* c, const float* h_iq, size_t n_samples, size_t null_offset_samples, float freq_offset,
                                    int fine_time_offset, dabgpu_noise_record* out) {
    if (!c || !h_iq || !out) { dabgpu_set_error("noise_estimate_host_sync: null argument"); return DABGPU_ERR_INVALID_ARG; }
    *out = dabgpu_noise_record{};
    const char* const who = "noise_estimate_host_sync";
    const long long first = host_window_first(who, n_samples, null_offset_samples, fine_time_offset, true, 0, NOISE_REACH,
                                              "NULL and phase reference symbol at", "leave");
    if (first < 0) return DABGPU_ERR_INVALID_ARG;
    // only the frame's NULL and phase reference symbol travel; the block of small words is the record
    constexpr size_t W_END = sizeof(dabgpu_noise_record) / 4;
    const HostField fields[] = {{0, W_END, out, HOST_OUT}};
    return host_round_trip(c, who, HostPayload{SCR_HOST_IQ, h_iq + 2 * (size_t)first, (size_t)NOISE_REACH * 8, nullptr}, W_END, fields,
                           [&](float* d_iq, float* d_rec, hipStream_t s) {
                               return noise_launch(c, d_iq, 1, NOISE_REACH, 0, nullptr, nullptr, freq_offset,
                                                   noise_out{d_rec, d_rec + 1, d_rec + 2, d_rec + 3, nullptr, reinterpret_cast<uint32_t*>(d_rec + 4)}, s);
                           });
}

}  // extern "C"
