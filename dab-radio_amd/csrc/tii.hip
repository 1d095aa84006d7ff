// tii.hip -- the TII detector on the device (include/dabgpu.h, "TII"): the NULL symbol's comb spectrum of a bank of receivers, folded into
// 24 x 8 group energies per receiver, accumulated over frames and decided against a noise floor.  The arithmetic behind the transform is
// tii_core.h's (shared with the tests' host model); the transform is ofdm_fft_lds.h's, the PLL ofdm_device.h's.
//
// One 256-thread workgroup per receiver.  The window's place, rotation, transform and the 2048 powers in LDS are null_window.h's (shared
// with noise.hip and noise_profile.hip), the process call's window checks plan_prelude.h's (shared with their planners); threads 0 .. 191 own one (comb, group) each for the fold
// and the accumulate; wave 0 decides: lane c < 24 sorts comb c in registers, the 24 floor shares meet in LDS and every lane sums them in
// the same order, the active lanes compact their records in comb order through a ballot.  LDS: 18432 + 8192 + 768 + 96 bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "null_window.h"
#include "plan_prelude.h"

namespace dabgpu {

__global__ __launch_bounds__(256)
void tii_kernel(const f2* __restrict__ iq, size_t stride, long long null_offset, const dabgpu_sync_state* __restrict__ states,
                const float* __restrict__ freq, float freq_all, int time_all, const f2* __restrict__ tw, float* __restrict__ acc,
                uint32_t* __restrict__ frames, int decide, float threshold, dabgpu_tii_record* __restrict__ results, uint32_t* __restrict__ counts)
{
    __shared__ __attribute__((aligned(16))) f2 A[4 * WAVE_PATCH];
    __shared__ float Pw[TII_FFT];
    __shared__ float accS[TII_ACC];
    __shared__ float shareS[TII_COMBS];
    const int t = threadIdx.x;
    const size_t rx = blockIdx.x;

    float f = freq_all;
    int fto = time_all;
    if (!null_window_place(states, freq, rx, null_offset, false, &f, &fto)) return;  // receiver skipped: nothing of it is touched
    const f2* win = iq + rx * stride + (null_offset + fto + TII_PREFIX);
    const Fft2048Tw w = fft2048_twiddles(tw);
    null_window_powers(win, f, w, A, Pw, t);
    if (t < TII_ACC) {
        const float e = tii_fold([&](int bin) { return Pw[bin]; }, t >> 3, t & 7);
        const float a = acc[rx * TII_ACC + t] + e;
        acc[rx * TII_ACC + t] = a;
        accS[t] = a;
    }
    if (t == 0) frames[rx] = frames[rx] + 1u;
    if (!decide) return;
    __syncthreads();
    if (t >= 64) return;

    const int c = t < TII_COMBS ? t : 0;
    float v[TII_GROUPS], s[TII_GROUPS];
#pragma unroll
    for (int b = 0; b < TII_GROUPS; b++) v[b] = accS[TII_GROUPS * c + b];
    tii_sort8(v, s);
    if (t < TII_COMBS) shareS[t] = tii_comb_floor(s);
    wave_lds_fence();
    const float n = tii_floor(shareS);
    dabgpu_tii_record rec;
    bool active = false;
    if (t < TII_COMBS && n > 0.0f) active = tii_comb_decide(c, v, s, threshold * n, n, tii_reciprocal(n), &rec);
    const unsigned long long on = __ballot(active);
    if (active) results[rx * TII_COMBS + __popcll(on & ((1ull << t) - 1ull))] = rec;
    if (t == 0) counts[rx] = (uint32_t)__popcll(on);
}

}  // namespace dabgpu

using namespace dabgpu;

struct dabgpu_tii_bank {
    dabgpu_ctx* ctx = nullptr;
    size_t n = 0;
    float threshold = DABGPU_TII_DEFAULT_THRESHOLD;
    DeviceBuffer<> d_mem;                       // one allocation: accumulators [n][192] | frame counts [n]
    float* d_acc = nullptr;                     // (into d_mem)
    uint32_t* d_frames = nullptr;
    // host form (one receiver): the window's samples, records and count
    DeviceBuffer<> d_host_iq, d_host_res;
};

static int tii_launch(dabgpu_tii_bank* b, const float* d_iq, size_t stride, long long null_offset, const dabgpu_sync_state* d_states, const float* d_freq,
                      float freq_all, int time_all, int decide, dabgpu_tii_record* d_results, uint32_t* d_counts, hipStream_t s) {
    hipLaunchKernelGGL(tii_kernel, dim3((unsigned)b->n), dim3(256), 0, s, reinterpret_cast<const f2*>(d_iq), stride, null_offset, d_states, d_freq,
                       freq_all, time_all, reinterpret_cast<const f2*>(b->ctx->d_tw), b->d_acc, b->d_frames, decide, b->threshold, d_results, d_counts);
    return dabgpu_check_hip(hipGetLastError(), "tii_kernel launch");
}

extern "C" {

int dabgpu_tii_bank_create(dabgpu_ctx* c, size_t n, const dabgpu_tii_cfg* cfg, dabgpu_tii_bank** out) {
    if (!c || !out) { dabgpu_set_error("tii_bank_create: null context / result"); return DABGPU_ERR_INVALID_ARG; }
    *out = nullptr;
    if (n == 0 || n > ((size_t)1 << 20)) { dabgpu_set_error("tii_bank_create: %zu receivers (1 .. 1048576)", n); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_tii_cfg def;
    dabgpu_tii_cfg_default(&def);
    if (!cfg) cfg = &def;
    if (!(cfg->threshold >= 1.0f) || !(cfg->threshold <= 1.0e6f)) {
        dabgpu_set_error("tii_bank_create: threshold %g outside 1 .. 1e6", (double)cfg->threshold); return DABGPU_ERR_INVALID_ARG;
    }
    dabgpu_tii_bank* b = new (std::nothrow) dabgpu_tii_bank;
    if (!b) return DABGPU_ERR_HIP;
    b->ctx = c; b->n = n; b->threshold = cfg->threshold;
    auto fail = [&](int status) { dabgpu_tii_bank_destroy(b); return status; };
    int st;
    if ((st = dabgpu_bind_device(c))) return fail(st);
    const size_t acc_bytes = n * TII_ACC * sizeof(float), bytes = acc_bytes + n * sizeof(uint32_t);
    if ((st = b->d_mem.alloc(bytes, "hipMalloc(tii bank)"))) return fail(st);
    b->d_acc = static_cast<float*>(b->d_mem.get());
    b->d_frames = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(b->d_mem.get()) + acc_bytes);
    if ((st = b->d_host_res.alloc(TII_COMBS * sizeof(dabgpu_tii_record) + 16, "hipMalloc(tii results)"))) return fail(st);
    if ((st = b->d_host_iq.alloc((size_t)TII_FFT * 8, "hipMalloc(tii window)"))) return fail(st);
    if ((st = dabgpu_check_hip(hipMemsetAsync(b->d_acc, 0, bytes, c->stream), "hipMemsetAsync(tii bank)"))) return fail(st);
    if ((st = dabgpu_check_hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize(tii_bank_create)"))) return fail(st);
    *out = b;
    return DABGPU_OK;
}

void dabgpu_tii_bank_destroy(dabgpu_tii_bank* b) {
    if (!dabgpu_destroy_begin(b, b ? b->ctx : nullptr)) return;
    delete b;
}

int dabgpu_tii_bank_reset(dabgpu_tii_bank* b, void* stream) {
    if (!b) { dabgpu_set_error("tii_bank_reset: null bank"); return DABGPU_ERR_INVALID_ARG; }
    DABGPU_BIND(b->ctx);
    return dabgpu_check_hip(hipMemsetAsync(b->d_acc, 0, b->n * (TII_ACC * sizeof(float) + sizeof(uint32_t)), (hipStream_t)stream),
                            "hipMemsetAsync(tii_bank_reset)");
}

int dabgpu_tii_bank_process(dabgpu_tii_bank* b, const float* d_iq, size_t stride, size_t null_offset, const dabgpu_sync_state* d_states,
                            const float* d_freq_offset, int decide, dabgpu_tii_record* d_results, uint32_t* d_counts, void* stream) {
    if (!b) { dabgpu_set_error("tii_bank_process: null bank"); return DABGPU_ERR_INVALID_ARG; }
    const char* const who = "tii_bank_process";
    if (plan_input(who, plan_or(d_iq), 8, "samples", "d_iq") || plan_null_reach(who, stride, null_offset, DABGPU_NB_NULL_PERIOD, d_states != nullptr))
        return DABGPU_ERR_INVALID_ARG;
    if (decide && (!d_results || !d_counts)) { dabgpu_set_error("%s: a decision needs d_results and d_counts", who); return DABGPU_ERR_INVALID_ARG; }
    if (plan_aligned(who, plan_or(d_states, d_freq_offset, d_results, d_counts), 4, "records, offsets, results and counts")) return DABGPU_ERR_INVALID_ARG;
    DABGPU_BIND(b->ctx);
    return tii_launch(b, d_iq, stride, (long long)null_offset, d_states, d_freq_offset, 0.0f, 0, decide, d_results, d_counts, (hipStream_t)stream);
}

int dabgpu_tii_bank_process_host_sync(dabgpu_tii_bank* b, const float* h_iq, size_t n_samples, size_t null_offset, float freq_offset,
                                      int fine_time_offset, int decide, dabgpu_tii_record* h_results, uint32_t* h_count) {
    if (!b) { dabgpu_set_error("tii_bank_process_host_sync: null bank"); return DABGPU_ERR_INVALID_ARG; }
    if (b->n != 1) { dabgpu_set_error("tii_bank_process_host_sync: a bank of %zu receivers (the host form serves one)", b->n); return DABGPU_ERR_INVALID_ARG; }
    if (!h_iq) { dabgpu_set_error("tii_bank_process_host_sync: null samples"); return DABGPU_ERR_INVALID_ARG; }
    if (decide && (!h_results || !h_count)) {
        dabgpu_set_error("tii_bank_process_host_sync: a decision needs h_results and h_count"); return DABGPU_ERR_INVALID_ARG;
    }
    const long long first = host_window_first("tii_bank_process_host_sync", n_samples, null_offset, fine_time_offset, false, TII_PREFIX, TII_FFT,
                                              "the window at", "+ 608 leaves");
    if (first < 0) return DABGPU_ERR_INVALID_ARG;
    dabgpu_ctx* c = b->ctx;
    DABGPU_BIND(c);
    DABGPU_HOST_LOCK(c);
    int st = DABGPU_OK;
    hipStream_t s = c->stream;
    // only the window travels
    const size_t bytes = (size_t)TII_FFT * 8;
    dabgpu_tii_record* d_res = static_cast<dabgpu_tii_record*>(b->d_host_res.get());
    uint32_t* d_cnt = reinterpret_cast<uint32_t*>(d_res + TII_COMBS);
    DABGPU_CK(hipMemcpyAsync(b->d_host_iq.get(), h_iq + 2 * (size_t)first, bytes, hipMemcpyHostToDevice, s));
    if ((st = tii_launch(b, static_cast<const float*>(b->d_host_iq.get()), TII_FFT, -(long long)TII_PREFIX, nullptr, nullptr, freq_offset, 0, decide, d_res,
                         d_cnt, s)))
        return st;
    if (decide) {
        DABGPU_CK(hipMemcpyAsync(h_count, d_cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        DABGPU_CK(hipMemcpyAsync(h_results, d_res, TII_COMBS * sizeof(dabgpu_tii_record), hipMemcpyDeviceToHost, s));
    }
    DABGPU_CK(hipStreamSynchronize(s));
    return DABGPU_OK;
}

int dabgpu_tii_bank_read(dabgpu_tii_bank* b, float* h_acc, uint32_t* h_frames, void* stream) {
    if (!b) { dabgpu_set_error("tii_bank_read: null bank"); return DABGPU_ERR_INVALID_ARG; }
    DABGPU_BIND(b->ctx);
    int st = DABGPU_OK;
    hipStream_t s = (hipStream_t)stream;
    if (h_acc) DABGPU_CK(hipMemcpyAsync(h_acc, b->d_acc, b->n * TII_ACC * sizeof(float), hipMemcpyDeviceToHost, s));
    if (h_frames) DABGPU_CK(hipMemcpyAsync(h_frames, b->d_frames, b->n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    DABGPU_CK(hipStreamSynchronize(s));
    return DABGPU_OK;
}

}  // extern "C"
