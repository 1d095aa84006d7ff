// sym_profile.hip -- the symbol noise profile on the device (include/dabgpu.h, "Symbol noise profile"): one frame's 75 x 1536 DQPSK
// products turned into one noise figure per product row (the quadrature spread across the decision diagonal, lifted by the row's excess
// rms where decisions fail) and the rows' relative weights against the frame's median.  The arithmetic is sym_profile_core.h's (shared
// with the host forms and the tests' host model).  The single-frame host form is host_round_trip.h's over this file's launch.
//
// One 256-thread workgroup per frame; the call is one pass over the products (921,600 bytes a frame) and writes about 0.6 kB.  Thread t
// owns the carrier pairs t, t + 256 and t + 512 of every row, as in dd_profile.hip: one 16-byte load per pair and row, adjacent lanes
// adjacent addresses, five rows = fifteen loads in flight per thread.  Per row a thread chains its six carriers into three sums, the
// wave folds them in the demodulator's wavefront tree (S1 and SD share the paired tree) and leaves three partials in LDS; there is no
// barrier inside the row loop.  Threads 0 .. 74 then own one row each: they join the four wave partials, take the two roots, rank-count
// the three medians through LDS and store.  LDS: 3600 + 900 + 12 bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "host_round_trip.h"
#include "ofdm_device.h"
#include "sym_profile_core.h"

namespace dabgpu {

typedef float syp_f4 __attribute__((ext_vector_type(4)));
constexpr int SYP_THREADS = (int)DABGPU_SYM_PROFILE_THREADS, SYP_PAIRS = SYP_CARRIERS / 2, SYP_OWN = SYP_PAIRS / SYP_THREADS, SYP_RUN = 5;
static_assert(SYP_THREADS == SYP_OWNERS && SYP_OWN == 3 && SYP_SYMBOLS % SYP_RUN == 0 && SYP_SYMBOLS <= SYP_THREADS, "three pairs a thread, runs of five rows");

struct syp_out { float *symbol_weight, *symbol_noise, *ref_noise; uint32_t* valid; };

// a skipped frame: zeros everywhere
__device__ __forceinline__ void syp_skip(const syp_out& o, size_t k, int t) {
    if (t < SYP_SYMBOLS) {
        if (o.symbol_weight) o.symbol_weight[k * SYP_SYMBOLS + t] = 0.0f;
        if (o.symbol_noise) o.symbol_noise[k * SYP_SYMBOLS + t] = 0.0f;
    }
    if (t == 0) {
        if (o.ref_noise) o.ref_noise[k] = 0.0f;
        if (o.valid) o.valid[k] = 0u;
    }
}

// the median of the 75 values in x: every row's thread counts its rank, the one of rank 37 publishes its value (uniform barriers)
__device__ __forceinline__ float syp_median_lds(const float* x, float* slot, int t) {
    if (t < SYP_SYMBOLS && syp_rank([&](int j) { return x[j]; }, t) == SYP_MEDIAN_RANK) *slot = x[t];
    __syncthreads();
    return *slot;
}

__global__ __launch_bounds__(256)
void sym_profile_kernel(const syp_f4* __restrict__ dq, const dabgpu_sync_state* __restrict__ sync, syp_out out)
{
    __shared__ float partS[SYP_SYMBOLS][SYP_WAVES][3];
    __shared__ float figS[3][SYP_SYMBOLS];
    __shared__ float medS[3];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t k = blockIdx.x;

    // a frame the synchroniser refused left stale products behind: none is read (the same for the whole workgroup)
    if (sync && !sync[k].sync_valid) {
        syp_skip(out, k, t);
        return;
    }

    // step 1: per row, this thread's six carriers, then the wave's tree
    const syp_f4* const p = dq + k * ((size_t)SYP_SYMBOLS * SYP_PAIRS) + t;
    for (int s0 = 0; s0 < SYP_SYMBOLS; s0 += SYP_RUN) {
        syp_f4 v[SYP_RUN][SYP_OWN];
#pragma unroll
        for (int r = 0; r < SYP_RUN; r++)
#pragma unroll
            for (int j = 0; j < SYP_OWN; j++) v[r][j] = p[(size_t)(s0 + r) * SYP_PAIRS + SYP_THREADS * j];
#pragma unroll
        for (int r = 0; r < SYP_RUN; r++) {
            syp_sums a{0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < SYP_OWN; j++) {
                syp_add(a, v[r][j].x, v[r][j].y);
                syp_add(a, v[r][j].z, v[r][j].w);
            }
            const float s1d = wave_tree_sum_pair(a.s1, a.sd);                          // lane 0: the sum of s1, lane 32: the sum of sd
            const float s2 = wave_tree_sum(a.s2, lane);
            float* const slot = partS[s0 + r][wave];
            if (lane == 0) { slot[0] = s1d; slot[2] = s2; }
            if (lane == 32) slot[1] = s1d;
        }
    }
    __syncthreads();

    // steps 2 and 3: a row per thread
    float qa = 0.0f, R = 0.0f;
    if (t < SYP_SYMBOLS) {
        const float(*const ps)[3] = partS[t];
        const syp_row f = syp_row_figures(syp_join(ps[0][0], ps[1][0], ps[2][0], ps[3][0]), syp_join(ps[0][1], ps[1][1], ps[2][1], ps[3][1]),
                                          syp_join(ps[0][2], ps[1][2], ps[2][2], ps[3][2]));
        qa = f.qa; R = f.R;
        figS[0][t] = qa;
        figS[1][t] = R;
    }
    __syncthreads();
    if (t < SYP_SYMBOLS) {
        if (syp_rank([&](int j) { return figS[0][j]; }, t) == SYP_MEDIAN_RANK) medS[0] = qa;
        if (syp_rank([&](int j) { return figS[1][j]; }, t) == SYP_MEDIAN_RANK) medS[1] = R;
    }
    __syncthreads();
    float q = 0.0f;
    if (t < SYP_SYMBOLS) {
        q = syp_noise(qa, R, medS[0], medS[1]);
        figS[2][t] = q;
    }
    __syncthreads();
    // step 4
    const float q_ref = syp_median_lds(figS[2], &medS[2], t);
    if (!syp_ref_ok(q_ref)) {                                                          // (uniform)
        syp_skip(out, k, t);
        return;
    }
    if (t < SYP_SYMBOLS) {
        if (out.symbol_weight) out.symbol_weight[k * SYP_SYMBOLS + t] = syp_weight(q, q_ref);
        if (out.symbol_noise) out.symbol_noise[k * SYP_SYMBOLS + t] = q;
    }
    if (t == 0) {
        if (out.ref_noise) out.ref_noise[k] = q_ref;
        if (out.valid) out.valid[k] = 1u;
    }
}

}  // namespace dabgpu

using namespace dabgpu;

static int syp_launch(const float* d_dqpsk, size_t n, const dabgpu_sync_state* d_sync, const syp_out& out, hipStream_t s) {
    hipLaunchKernelGGL(sym_profile_kernel, dim3((unsigned)n), dim3(DABGPU_SYM_PROFILE_THREADS), 0, s, reinterpret_cast<const syp_f4*>(d_dqpsk), d_sync, out);
    return dabgpu_check_hip(hipGetLastError(), "sym_profile_kernel launch");
}

extern "C" {

int dabgpu_sym_profile_frames(dabgpu_ctx* c, const float* d_dqpsk, size_t n_frames, const dabgpu_sync_state* d_sync, float* d_symbol_weight,
                              float* d_symbol_noise, float* d_ref_noise, uint32_t* d_valid, void* stream) {
    if (!c) { dabgpu_set_error("sym_profile_frames: null context"); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_noise_geometry g;
    const int st = dabgpu_sym_profile_plan(1, d_dqpsk, n_frames, d_sync, d_symbol_weight, d_symbol_noise, d_ref_noise, d_valid, &g);
    if (st) return st;
    DABGPU_BIND(c);
    return syp_launch(d_dqpsk, g.grid, d_sync, syp_out{d_symbol_weight, d_symbol_noise, d_ref_noise, d_valid}, (hipStream_t)stream);
}

int dabgpu_sym_profile_host_sync(dabgpu_ctx* c, const float* h_dqpsk, float* h_symbol_weight, float* h_symbol_noise, float* h_ref_noise,
                                 uint32_t* h_valid) {
    if (!c || !h_dqpsk) { dabgpu_set_error("sym_profile_host_sync: null argument"); return DABGPU_ERR_INVALID_ARG; }
    if (h_valid) *h_valid = 0u;
    // the frame's products, and one block of small words: weights, noise, reference, valid
    constexpr size_t W_V = 0, W_Q = W_V + SYP_SYMBOLS, W_REF = W_Q + SYP_SYMBOLS, W_VALID = W_REF + 1, W_END = W_VALID + 1;
    const HostField fields[] = {{W_V, SYP_SYMBOLS, h_symbol_weight, HOST_OUT}, {W_Q, SYP_SYMBOLS, h_symbol_noise, HOST_OUT},
                                {W_REF, 1, h_ref_noise, HOST_LATE},            {W_VALID, 1, h_valid, HOST_LATE}};
    return host_round_trip(c, "sym_profile_host_sync", HostPayload{SCR_HOST_DQPSK, h_dqpsk, (size_t)SYP_SYMBOLS * SYP_CARRIERS * 2 * sizeof(float), nullptr},
                           W_END, fields, [&](float* d_dq, float* d_small, hipStream_t s) {
                               return syp_launch(d_dq, 1, nullptr, syp_out{d_small + W_V, d_small + W_Q, d_small + W_REF,
                                                                           reinterpret_cast<uint32_t*>(d_small + W_VALID)}, s);
                           });
}

}  // extern "C"
