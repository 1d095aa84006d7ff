// clock.hip -- the sampling-clock tracker on the device (include/dabgpu.h, "Sampling-clock tracker"): an estimator that turns one frame's
// 75 x 1536 DQPSK products into the slope of their phase ramp over the carriers, and a de-rotator that takes the ramp out again.  The
// arithmetic is clock_core.h's (shared with the host forms and the tests' host model).  The single-frame host form is
// host_round_trip.h's: both launches are its launch callable, the de-rotated products its payload coming back.
//
// Estimator: one 256-thread workgroup per frame, one pass over the products (921,600 bytes a frame), a few words written.  Thread t owns
// the float4 positions t, t + 256 and t + 512 of every row, as in sym_profile.hip; the lag partner of position j is position j + 16 of the
// same row and comes by a second 16-byte load, which the cache serves (the line was fetched for a neighbour 256 bytes on).  Staging the
// row in LDS instead would put a barrier into every row; exchanging registers serves 48 lanes of 64 and leaves the rest to load anyway.
// Three rows = eighteen loads are in flight per thread: with five rows the loads alone take 120 registers, three waves fit a SIMD and
// the call ran at 0.44 of the memory rate; with three rows (85 registers, five waves) at 0.73, beside the symbol profile's 0.75
// (profiles/tx/bench_clock.md).  A thread chains its folded products over the whole frame, so the wave's tree and the one barrier come
// once per frame.  LDS: 48 bytes.
//
// De-rotator: memory-bound, 1.84 MB a frame in and out.  A workgroup computes the 1536 rotations of its frame once into LDS (12 KB) and
// then walks its run of rows: thread t rotates the positions t, t + 256, t + 512 of each row, one 16-byte load, one 16-byte LDS read and
// one 16-byte store per position.  The frame's rows are split into runs (the combiner's symbols_per_block rule) so that a small batch
// still spreads over the chip; every element is read and written by the same thread, so in place is safe, and no result depends on the
// split.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "host_round_trip.h"
#include "ofdm_device.h"
#include "clock_core.h"

namespace dabgpu {

typedef float clk_f4 __attribute__((ext_vector_type(4)));
constexpr int CLK_THREADS = (int)DABGPU_CLOCK_THREADS, CLK_OWN = CLK_ROW_F4 / CLK_THREADS, CLK_RUN = 3, CLK_ROT_RUN = 4;
static_assert(CLK_THREADS == CLK_OWNERS && CLK_OWN == 3 && CLK_SYMBOLS % CLK_RUN == 0, "three positions a thread, runs of three rows");

struct clk_est_out { int64_t *slope, *residual; float* corr; uint32_t* valid; };

__device__ __forceinline__ void clk_store(const clk_est_out& o, size_t k, const clk_update& u, float re, float im) {
    if (o.slope) o.slope[k] = u.slope;
    if (o.residual) o.residual[k] = u.residual;
    if (o.corr) { o.corr[2 * k] = u.valid ? re : 0.0f; o.corr[2 * k + 1] = u.valid ? im : 0.0f; }
    if (o.valid) o.valid[k] = u.valid ? 1u : 0u;
}

__global__ __launch_bounds__(256)
void clock_estimate_kernel(const clk_f4* __restrict__ dq, const dabgpu_sync_state* __restrict__ sync, const int64_t* slope_in, float gain,
                           clk_est_out out)
{
    __shared__ float partS[CLK_WAVES][2];
    __shared__ uint32_t dropS[CLK_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t k = blockIdx.x;
    const int64_t s_in = slope_in ? slope_in[k] : 0;

    // a frame the synchroniser refused left stale products behind: none is read (the same for the whole workgroup)
    if (sync && !sync[k].sync_valid) {
        if (t == 0) clk_store(out, k, clk_update{s_in, 0, false}, 0.0f, 0.0f);
        return;
    }
    const int64_t prior_slope = clk_clamp(s_in);
    const bool prior = prior_slope != 0;
    const chf2 rot = prior ? clk_prior(prior_slope) : chf2{1.0f, 0.0f};
    bool own[CLK_OWN];
#pragma unroll
    for (int j = 0; j < CLK_OWN; j++) own[j] = clk_position_pairs(t + CLK_THREADS * j);

    // steps 1 to 4: this thread's chain over the frame
    const clk_f4* const p = dq + k * ((size_t)CLK_SYMBOLS * CLK_ROW_F4) + t;
    clk_sum a{0.0f, 0.0f, 0u};
    for (int s0 = 0; s0 < CLK_SYMBOLS; s0 += CLK_RUN) {
        clk_f4 lo[CLK_RUN][CLK_OWN], hi[CLK_RUN][CLK_OWN];
#pragma unroll
        for (int r = 0; r < CLK_RUN; r++)
#pragma unroll
            for (int j = 0; j < CLK_OWN; j++) {
                if (!own[j]) continue;                                                 // (a position without a partner loads nothing)
                const clk_f4* const q = p + (size_t)(s0 + r) * CLK_ROW_F4 + CLK_THREADS * j;
                lo[r][j] = q[0];
                hi[r][j] = q[CLK_LAG_F4];
            }
#pragma unroll
        for (int r = 0; r < CLK_RUN; r++)
#pragma unroll
            for (int j = 0; j < CLK_OWN; j++) {
                if (!own[j]) continue;
                clk_add(a, prior, rot, chf2{lo[r][j].x, lo[r][j].y}, chf2{hi[r][j].x, hi[r][j].y});
                clk_add(a, prior, rot, chf2{lo[r][j].z, lo[r][j].w}, chf2{hi[r][j].z, hi[r][j].w});
            }
    }
    const float sum = wave_tree_sum_pair(a.re, a.im);                                  // lane 0: the sum of re, lane 32: the sum of im
    uint32_t n = a.dropped;
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) n += (uint32_t)__shfl_xor((int)n, h);
    if (lane == 0) { partS[wave][0] = sum; dropS[wave] = n; }
    if (lane == 32) partS[wave][1] = sum;
    __syncthreads();

    // steps 5 and 6
    if (t == 0) {
        const float re = clk_join(partS[0][0], partS[1][0], partS[2][0], partS[3][0]);
        const float im = clk_join(partS[0][1], partS[1][1], partS[2][1], partS[3][1]);
        clk_store(out, k, clk_frame_update(re, im, dropS[0] + dropS[1] + dropS[2] + dropS[3], s_in, gain), re, im);
    }
}

// in and out may be the same buffer: no __restrict__ on either
__global__ __launch_bounds__(256)
void clock_derotate_kernel(const clk_f4* in, clk_f4* out, const dabgpu_sync_state* __restrict__ sync, const int64_t* __restrict__ slope,
                           uint32_t rows_per_block, uint32_t runs_per_frame)
{
    __shared__ clk_f4 rotS[CLK_ROW_F4];
    const int t = threadIdx.x;
    const size_t k = blockIdx.x / runs_per_frame;
    const int row0 = (int)((blockIdx.x % runs_per_frame) * rows_per_block);
    const int row1 = min(row0 + (int)rows_per_block, CLK_SYMBOLS);
    if (sync && !sync[k].sync_valid) return;                                           // (uniform) neither read nor written
    const int64_t s = slope[k];
    const size_t base = k * ((size_t)CLK_SYMBOLS * CLK_ROW_F4) + (size_t)t;
    if (s == 0) {                                                                      // (uniform) a copy bit for bit; in place: nothing
        if (in == out) return;
        for (int row = row0; row < row1; row++)
#pragma unroll
            for (int j = 0; j < CLK_OWN; j++) {
                const size_t i = base + (size_t)row * CLK_ROW_F4 + CLK_THREADS * j;
                out[i] = in[i];
            }
        return;
    }
#pragma unroll
    for (int j = 0; j < CLK_OWN; j++) {
        const int c = 2 * (t + CLK_THREADS * j);
        const chf2 r0 = clk_rotation(s, clk_carrier_number(c)), r1 = clk_rotation(s, clk_carrier_number(c + 1));
        rotS[t + CLK_THREADS * j] = clk_f4{r0.re, r0.im, r1.re, r1.im};
    }
    __syncthreads();
    clk_f4 rot[CLK_OWN];
#pragma unroll
    for (int j = 0; j < CLK_OWN; j++) rot[j] = rotS[t + CLK_THREADS * j];
    for (int r0 = row0; r0 < row1; r0 += CLK_ROT_RUN) {
        clk_f4 v[CLK_ROT_RUN][CLK_OWN];
#pragma unroll
        for (int r = 0; r < CLK_ROT_RUN; r++)
#pragma unroll
            for (int j = 0; j < CLK_OWN; j++)
                if (r0 + r < row1) v[r][j] = in[base + (size_t)(r0 + r) * CLK_ROW_F4 + CLK_THREADS * j];
#pragma unroll
        for (int r = 0; r < CLK_ROT_RUN; r++)
#pragma unroll
            for (int j = 0; j < CLK_OWN; j++) {
                if (r0 + r >= row1) continue;
                const chf2 a = clk_rotate(chf2{rot[j].x, rot[j].y}, chf2{v[r][j].x, v[r][j].y});
                const chf2 b = clk_rotate(chf2{rot[j].z, rot[j].w}, chf2{v[r][j].z, v[r][j].w});
                out[base + (size_t)(r0 + r) * CLK_ROW_F4 + CLK_THREADS * j] = clk_f4{a.re, a.im, b.re, b.im};
            }
    }
}

}  // namespace dabgpu

using namespace dabgpu;

static int clk_launch_estimate(const float* d_dqpsk, size_t n, const dabgpu_sync_state* d_sync, const int64_t* d_slope_in, float gain,
                               const clk_est_out& out, hipStream_t s) {
    hipLaunchKernelGGL(clock_estimate_kernel, dim3((unsigned)n), dim3(DABGPU_CLOCK_THREADS), 0, s, reinterpret_cast<const clk_f4*>(d_dqpsk), d_sync,
                       d_slope_in, gain, out);
    return dabgpu_check_hip(hipGetLastError(), "clock_estimate_kernel launch");
}
static int clk_launch_derotate(const float* d_in, float* d_out, const dabgpu_diversity_geometry& g, const dabgpu_sync_state* d_sync,
                               const int64_t* d_slope, hipStream_t s) {
    hipLaunchKernelGGL(clock_derotate_kernel, dim3(g.grid), dim3(g.threads), 0, s, reinterpret_cast<const clk_f4*>(d_in),
                       reinterpret_cast<clk_f4*>(d_out), d_sync, d_slope, g.symbols_per_block, g.runs_per_frame);
    return dabgpu_check_hip(hipGetLastError(), "clock_derotate_kernel launch");
}

extern "C" {

int dabgpu_clock_estimate_frames(dabgpu_ctx* c, const float* d_dqpsk, size_t n_frames, const dabgpu_sync_state* d_sync, const int64_t* d_slope_in,
                                 float gain, int64_t* d_slope_out, int64_t* d_residual, float* d_corr, uint32_t* d_valid, void* stream) {
    if (!c) { dabgpu_set_error("clock_estimate_frames: null context"); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_noise_geometry g;
    const int st = dabgpu_clock_estimate_plan(1, d_dqpsk, n_frames, d_sync, d_slope_in, gain, d_slope_out, d_residual, d_corr, d_valid, &g);
    if (st) return st;
    DABGPU_BIND(c);
    return clk_launch_estimate(d_dqpsk, g.grid, d_sync, d_slope_in, gain, clk_est_out{d_slope_out, d_residual, d_corr, d_valid}, (hipStream_t)stream);
}

int dabgpu_clock_derotate_frames_split(dabgpu_ctx* c, const float* d_dqpsk_in, float* d_dqpsk_out, size_t n_frames, const dabgpu_sync_state* d_sync,
                                       const int64_t* d_slope, int symbols_per_block, void* stream) {
    if (!c) { dabgpu_set_error("clock_derotate_frames: null context"); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_diversity_geometry g;
    const int st = dabgpu_clock_derotate_plan(1, d_dqpsk_in, d_dqpsk_out, n_frames, d_sync, d_slope, symbols_per_block, &g);
    if (st) return st;
    DABGPU_BIND(c);
    return clk_launch_derotate(d_dqpsk_in, d_dqpsk_out, g, d_sync, d_slope, (hipStream_t)stream);
}

int dabgpu_clock_derotate_frames(dabgpu_ctx* c, const float* d_dqpsk_in, float* d_dqpsk_out, size_t n_frames, const dabgpu_sync_state* d_sync,
                                 const int64_t* d_slope, void* stream) {
    return dabgpu_clock_derotate_frames_split(c, d_dqpsk_in, d_dqpsk_out, n_frames, d_sync, d_slope, 0, stream);
}

int dabgpu_clock_track_host_sync(dabgpu_ctx* c, const float* h_dqpsk_in, float* h_dqpsk_out, int64_t* slope, float gain, float* h_corr,
                                 uint32_t* h_valid) {
    if (!c || !h_dqpsk_in || !slope) { dabgpu_set_error("clock_track_host_sync: null argument"); return DABGPU_ERR_INVALID_ARG; }
    if (!clk_gain_ok(gain)) { dabgpu_set_error("clock_track_host_sync: gain %g outside (0, 1]", (double)gain); return DABGPU_ERR_INVALID_ARG; }
    if (h_valid) *h_valid = 0u;
    // the frame's products (de-rotated in place, and back when the caller wants them), and one block of small words: the slope (eight
    // bytes, aligned), the sum, valid and a word that pads the block to whole slope words; all of it comes back behind the synchronise
    constexpr size_t W_SLOPE = 0, W_CORR = W_SLOPE + 2, W_VALID = W_CORR + 2, W_PAD = W_VALID + 1, W_END = W_PAD + 1;
    const HostField fields[] = {{W_SLOPE, 2, slope, HOST_IN | HOST_LATE}, {W_CORR, 2, h_corr, HOST_LATE}, {W_VALID, 1, h_valid, HOST_LATE},
                                {W_PAD, 1, nullptr, HOST_LATE}};
    return host_round_trip(c, "clock_track_host_sync",
                           HostPayload{SCR_HOST_DQPSK, h_dqpsk_in, (size_t)CLK_SYMBOLS * CLK_CARRIERS * 2 * sizeof(float), h_dqpsk_out}, W_END, fields,
                           [&](float* d_dq, float* d_small, hipStream_t s) {
                               int64_t* const d_slope = reinterpret_cast<int64_t*>(d_small + W_SLOPE);
                               int st = clk_launch_estimate(d_dq, 1, nullptr, d_slope, gain,
                                                            clk_est_out{d_slope, nullptr, d_small + W_CORR, reinterpret_cast<uint32_t*>(d_small + W_VALID)}, s);
                               if (st || !h_dqpsk_out) return st;
                               dabgpu_diversity_geometry g;
                               if ((st = dabgpu_clock_derotate_plan(1, d_dq, d_dq, 1, nullptr, d_slope, 0, &g))) return st;
                               return clk_launch_derotate(d_dq, d_dq, g, nullptr, d_slope, s);
                           });
}

}  // extern "C"
