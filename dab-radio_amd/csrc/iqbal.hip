// iqbal.hip -- the IQ balance bank on the device (include/dabgpu.h, "IQ balance"): one widely-linear map per sample, z = a y + b conj(y) + c,
// and in the same pass the five moments of the raw input from which the DC term and the image coefficient are solved blindly, in a bank
// of independent streams.  Every arithmetic step is iqbal_core.h's; this file is where the samples come from and go to.
//
// The work kernel: one 256-thread workgroup per (stream, tile of DABGPU_IQBAL_TILE = 1024 samples), tiles aligned to ABSOLUTE sample
// numbers as the blanker's.  A thread owns samples 2 t, 2 t + 1 and 512 + 2 t, 513 + 2 t of the tile: two 16-byte loads where the call's
// position is even, two non-temporal 16-byte stores (or 4-byte stores of u8 pairs); a call that starts at an odd position, and the partial
// tiles at either end of an APPLY call, go sample by sample.  The stream's parameters and record are read through pointers that are the
// same for the whole workgroup (scalar loads).  With MEASURE the thread adds its four samples' terms (index bits 0 and 9 of iqbal_core.h's
// tree), the wave sums them as a butterfly over its 64 lanes (bits 1 .. 6), the four waves meet in LDS (bits 7, 8), and thread 0 writes the
// tile's 32 bytes to the scratch, [tile][stream] so that the fold's lanes read neighbouring records.
// The fold-and-solve kernel: one lane per stream, the call's tiles in increasing order, no atomics anywhere: the tile order is the
// contract.  The position advance follows it.  A MEASURE call that finds the position off a tile edge does nothing in all three kernels
// but count itself in the records.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <new>
#include <vector>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "iqbal_core.h"
#include "channel_device.h"
#include "signal_bank.h"

namespace dabgpu {

static_assert(IQB_TILE == 2 * 256 * 2, "a tile is two passes of 256 threads x 2 samples");
static_assert(sizeof(dabgpu_iqbal_record) == 104 && sizeof(dabgpu_iqbal_stream) == 40, "record / stream layout");

template <int OUT>
__global__ __launch_bounds__(256)
void iqbal_kernel(const dabgpu_iqbal_stream* __restrict__ params, const dabgpu_iqbal_record* __restrict__ rec, const uint64_t* __restrict__ d_pos,
                  const chf2* in, size_t in_stride, uint32_t n, int tiles, uint8_t* out, size_t out_stride_bytes, float scale, uint32_t flags,
                  float* __restrict__ scratch, uint32_t n_streams)
{
    __shared__ float wave_sum[4][IQB_TILE_FLOATS];
    const int t = threadIdx.x;
    const uint32_t s = blockIdx.x / (uint32_t)tiles, tile = blockIdx.x % (uint32_t)tiles;
    const bool measure = (flags & DABGPU_IQBAL_MEASURE) != 0, apply = (flags & DABGPU_IQBAL_APPLY) != 0;
    const uint64_t pos = *d_pos;
    if (measure && (pos & (uint64_t)(IQB_TILE - 1))) return;                 // refused: nothing is written (the fold kernel counts it)
    const uint64_t T0 = (pos & ~(uint64_t)(IQB_TILE - 1)) + (uint64_t)tile * IQB_TILE;   // absolute number of the tile's first sample
    const uint64_t rel0 = T0 - pos;                                          // -1023 .. 0 (as unsigned) for tile 0
    const int lo = (tile == 0) ? (int)(pos & (uint64_t)(IQB_TILE - 1)) : 0;  // samples of this tile inside the call: tile-local [lo, hi)
    const int64_t left = (int64_t)n - (int64_t)rel0;
    if (left <= lo) return;                                                  // a tile past the call's end
    const int hi = left < IQB_TILE ? (int)left : IQB_TILE;
    const chf2* x = in + (size_t)s * in_stride;
    const bool even = (pos & 1) == 0;

    chf2 y[2][2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const int n0 = 2 * 256 * c + 2 * t;                                  // tile-local number of the thread's first sample
        y[c][0] = y[c][1] = chf2{0.0f, 0.0f};
        if (n0 + 2 <= lo || n0 >= hi) continue;
        const size_t o = (size_t)(rel0 + (uint64_t)n0);                      // sample of n0 in the call (meaningful where n0 >= lo)
        if (even && n0 >= lo && n0 + 2 <= hi) {
            const ch_f4 v = *reinterpret_cast<const ch_f4*>(x + o);
            y[c][0] = chf2{v.x, v.y}; y[c][1] = chf2{v.z, v.w};
        } else {
#pragma unroll
            for (int h = 0; h < 2; h++)
                if (n0 + h >= lo && n0 + h < hi) y[c][h] = ch_ld(x + o + h);
        }
    }

    if (measure) {                                                           // (whole tiles only: lo = 0, hi = 1024)
        iqb_moments a = iqb_add(iqb_add(iqb_terms(y[0][0]), iqb_terms(y[0][1])), iqb_add(iqb_terms(y[1][0]), iqb_terms(y[1][1])));
#pragma unroll
        for (int k = 0; k < IQB_MOMENTS; k++) {
#pragma unroll
            for (int lane = 1; lane < 64; lane <<= 1) a.m[k] = a.m[k] + __shfl_xor(a.m[k], lane);
            if ((t & 63) == 0) wave_sum[t >> 6][k] = a.m[k];
        }
        __syncthreads();
        if (t == 0) {
            float r[IQB_TILE_FLOATS];
#pragma unroll
            for (int k = 0; k < IQB_TILE_FLOATS; k++)
                r[k] = k < IQB_MOMENTS ? (wave_sum[0][k] + wave_sum[1][k]) + (wave_sum[2][k] + wave_sum[3][k]) : 0.0f;
            ch_f4* dst = reinterpret_cast<ch_f4*>(scratch + ((size_t)tile * n_streams + s) * IQB_TILE_FLOATS);
            dst[0] = ch_f4{r[0], r[1], r[2], r[3]};
            dst[1] = ch_f4{r[4], r[5], r[6], r[7]};
        }
    }
    if (!apply) return;

    const dabgpu_iqbal_stream& P = params[s];
    const bool copy = P.mode == DABGPU_IQBAL_OFF;
    const iqb_coef K = iqb_stream_coef(P, rec[s]);
    uint8_t* orow = out + (size_t)s * out_stride_bytes;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const int n0 = 2 * 256 * c + 2 * t;
        if (n0 + 2 <= lo || n0 >= hi) continue;
        chf2 z[2];
#pragma unroll
        for (int h = 0; h < 2; h++) z[h] = copy ? y[c][h] : iqb_map(K, y[c][h]);
        const size_t o = (size_t)(rel0 + (uint64_t)n0);
        const bool whole = even && n0 >= lo && n0 + 2 <= hi;
        if (OUT == DABGPU_IQ_RAW_F32L) {
            if (whole) {
                __builtin_nontemporal_store(ch_f4{z[0].re, z[0].im, z[1].re, z[1].im}, reinterpret_cast<ch_f4*>(orow + 8 * o));
            } else {
#pragma unroll
                for (int h = 0; h < 2; h++)
                    if (n0 + h >= lo && n0 + h < hi) *reinterpret_cast<ch_f2v*>(orow + 8 * (o + h)) = ch_f2v{z[h].re, z[h].im};
            }
        } else {
            uint32_t b[2];
#pragma unroll
            for (int h = 0; h < 2; h++) b[h] = ch_u8(z[h].re, scale) | (ch_u8(z[h].im, scale) << 8);
            if (whole) {
                *reinterpret_cast<uint32_t*>(orow + 2 * o) = b[0] | (b[1] << 16);
            } else {
#pragma unroll
                for (int h = 0; h < 2; h++)
                    if (n0 + h >= lo && n0 + h < hi) *reinterpret_cast<uint16_t*>(orow + 2 * (o + h)) = (uint16_t)b[h];
            }
        }
    }
}

// one lane per stream: the call's tiles into the record, in increasing tile number, then the solve
__global__ __launch_bounds__(64)
void iqbal_fold_kernel(const dabgpu_iqbal_stream* __restrict__ params, dabgpu_iqbal_record* __restrict__ rec, const uint64_t* __restrict__ d_pos,
                       const float* __restrict__ scratch, uint32_t n_streams, int tiles)
{
    const uint32_t s = blockIdx.x * 64u + threadIdx.x;
    if (s >= n_streams) return;
    if (*d_pos & (uint64_t)(IQB_TILE - 1)) { rec[s].calls_refused++; return; }
    if (params[s].mode != DABGPU_IQBAL_TRACK) return;
    dabgpu_iqbal_record R = rec[s];
    iqb_fold_and_solve(params[s], R, tiles, [&](int j) { return scratch + ((size_t)j * n_streams + s) * IQB_TILE_FLOATS; });
    rec[s] = R;
}

__global__ void iqbal_reset_kernel(dabgpu_iqbal_record* rec, uint32_t n_streams) {
    const uint32_t s = blockIdx.x * 64u + threadIdx.x;
    if (s < n_streams) iqb_record_reset(rec[s]);
}

// the advance of a call that the device did not refuse
__global__ void iqbal_advance_kernel(uint64_t* pos, uint64_t n, uint32_t flags) {
    if ((flags & DABGPU_IQBAL_MEASURE) && (*pos & (uint64_t)(IQB_TILE - 1))) return;
    *pos += n;
}

}  // namespace dabgpu

using namespace dabgpu;

struct dabgpu_iqbal_bank : SignalBank {           // d_mem: position (16 bytes) | records | parameters | tile scratch
    size_t n = 0;
    dabgpu_iqbal_geometry geom = {};
    dabgpu_iqbal_record* d_rec = nullptr;
    dabgpu_iqbal_stream* d_params = nullptr;
    float* d_scratch = nullptr;
};

static size_t iqb_round16(size_t v) { return (v + 15) & ~(size_t)15; }

static int iqb_launch(dabgpu_iqbal_bank* b, const float* d_in, size_t in_stride, size_t n, void* d_out, int out_format, size_t out_stride_bytes,
                      float u8_scale, uint32_t flags, hipStream_t s) {
    const bool measure = (flags & DABGPU_IQBAL_MEASURE) != 0;
    const int tiles = (int)(measure ? n / IQB_TILE : n / IQB_TILE + 2);      // (an APPLY call may start and end inside a tile)
    const unsigned grid = (unsigned)((size_t)tiles * b->n);
    const chf2* in = reinterpret_cast<const chf2*>(d_in);
#define IQB_GO(OUT)                                                                                                                          \
    hipLaunchKernelGGL((iqbal_kernel<OUT>), dim3(grid), dim3(256), 0, s, b->d_params, b->d_rec, b->d_pos, in, in_stride, (uint32_t)n, tiles, \
                       static_cast<uint8_t*>(d_out), out_stride_bytes, u8_scale, flags, b->d_scratch, (uint32_t)b->n)
    if (out_format == DABGPU_IQ_RAW_U8) IQB_GO(DABGPU_IQ_RAW_U8); else IQB_GO(DABGPU_IQ_RAW_F32L);
#undef IQB_GO
    if (measure)
        hipLaunchKernelGGL(iqbal_fold_kernel, dim3((unsigned)((b->n + 63) / 64)), dim3(64), 0, s, b->d_params, b->d_rec, b->d_pos, b->d_scratch,
                           (uint32_t)b->n, tiles);
    hipLaunchKernelGGL(iqbal_advance_kernel, dim3(1), dim3(1), 0, s, b->d_pos, (uint64_t)n, flags);
    return dabgpu_check_hip(hipGetLastError(), "iqbal_kernel launch");
}

extern "C" {

int dabgpu_iqbal_bank_create(dabgpu_ctx* c, size_t n_streams, const dabgpu_iqbal_stream* h_params, size_t max_samples_per_call,
                             dabgpu_iqbal_bank** out) {
    if (!c || !out) { dabgpu_set_error("iqbal_bank_create: null context / result"); return DABGPU_ERR_INVALID_ARG; }
    *out = nullptr;
    dabgpu_iqbal_geometry g;
    int st = dabgpu_host_iqbal_plan("iqbal_bank_create", h_params, n_streams, max_samples_per_call, &g);
    if (st) return st;
    dabgpu_iqbal_bank* b = new (std::nothrow) dabgpu_iqbal_bank;
    if (!b) return DABGPU_ERR_HIP;
    b->ctx = c; b->n = n_streams; b->geom = g;
    auto fail = [&](int status) { dabgpu_iqbal_bank_destroy(b); return status; };
    if ((st = dabgpu_bind_device(c))) return fail(st);
    const size_t rec_bytes = iqb_round16(n_streams * sizeof(dabgpu_iqbal_record)), par_bytes = iqb_round16(n_streams * sizeof(dabgpu_iqbal_stream));
    uint8_t* payload;
    if ((st = sb_alloc(b, rec_bytes + par_bytes + (size_t)g.scratch_bytes, "iqbal", &payload))) return fail(st);
    b->d_rec = reinterpret_cast<dabgpu_iqbal_record*>(payload);
    b->d_params = reinterpret_cast<dabgpu_iqbal_stream*>(payload + rec_bytes);
    b->d_scratch = reinterpret_cast<float*>(payload + rec_bytes + par_bytes);
    if ((st = dabgpu_stage_h2d(c, b->d_params, h_params, n_streams * sizeof(dabgpu_iqbal_stream), c->stream))) return fail(st);
    if ((st = dabgpu_check_hip(hipMemsetAsync(b->d_scratch, 0, (size_t)g.scratch_bytes, c->stream), "hipMemsetAsync(iqbal scratch)"))) return fail(st);
    hipLaunchKernelGGL(iqbal_reset_kernel, dim3((unsigned)((n_streams + 63) / 64)), dim3(64), 0, c->stream, b->d_rec, (uint32_t)n_streams);
    if ((st = dabgpu_check_hip(hipGetLastError(), "iqbal_reset_kernel launch"))) return fail(st);
    if ((st = dabgpu_check_hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize(iqbal_bank_create)"))) return fail(st);
    *out = b;
    return DABGPU_OK;
}

void dabgpu_iqbal_bank_destroy(dabgpu_iqbal_bank* b) {
    if (!dabgpu_destroy_begin(b, b ? b->ctx : nullptr)) return;
    delete b;
}

int dabgpu_iqbal_bank_set_params(dabgpu_iqbal_bank* b, const dabgpu_iqbal_stream* h_params, void* stream) {
    if (!b) { dabgpu_set_error("iqbal_bank_set_params: null bank"); return DABGPU_ERR_INVALID_ARG; }
    const int st = dabgpu_host_iqbal_plan("iqbal_bank_set_params", h_params, b->n, (size_t)b->geom.tiles_per_call * IQB_TILE, nullptr);
    if (st) return st;
    DABGPU_BIND(b->ctx);
    return dabgpu_stage_h2d(b->ctx, b->d_params, h_params, b->n * sizeof(dabgpu_iqbal_stream), (hipStream_t)stream);
}

int dabgpu_iqbal_bank_seek(dabgpu_iqbal_bank* b, uint64_t position, void* stream) {
    return sb_seek(b, "iqbal_bank_seek", position, (uint64_t)DABGPU_IQBAL_MAX_POSITION, "2^62", stream);
}

int dabgpu_iqbal_bank_reset(dabgpu_iqbal_bank* b, void* stream) {
    if (!b) { dabgpu_set_error("iqbal_bank_reset: null bank"); return DABGPU_ERR_INVALID_ARG; }
    DABGPU_BIND(b->ctx);
    hipLaunchKernelGGL(iqbal_reset_kernel, dim3((unsigned)((b->n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, b->d_rec, (uint32_t)b->n);
    return dabgpu_check_hip(hipGetLastError(), "iqbal_reset_kernel launch");
}

int dabgpu_iqbal_bank_apply(dabgpu_iqbal_bank* b, const float* d_in, size_t in_stride_samples, size_t n, void* d_out, int out_format,
                            size_t out_stride_bytes, float u8_scale, uint32_t flags, void* stream) {
    if (!b) { dabgpu_set_error("iqbal_bank_apply: null bank"); return DABGPU_ERR_INVALID_ARG; }
    const int st = dabgpu_host_iqbal_check_apply("iqbal_bank_apply", b->n, b->geom, d_in, in_stride_samples, n, d_out, out_format, &out_stride_bytes,
                                                 u8_scale, flags);
    if (st) return st;
    DABGPU_BIND(b->ctx);
    return iqb_launch(b, d_in, in_stride_samples, n, d_out, out_format, out_stride_bytes, u8_scale, flags, (hipStream_t)stream);
}

int dabgpu_iqbal_bank_apply_host_sync(dabgpu_iqbal_bank* b, const float* h_in, size_t in_stride_samples, size_t n, void* h_out, int out_format,
                                      size_t out_stride_bytes, float u8_scale, uint32_t flags) {
    if (!b) { dabgpu_set_error("iqbal_bank_apply_host_sync: null bank"); return DABGPU_ERR_INVALID_ARG; }
    int st = dabgpu_host_iqbal_check_apply("iqbal_bank_apply_host_sync", b->n, b->geom, h_in, in_stride_samples, n, h_out, out_format, &out_stride_bytes,
                                           u8_scale, flags, false);
    if (st) return st;
    dabgpu_ctx* c = b->ctx;
    DABGPU_BIND(c);
    DABGPU_HOST_LOCK(c);
    const bool measure = (flags & DABGPU_IQBAL_MEASURE) != 0;
    uint32_t refused[2] = {0, 0};                                            // calls_refused of record 0 before and after
    auto read_refused = [&](uint32_t* dst) {
        return dabgpu_check_hip(hipMemcpyAsync(dst, &b->d_rec[0].calls_refused, 4, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync(iqbal refusals)");
    };
    if (measure) {
        if ((st = read_refused(&refused[0]))) return st;
        DABGPU_CK(hipStreamSynchronize(c->stream));
    }
    if (flags & DABGPU_IQBAL_APPLY) {
        st = sb_host_round_trip(b, b->n, b->n, false, h_in, in_stride_samples, n, n, h_out, out_format, out_stride_bytes,
                                [&](const float* d_in, size_t d_in_stride, void* d_out, size_t d_out_stride, hipStream_t s) {
                                    const int st2 = iqb_launch(b, d_in, d_in_stride, n, d_out, out_format, d_out_stride, u8_scale, flags, s);
                                    return (st2 || !measure) ? st2 : read_refused(&refused[1]);
                                });
        if (st) return st;
    } else {                                                                 // MEASURE alone: the rows in, the launch, no rows back
        const size_t d_in_stride = in_stride_samples ? (n + 1) & ~(size_t)1 : 0, n_rows = in_stride_samples ? b->n : 1;
        const size_t need = n_rows * (d_in_stride ? d_in_stride : n) * 8;
        if (b->buf[0].needs(need)) {
            if (b->buf[0]) DABGPU_CK(hipDeviceSynchronize());
            if ((st = b->buf[0].regrow(need, "hipMalloc(iqbal input)"))) return st;
        }
        void* d_in = b->buf[0].get();
        DABGPU_CK(hipMemcpy2DAsync(d_in, (d_in_stride ? d_in_stride : n) * 8, h_in, (in_stride_samples ? in_stride_samples : n) * 8, n * 8, n_rows,
                                   hipMemcpyHostToDevice, c->stream));
        if ((st = iqb_launch(b, static_cast<const float*>(d_in), d_in_stride, n, nullptr, DABGPU_IQ_RAW_F32L, 0, 1.0f, flags, c->stream))) return st;
        if ((st = read_refused(&refused[1]))) return st;
        DABGPU_CK(hipStreamSynchronize(c->stream));
    }
    if (measure && refused[1] != refused[0]) {
        dabgpu_set_error("iqbal_bank_apply_host_sync: MEASURE needs the position to be a multiple of 1024 (the call did nothing)");
        return DABGPU_ERR_INVALID_ARG;
    }
    return DABGPU_OK;
}

int dabgpu_iqbal_bank_read_state_host_sync(dabgpu_iqbal_bank* b, dabgpu_iqbal_record* h_records) {
    if (!b || !h_records) { dabgpu_set_error("iqbal_bank_read_state_host_sync: null bank / result"); return DABGPU_ERR_INVALID_ARG; }
    int st;
    dabgpu_ctx* c = b->ctx;
    DABGPU_BIND(c);
    DABGPU_HOST_LOCK(c);
    DABGPU_CK(hipMemcpyAsync(h_records, b->d_rec, b->n * sizeof(dabgpu_iqbal_record), hipMemcpyDeviceToHost, c->stream));
    DABGPU_CK(hipStreamSynchronize(c->stream));
    return DABGPU_OK;
}

int dabgpu_iqbal_bank_read_moments_host_sync(dabgpu_iqbal_bank* b, size_t n_tiles, float* h_moments) {
    if (!b || !h_moments) { dabgpu_set_error("iqbal_bank_read_moments_host_sync: null bank / result"); return DABGPU_ERR_INVALID_ARG; }
    if (n_tiles == 0 || n_tiles > b->geom.tiles_per_call) {
        dabgpu_set_error("iqbal_bank_read_moments_host_sync: %zu tiles (1..%u, the bank's tiles per call)", n_tiles, b->geom.tiles_per_call);
        return DABGPU_ERR_INVALID_ARG;
    }
    int st;
    dabgpu_ctx* c = b->ctx;
    DABGPU_BIND(c);
    DABGPU_HOST_LOCK(c);
    std::vector<float> tmp(n_tiles * b->n * IQB_TILE_FLOATS);                // the scratch is [tile][stream]
    DABGPU_CK(hipMemcpyAsync(tmp.data(), b->d_scratch, tmp.size() * 4, hipMemcpyDeviceToHost, c->stream));
    DABGPU_CK(hipStreamSynchronize(c->stream));
    for (size_t j = 0; j < n_tiles; j++)
        for (size_t s = 0; s < b->n; s++)
            for (int k = 0; k < IQB_TILE_FLOATS; k++) h_moments[(s * n_tiles + j) * IQB_TILE_FLOATS + k] = tmp[(j * b->n + s) * IQB_TILE_FLOATS + k];
    return DABGPU_OK;
}

}  // extern "C"
