// channel.hip -- the channel model on the device (include/dabgpu.h, "Channel model"): multipath, carrier offset, timing offset and white
// Gaussian noise for a bank of independent streams.  Every arithmetic step is channel_core.h's; this file is where the samples come from
// and go to.
//
// One 256-thread workgroup per (stream, tile of DABGPU_CHANNEL_BLOCK = 1024 output samples).  Tiles are aligned to ABSOLUTE sample
// numbers (the first starts at position & ~3), so that the two samples of a Philox call and the 16 / 8 bytes of a store belong to one
// thread wherever the stream position stands; a call that starts at an odd position stores sample by sample.
// STAGE: the tile's input window -- 1024 samples plus the stream's largest delay -- goes to LDS once, two samples per 16-byte load, wrap
// and zero-fill resolved there; the taps then read LDS.  !STAGE (every stream of the bank one tap of delay 0): the two samples come
// straight from memory.  Complex float: two samples per thread and pass, one non-temporal 16-byte store; u8: four samples, one 8-byte
// store.  The stream's parameters are read through a pointer that is the same for the whole workgroup (scalar loads).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <new>
#include <vector>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "channel_core.h"
#include "channel_device.h"
#include "signal_bank.h"

namespace dabgpu {

template <int OUT, bool STAGE>
__global__ __launch_bounds__(256)
void channel_kernel(const dabgpu_channel_stream* __restrict__ params, const uint64_t* __restrict__ d_pos, const chf2* __restrict__ in,
                    size_t in_stride, int64_t n_in, int wrap, uint32_t n_out, int tiles, uint8_t* __restrict__ out, size_t out_stride_bytes,
                    float scale)
{
    extern __shared__ __attribute__((aligned(16))) ch_f4 ch_lds4[];
    constexpr int SPT = (OUT == DABGPU_IQ_RAW_F32L) ? 2 : 4;            // samples per thread and pass
    const int t = threadIdx.x;
    const uint32_t s = blockIdx.x / (uint32_t)tiles, tile = blockIdx.x % (uint32_t)tiles;
    const dabgpu_channel_stream& P = params[s];
    const uint64_t pos = *d_pos;
    const uint64_t T0 = (pos & ~(uint64_t)3) + (uint64_t)tile * CH_BLK;       // absolute number of the tile's first sample
    const uint64_t rel0 = T0 - pos;                                          // -3 .. 0 (as unsigned) for tile 0
    // samples of this tile inside the call: tile-local [lo, hi)
    const int lo = (tile == 0) ? (int)(pos & 3) : 0;
    const int64_t left = (int64_t)n_out - (int64_t)rel0;                      // samples from T0 to the call's end
    if (left <= lo) return;
    const int hi = left < CH_BLK ? (int)left : CH_BLK;
    const chf2* x = in + (size_t)s * in_stride;
    uint8_t* orow = out + (size_t)s * out_stride_bytes;
    const bool aligned = (pos & (uint64_t)(SPT - 1)) == 0;

    const chf2* lds = reinterpret_cast<const chf2*>(ch_lds4);
    int lds_shift = 0;                                                       // LDS sample i = x[T0 - start - halo - lds_shift + i]
    const int halo = STAGE ? ch_stream_halo(P) : 0;
    ChWindow W;
    if constexpr (STAGE) {
        const uint64_t base = T0 - (uint64_t)P.start - (uint64_t)halo;
        lds_shift = (int)(base & 1);
        const int count = (hi + halo + lds_shift + 1) & ~1;                  // <= CH_BLK + halo + 2
        W = ch_window(x, n_in, wrap != 0, base - (uint64_t)lds_shift, count);
        for (int i = t; i < count / 2; i += 256) {
            chf2 a, b;
            ch_load2(W, 2 * i, a, b);
            ch_lds4[i] = ch_f4{a.re, a.im, b.re, b.im};
        }
        __syncthreads();
    } else {
        W = ch_window(x, n_in, wrap != 0, T0 - (uint64_t)P.start, CH_BLK);
    }

    const bool noisy = P.noise_sigma != 0.0f;
    for (int q = t; q < CH_BLK / SPT; q += 256) {
        const int n0 = SPT * q;                                              // tile-local number of the thread's first sample
        if (n0 + SPT <= lo || n0 >= hi) continue;
        chf2 y[SPT];
#pragma unroll
        for (int h = 0; h < SPT; h += 2) {
            const uint64_t m = T0 + (uint64_t)(n0 + h);                      // even
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            if (noisy) ch_noise_words(P.seed, s, m >> 1, w);
            chf2 z0, z1;
            if constexpr (STAGE) {
                const int li = n0 + h + halo + lds_shift;
                z0 = ch_paths(P, [&](int k) { return lds[li - P.tap_delay[k]]; });
                z1 = ch_paths(P, [&](int k) { return lds[li + 1 - P.tap_delay[k]]; });
            } else {
                chf2 a, b;
                ch_load2(W, n0 + h, a, b);
                z0 = ch_tap_first(P.tap_re[0], P.tap_im[0], a);
                z1 = ch_tap_first(P.tap_re[0], P.tap_im[0], b);
            }
            y[h] = ch_finish(P, m, z0, w);
            y[h + 1] = ch_finish(P, m + 1, z1, w);
        }
        const bool whole = aligned && n0 >= lo && n0 + SPT <= hi;
        const size_t o = (size_t)(rel0 + (uint64_t)n0);                      // output sample of n0 (meaningful where n0 >= lo)
        if constexpr (OUT == DABGPU_IQ_RAW_F32L) {
            if (whole) {
                __builtin_nontemporal_store(ch_f4{y[0].re, y[0].im, y[1].re, y[1].im}, reinterpret_cast<ch_f4*>(orow + 8 * o));
            } else {
#pragma unroll
                for (int h = 0; h < SPT; h++)
                    if (n0 + h >= lo && n0 + h < hi) *reinterpret_cast<ch_f2v*>(orow + 8 * (o + h)) = ch_f2v{y[h].re, y[h].im};
            }
        } else {
            uint32_t b[SPT];
#pragma unroll
            for (int h = 0; h < SPT; h++) b[h] = ch_u8(y[h].re, scale) | (ch_u8(y[h].im, scale) << 8);
            if (whole) {
                *reinterpret_cast<uint2*>(orow + 2 * o) = make_uint2(b[0] | (b[1] << 16), b[2] | (b[3] << 16));
            } else {
#pragma unroll
                for (int h = 0; h < SPT; h++)
                    if (n0 + h >= lo && n0 + h < hi) *reinterpret_cast<uint16_t*>(orow + 2 * (o + h)) = (uint16_t)b[h];
            }
        }
    }
}

// channel_fading.hip
void ch_launch_fading(const dabgpu_channel_stream* d_params, const dabgpu_channel_fading_stream* d_tables, const uint64_t* d_pos,
                      const dabgpu_channel_geometry& geom, int tiles, unsigned grid, const float* d_in, size_t in_stride, size_t n_in, int wrap, size_t n_out,
                      void* d_out, int out_format, size_t out_stride_bytes, float u8_scale, hipStream_t s);

}  // namespace dabgpu

using namespace dabgpu;

struct dabgpu_channel_bank : SignalBank {         // d_mem: position (16 bytes) | parameters
    size_t n = 0;
    dabgpu_channel_geometry geom = {};
    dabgpu_channel_stream* d_params = nullptr;
    DeviceBuffer<dabgpu_channel_fading_stream> d_fading;   // a fading bank's tables (its own allocation); empty: a plain bank
    std::vector<dabgpu_channel_stream> h_params;        // a fading bank keeps its parameters and tables on the host: _set_fading and
    std::vector<dabgpu_channel_fading_stream> h_tables; // _set_params check the one against the other (n_taps may grow past checked kinds)
};

static int ch_launch(dabgpu_channel_bank* b, const float* d_in, size_t in_stride, size_t n_in, int wrap, size_t n_out, void* d_out, int out_format,
                     size_t out_stride_bytes, float u8_scale, hipStream_t s) {
    const int tiles = (int)((n_out + 3 + CH_BLK - 1) / CH_BLK);
    const unsigned grid = (unsigned)((size_t)tiles * b->n);
    const bool stage = b->geom.staged != 0;
    const size_t lds = stage ? (size_t)(CH_BLK + b->geom.halo + 2) * 8 : 0;
    const chf2* in = reinterpret_cast<const chf2*>(d_in);
#define CH_GO(OUT, STAGE)                                                                                                                     \
    hipLaunchKernelGGL((channel_kernel<OUT, STAGE>), dim3(grid), dim3(256), lds, s, b->d_params, b->d_pos, in, in_stride, (int64_t)n_in, wrap, \
                       (uint32_t)n_out, tiles, static_cast<uint8_t*>(d_out), out_stride_bytes, u8_scale)
    if (b->d_fading)
        ch_launch_fading(b->d_params, b->d_fading.get(), b->d_pos, b->geom, tiles, grid, d_in, in_stride, n_in, wrap, n_out, d_out, out_format, out_stride_bytes, u8_scale, s);
    else if (out_format == DABGPU_IQ_RAW_F32L) { if (stage) CH_GO(DABGPU_IQ_RAW_F32L, true); else CH_GO(DABGPU_IQ_RAW_F32L, false); }
    else { if (stage) CH_GO(DABGPU_IQ_RAW_U8, true); else CH_GO(DABGPU_IQ_RAW_U8, false); }
#undef CH_GO
    sb_enqueue_advance(b->d_pos, n_out, s);
    return dabgpu_check_hip(hipGetLastError(), b->d_fading ? "channel_fading_kernel launch" : "channel_kernel launch");
}

static int ch_create(const char* who, dabgpu_ctx* c, size_t n_streams, const dabgpu_channel_stream* h_params, const dabgpu_channel_fading_stream* h_tables,
                     bool fading, dabgpu_channel_bank** out) {
    if (!c || !out) { dabgpu_set_error("%s: null context / result", who); return DABGPU_ERR_INVALID_ARG; }
    *out = nullptr;
    dabgpu_channel_geometry g;
    int st = dabgpu_host_channel_plan(h_params, n_streams, &g);
    if (st) return st;
    if (fading && (st = dabgpu_host_channel_fading_check(who, h_params, h_tables, n_streams))) return st;
    dabgpu_channel_bank* b = new (std::nothrow) dabgpu_channel_bank;
    if (!b) return DABGPU_ERR_HIP;
    b->ctx = c; b->n = n_streams; b->geom = fading ? dabgpu_host_channel_fading_geometry(g) : g;
    auto fail = [&](int status) { dabgpu_channel_bank_destroy(b); return status; };
    if ((st = dabgpu_bind_device(c))) return fail(st);
    if (fading) {
        b->h_params.assign(h_params, h_params + n_streams);
        b->h_tables.assign(h_tables, h_tables + n_streams);
        const size_t table_bytes = n_streams * sizeof(dabgpu_channel_fading_stream);
        if ((st = b->d_fading.alloc(n_streams, "hipMalloc(channel fading tables)"))) return fail(st);
        if ((st = dabgpu_stage_h2d(c, b->d_fading.get(), h_tables, table_bytes, c->stream))) return fail(st);
    }
    uint8_t* payload;
    if ((st = sb_alloc(b, n_streams * sizeof(dabgpu_channel_stream), "channel", &payload))) return fail(st);
    b->d_params = reinterpret_cast<dabgpu_channel_stream*>(payload);
    if ((st = dabgpu_stage_h2d(c, b->d_params, h_params, n_streams * sizeof(dabgpu_channel_stream), c->stream))) return fail(st);
    if ((st = dabgpu_check_hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize(channel_bank_create)"))) return fail(st);
    *out = b;
    return DABGPU_OK;
}

extern "C" {

int dabgpu_channel_bank_create(dabgpu_ctx* c, size_t n_streams, const dabgpu_channel_stream* h_params, dabgpu_channel_bank** out) {
    return ch_create("channel_bank_create", c, n_streams, h_params, nullptr, false, out);
}

int dabgpu_channel_bank_create_fading(dabgpu_ctx* c, size_t n_streams, const dabgpu_channel_stream* h_params, const dabgpu_channel_fading_stream* h_tables,
                                      dabgpu_channel_bank** out) {
    return ch_create("channel_bank_create_fading", c, n_streams, h_params, h_tables, true, out);
}

int dabgpu_channel_bank_set_fading(dabgpu_channel_bank* b, const dabgpu_channel_fading_stream* h_tables, void* stream) {
    if (!b) { dabgpu_set_error("channel_bank_set_fading: null bank"); return DABGPU_ERR_INVALID_ARG; }
    if (!b->d_fading) { dabgpu_set_error("channel_bank_set_fading: the bank was not created with dabgpu_channel_bank_create_fading"); return DABGPU_ERR_INVALID_ARG; }
    const int st = dabgpu_host_channel_fading_check("channel_bank_set_fading", b->h_params.data(), h_tables, b->n);
    if (st) return st;
    b->h_tables.assign(h_tables, h_tables + b->n);
    DABGPU_BIND(b->ctx);
    return dabgpu_stage_h2d(b->ctx, b->d_fading.get(), h_tables, b->n * sizeof(dabgpu_channel_fading_stream), (hipStream_t)stream);
}

void dabgpu_channel_bank_destroy(dabgpu_channel_bank* b) {
    if (!dabgpu_destroy_begin(b, b ? b->ctx : nullptr)) return;
    delete b;
}

int dabgpu_channel_bank_set_params(dabgpu_channel_bank* b, const dabgpu_channel_stream* h_params, void* stream) {
    if (!b) { dabgpu_set_error("channel_bank_set_params: null bank"); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_channel_geometry g;
    int st = dabgpu_host_channel_plan(h_params, b->n, &g);
    if (st || (st = dabgpu_host_channel_fits(b->geom, g))) return st;       // (b->geom stays: captured calls launch with it)
    if (b->d_fading) {
        if ((st = dabgpu_host_channel_fading_check("channel_bank_set_params", h_params, b->h_tables.data(), b->n))) return st;
        b->h_params.assign(h_params, h_params + b->n);
    }
    DABGPU_BIND(b->ctx);
    return dabgpu_stage_h2d(b->ctx, b->d_params, h_params, b->n * sizeof(dabgpu_channel_stream), (hipStream_t)stream);
}

int dabgpu_channel_bank_seek(dabgpu_channel_bank* b, uint64_t position, void* stream) {
    return sb_seek(b, "channel_bank_seek", position, (uint64_t)DABGPU_CHANNEL_MAX_POSITION, "2^62", stream);
}

int dabgpu_channel_bank_apply(dabgpu_channel_bank* b, const float* d_in, size_t in_stride_samples, size_t n_in, int wrap, size_t n_out, void* d_out,
                              int out_format, size_t out_stride_bytes, float u8_scale, void* stream) {
    if (!b) { dabgpu_set_error("channel_bank_apply: null bank"); return DABGPU_ERR_INVALID_ARG; }
    const int st = dabgpu_host_channel_check_apply("channel_bank_apply", b->n, d_in, in_stride_samples, n_in, n_out, d_out, out_format, &out_stride_bytes,
                                                   u8_scale);
    if (st || n_out == 0) return st;
    DABGPU_BIND(b->ctx);
    return ch_launch(b, d_in, in_stride_samples, n_in, wrap, n_out, d_out, out_format, out_stride_bytes, u8_scale, (hipStream_t)stream);
}

int dabgpu_channel_bank_apply_host_sync(dabgpu_channel_bank* b, const float* h_in, size_t in_stride_samples, size_t n_in, int wrap, size_t n_out,
                                        void* h_out, int out_format, size_t out_stride_bytes, float u8_scale) {
    if (!b) { dabgpu_set_error("channel_bank_apply_host_sync: null bank"); return DABGPU_ERR_INVALID_ARG; }
    const int st = dabgpu_host_channel_check_apply("channel_bank_apply_host_sync", b->n, h_in, in_stride_samples, n_in, n_out, h_out, out_format,
                                                   &out_stride_bytes, u8_scale, false);
    if (st || n_out == 0) return st;
    return sb_host_round_trip(b, b->n, b->n, false, h_in, in_stride_samples, n_in, n_out, h_out, out_format, out_stride_bytes,
                              [&](const float* d_in, size_t d_in_stride, void* d_out, size_t d_out_stride, hipStream_t s) {
                                  return ch_launch(b, d_in, d_in_stride, n_in, wrap, n_out, d_out, out_format, d_out_stride, u8_scale, s);
                              });
}

}  // extern "C"
