// interferer.hip -- the interferer on the device (include/dabgpu.h, "Interferer"): tones, band-limited noise and gated bursts added to a
// bank of independent streams.  Every arithmetic step is interferer_core.h's; this file is where the samples come from and go to.
//
// One 256-thread workgroup per (stream, tile of DABGPU_INTERFERER_BLOCK = 1024 output samples), tiles aligned to ABSOLUTE sample numbers
// as in channel.hip: a thread owns the two samples of a Philox call and of a 16-byte load and store (u8: four samples, one 8-byte store)
// wherever the stream position stands; a call that starts at an odd position stores sample by sample.
// BAND: every shaped BAND source that is on somewhere in the tile gets a slot of LDS: the 16 L floats of its shape and the tile's
// 1024 / L + 17 values of g, generated cooperatively (one Philox call, two values).  The per-sample sum then reads taps[r + L t]
// (consecutive addresses across lanes, period L) and g[q - t] (a broadcast within L consecutive lanes); for L >= 2 a thread's two samples
// share q and their taps are neighbours, so one 8-byte read of either serves both.  !BAND (a bank of tones and white
// sources) allocates no LDS.  Kind and gate are decided per source and tile: a source that is off over the whole tile is skipped, one
// that is on over the whole tile runs ungated, and only a tile with a gate edge selects per lane, stepping the remainder the tile's first
// sample has.  The stream's parameters are read through a pointer that is the same for the whole workgroup (scalar loads).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <new>
#include <vector>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "interferer_core.h"
#include "channel_device.h"
#include "signal_bank.h"

namespace dabgpu {

constexpr int ITF_BLK = DABGPU_INTERFERER_BLOCK;
static_assert(ITF_BLK == CH_BLK, "the tile arithmetic is the channel kernel's");

template <int OUT, bool BAND>
__global__ __launch_bounds__(256)
void interferer_kernel(const dabgpu_interferer_stream* __restrict__ params, const dabgpu_interferer_shape* __restrict__ shapes,
                       const uint64_t* __restrict__ d_pos, const chf2* in, size_t in_stride, uint32_t n_out, int tiles, uint8_t* out,
                       size_t out_stride_bytes, float scale, uint32_t slot_bytes)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t itf_lds[];
    constexpr int SPT = (OUT == DABGPU_IQ_RAW_F32L) ? 2 : 4;            // samples per thread and pass
    constexpr int NS = DABGPU_INTERFERER_MAX;
    const int t = threadIdx.x;
    const uint32_t s = blockIdx.x / (uint32_t)tiles, tile = blockIdx.x % (uint32_t)tiles;
    const dabgpu_interferer_stream& P = params[s];
    const uint64_t pos = *d_pos;
    const uint64_t T0 = (pos & ~(uint64_t)3) + (uint64_t)tile * ITF_BLK;      // absolute number of the tile's first sample
    const uint64_t rel0 = T0 - pos;                                          // -3 .. 0 (as unsigned) for tile 0
    const int lo = (tile == 0) ? (int)(pos & 3) : 0;                         // samples of this tile inside the call: tile-local [lo, hi)
    const int64_t left = (int64_t)n_out - (int64_t)rel0;
    if (left <= lo) return;
    const int hi = left < ITF_BLK ? (int)left : ITF_BLK;
    const chf2* x = in ? in + (size_t)s * in_stride : nullptr;
    uint8_t* orow = out + (size_t)s * out_stride_bytes;
    const bool aligned = (pos & (uint64_t)(SPT - 1)) == 0, even = (pos & 1) == 0;

    // per source, the same for the whole workgroup: does it run in this tile, does the tile hold a gate edge, where is its LDS
    uint32_t active = 0, mixed = 0;
    uint64_t rem0[NS], g_first[NS];
    uint32_t slot_at[NS];
    int shift[NS];
    uint32_t slots = 0;
#pragma unroll
    for (int k = 0; k < NS; k++) {
        rem0[k] = 0; g_first[k] = 0; slot_at[k] = 0; shift[k] = 0;
        if (k >= P.n_sources) continue;
        const dabgpu_interferer_source& S = P.source[k];
        if (!itf_live(S)) continue;
        if (S.gate_period != 0) {
            const uint64_t r = itf_gate_rem(T0, S.gate_offset, S.gate_period);
            rem0[k] = r;
            const bool all_on = r < S.gate_on && S.gate_on - r >= (uint64_t)ITF_BLK;
            const bool all_off = r >= S.gate_on && S.gate_period - r >= (uint64_t)ITF_BLK;
            if (all_off) continue;
            if (!all_on) mixed |= 1u << k;
        }
        if (itf_shaped(S)) {
            if constexpr (!BAND) continue;                                   // (the planner admits none to such a bank)
            const dabgpu_interferer_shape& H = shapes[S.shape];
            const int l = itf_log2(H.interp), L = H.interp;
            shift[k] = l;
            g_first[k] = ((T0 >> l) - (uint64_t)(ITF_TAPS - 1)) & ~(uint64_t)1;  // even: LDS value i is g[g_first + i] (wrapping below 0)
            slot_at[k] = slots * slot_bytes;
            slots++;
            float* taps = reinterpret_cast<float*>(itf_lds + slot_at[k]);
            chf2* g = reinterpret_cast<chf2*>(itf_lds + slot_at[k] + (uint32_t)(ITF_TAPS * L) * 4u);
            for (int i = t; i < ITF_TAPS * L; i += 256) taps[i] = H.taps[i];
            const uint64_t q_last = (T0 + (uint64_t)(hi - 1)) >> l;
            const int pairs = (int)((q_last - g_first[k]) >> 1) + 1;         // <= (1024 / L + 18) / 2
            for (int p = t; p < pairs; p += 256) {
                const uint64_t n = g_first[k] + 2u * (uint64_t)p;
                uint32_t w[4];
                itf_noise_words(P.seed, s, (uint32_t)k, n >> 1, w);
                g[2 * p] = ch_gauss_pair(w[0], w[1]);
                g[2 * p + 1] = ch_gauss_pair(w[2], w[3]);
            }
        }
        active |= 1u << k;
    }
    if constexpr (BAND) __syncthreads();

    for (int q = t; q < ITF_BLK / SPT; q += 256) {
        const int n0 = SPT * q;                                              // tile-local number of the thread's first sample
        if (n0 + SPT <= lo || n0 >= hi) continue;
        const size_t o = (size_t)(rel0 + (uint64_t)n0);                      // sample of n0 in the call (meaningful where n0 >= lo)
        chf2 y[SPT];
#pragma unroll
        for (int h = 0; h < SPT; h += 2) {
            y[h] = y[h + 1] = chf2{0.0f, 0.0f};
            if (x) {
                const bool in0 = n0 + h >= lo && n0 + h < hi, in1 = n0 + h + 1 >= lo && n0 + h + 1 < hi;
                if (in0 && in1 && even) {
                    const ch_f4 v = *reinterpret_cast<const ch_f4*>(x + o + h);
                    y[h] = chf2{v.x, v.y}; y[h + 1] = chf2{v.z, v.w};
                } else {
                    if (in0) y[h] = ch_ld(x + o + h);
                    if (in1) y[h + 1] = ch_ld(x + o + h + 1);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NS; k++) {
            if (!((active >> k) & 1u)) continue;
            const dabgpu_interferer_source& S = P.source[k];
#pragma unroll
            for (int h = 0; h < SPT; h += 2) {
                const uint64_t m = T0 + (uint64_t)(n0 + h);                  // even
                chf2 v0, v1;
                if (S.kind == DABGPU_INTERFERER_TONE) {
                    v0 = itf_tone(S, m);
                    v1 = itf_tone(S, m + 1);
                } else if (S.shape < 0) {
                    uint32_t w[4];
                    itf_noise_words(P.seed, s, (uint32_t)k, m >> 1, w);
                    v0 = itf_band_finish(S, m, itf_white(ch_gauss_pair(w[0], w[1])));
                    v1 = itf_band_finish(S, m + 1, itf_white(ch_gauss_pair(w[2], w[3])));
                } else {
                    v0 = v1 = chf2{0.0f, 0.0f};
                    if constexpr (BAND) {
                        const int l = shift[k], L = 1 << l;
                        const float* taps = reinterpret_cast<const float*>(itf_lds + slot_at[k]);
                        const chf2* g = reinterpret_cast<const chf2*>(itf_lds + slot_at[k] + (uint32_t)(ITF_TAPS * L) * 4u);
                        const int i0 = (int)((m >> l) - g_first[k]), i1 = (int)(((m + 1) >> l) - g_first[k]);      // >= 15
                        const int r = (int)(m & (uint64_t)(L - 1));
                        chf2 b0, b1;
                        if (l > 0) {
                            // m is even: both samples share q and their taps are neighbours, so one 8-byte read serves both of either;
                            // the operations per sample are itf_band_sum's, in its order
                            const ch_f2v h0 = *reinterpret_cast<const ch_f2v*>(taps + r);
                            const chf2 g0 = g[i0];
                            b0 = chf2{h0.x * g0.re, h0.x * g0.im};
                            b1 = chf2{h0.y * g0.re, h0.y * g0.im};
#pragma unroll
                            for (int tt = 1; tt < ITF_TAPS; tt++) {
                                const ch_f2v h = *reinterpret_cast<const ch_f2v*>(taps + r + L * tt);
                                const chf2 gt = g[i0 - tt];
                                b0 = chf2{__builtin_fmaf(h.x, gt.re, b0.re), __builtin_fmaf(h.x, gt.im, b0.im)};
                                b1 = chf2{__builtin_fmaf(h.y, gt.re, b1.re), __builtin_fmaf(h.y, gt.im, b1.im)};
                            }
                        } else {
                            b0 = itf_band_sum(taps, L, 0, [&](int tt) { return g[i0 - tt]; });
                            b1 = itf_band_sum(taps, L, 0, [&](int tt) { return g[i1 - tt]; });
                        }
                        v0 = itf_band_finish(S, m, b0);
                        v1 = itf_band_finish(S, m + 1, b1);
                    }
                }
                bool on0 = true, on1 = true;
                if ((mixed >> k) & 1u) {
                    on0 = itf_gate_step(rem0[k], (uint32_t)(n0 + h), S.gate_period) < S.gate_on;
                    on1 = itf_gate_step(rem0[k], (uint32_t)(n0 + h + 1), S.gate_period) < S.gate_on;
                }
                if (on0) y[h] = itf_add(y[h], v0);
                if (on1) y[h + 1] = itf_add(y[h + 1], v1);
            }
        }
        const bool whole = aligned && n0 >= lo && n0 + SPT <= hi;
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

}  // namespace dabgpu

using namespace dabgpu;

struct dabgpu_interferer_bank : SignalBank {      // d_mem: position (16 bytes) | parameters | shapes
    size_t n = 0;
    int n_shapes = 0;
    dabgpu_interferer_geometry geom = {};
    dabgpu_interferer_stream* d_params = nullptr;
    dabgpu_interferer_shape* d_shapes = nullptr;
    std::vector<dabgpu_interferer_shape> h_shapes;  // _set_params checks new parameters against the shapes of the creation
};

static int itf_launch(dabgpu_interferer_bank* b, const float* d_in, size_t in_stride, size_t n_out, void* d_out, int out_format, size_t out_stride_bytes,
                      float u8_scale, hipStream_t s) {
    const int tiles = (int)((n_out + 3 + ITF_BLK - 1) / ITF_BLK);
    const unsigned grid = (unsigned)((size_t)tiles * b->n);
    const bool band = b->geom.band_slots != 0;
    const chf2* in = reinterpret_cast<const chf2*>(d_in);
#define ITF_GO(OUT, BAND)                                                                                                                       \
    hipLaunchKernelGGL((interferer_kernel<OUT, BAND>), dim3(grid), dim3(256), (BAND) ? b->geom.lds_bytes : 0, s, b->d_params, b->d_shapes, b->d_pos, in, \
                       in_stride, (uint32_t)n_out, tiles, static_cast<uint8_t*>(d_out), out_stride_bytes, u8_scale, b->geom.slot_bytes)
    if (out_format == DABGPU_IQ_RAW_F32L) { if (band) ITF_GO(DABGPU_IQ_RAW_F32L, true); else ITF_GO(DABGPU_IQ_RAW_F32L, false); }
    else { if (band) ITF_GO(DABGPU_IQ_RAW_U8, true); else ITF_GO(DABGPU_IQ_RAW_U8, false); }
#undef ITF_GO
    sb_enqueue_advance(b->d_pos, n_out, s);
    return dabgpu_check_hip(hipGetLastError(), "interferer_kernel launch");
}

extern "C" {

int dabgpu_interferer_bank_create(dabgpu_ctx* c, size_t n_streams, const dabgpu_interferer_stream* h_params, const dabgpu_interferer_shape* h_shapes,
                                  int n_shapes, dabgpu_interferer_bank** out) {
    if (!c || !out) { dabgpu_set_error("interferer_bank_create: null context / result"); return DABGPU_ERR_INVALID_ARG; }
    *out = nullptr;
    dabgpu_interferer_geometry g;
    int st = dabgpu_host_interferer_plan("interferer_bank_create", h_params, n_streams, h_shapes, n_shapes, &g);
    if (st) return st;
    dabgpu_interferer_bank* b = new (std::nothrow) dabgpu_interferer_bank;
    if (!b) return DABGPU_ERR_HIP;
    b->ctx = c; b->n = n_streams; b->n_shapes = n_shapes; b->geom = g;
    if (n_shapes > 0) b->h_shapes.assign(h_shapes, h_shapes + n_shapes);
    auto fail = [&](int status) { dabgpu_interferer_bank_destroy(b); return status; };
    if ((st = dabgpu_bind_device(c))) return fail(st);
    const size_t param_bytes = n_streams * sizeof(dabgpu_interferer_stream), shape_bytes = (size_t)n_shapes * sizeof(dabgpu_interferer_shape);
    uint8_t* payload;
    if ((st = sb_alloc(b, param_bytes + shape_bytes, "interferer", &payload))) return fail(st);
    b->d_params = reinterpret_cast<dabgpu_interferer_stream*>(payload);
    b->d_shapes = reinterpret_cast<dabgpu_interferer_shape*>(payload + param_bytes);
    if ((st = dabgpu_stage_h2d(c, b->d_params, h_params, param_bytes, c->stream))) return fail(st);
    if (n_shapes > 0 && (st = dabgpu_stage_h2d(c, b->d_shapes, h_shapes, shape_bytes, c->stream))) return fail(st);
    if ((st = dabgpu_check_hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize(interferer_bank_create)"))) return fail(st);
    *out = b;
    return DABGPU_OK;
}

void dabgpu_interferer_bank_destroy(dabgpu_interferer_bank* b) {
    if (!dabgpu_destroy_begin(b, b ? b->ctx : nullptr)) return;
    delete b;
}

int dabgpu_interferer_bank_set_params(dabgpu_interferer_bank* b, const dabgpu_interferer_stream* h_params, void* stream) {
    if (!b) { dabgpu_set_error("interferer_bank_set_params: null bank"); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_interferer_geometry g;
    int st = dabgpu_host_interferer_plan("interferer_bank_set_params", h_params, b->n, b->h_shapes.data(), b->n_shapes, &g);
    if (st || (st = dabgpu_host_interferer_fits(b->geom, g))) return st;     // (b->geom stays: captured calls launch with it)
    DABGPU_BIND(b->ctx);
    return dabgpu_stage_h2d(b->ctx, b->d_params, h_params, b->n * sizeof(dabgpu_interferer_stream), (hipStream_t)stream);
}

int dabgpu_interferer_bank_seek(dabgpu_interferer_bank* b, uint64_t position, void* stream) {
    return sb_seek(b, "interferer_bank_seek", position, (uint64_t)DABGPU_INTERFERER_MAX_POSITION - 1u, "2^62 - 1", stream);
}

int dabgpu_interferer_bank_apply(dabgpu_interferer_bank* b, const float* d_in, size_t in_stride_samples, size_t n_out, void* d_out, int out_format,
                                 size_t out_stride_bytes, float u8_scale, void* stream) {
    if (!b) { dabgpu_set_error("interferer_bank_apply: null bank"); return DABGPU_ERR_INVALID_ARG; }
    const int st = dabgpu_host_interferer_check_apply("interferer_bank_apply", b->n, d_in, in_stride_samples, n_out, d_out, out_format, &out_stride_bytes,
                                                      u8_scale);
    if (st || n_out == 0) return st;
    DABGPU_BIND(b->ctx);
    return itf_launch(b, d_in, in_stride_samples, n_out, d_out, out_format, out_stride_bytes, u8_scale, (hipStream_t)stream);
}

int dabgpu_interferer_bank_apply_host_sync(dabgpu_interferer_bank* b, const float* h_in, size_t in_stride_samples, size_t n_out, void* h_out,
                                           int out_format, size_t out_stride_bytes, float u8_scale) {
    if (!b) { dabgpu_set_error("interferer_bank_apply_host_sync: null bank"); return DABGPU_ERR_INVALID_ARG; }
    const int st = dabgpu_host_interferer_check_apply("interferer_bank_apply_host_sync", b->n, h_in, in_stride_samples, n_out, h_out, out_format,
                                                      &out_stride_bytes, u8_scale, false);
    if (st || n_out == 0) return st;
    std::vector<float> zeros;                                                // no input: one shared row of zeros, which is what NULL means
    if (!h_in) { zeros.assign(2 * n_out, 0.0f); h_in = zeros.data(); in_stride_samples = 0; }
    return sb_host_round_trip(b, b->n, b->n, false, h_in, in_stride_samples, n_out, n_out, h_out, out_format, out_stride_bytes,
                              [&](const float* d_in, size_t d_in_stride, void* d_out, size_t d_out_stride, hipStream_t s) {
                                  return itf_launch(b, d_in, d_in_stride, n_out, d_out, out_format, d_out_stride, u8_scale, s);
                              });
}

}  // extern "C"
