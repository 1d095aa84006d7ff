// resample.hip -- the resampler on the device (include/dabgpu.h, "Resampler"): arbitrary-ratio, fractional-delay resampling for a bank of
// independent streams.  Every arithmetic step is resample_core.h's; this file is where the samples and the table rows come from and go to.
//
// One 256-thread workgroup per (stream, block of DABGPU_RESAMPLE_BLOCK = 1024 outputs of the call).  The block's input window -- the
// samples between the first output's first tap and the last output's last tap, at most ceil(1024 step) + taps + 2 -- goes to LDS once, two
// samples per 16-byte load, wrap and zero-fill resolved there (the loads of the channel kernels, channel_device.h).  The coefficient rows
// go to LDS as well, in rows of taps + 1 floats (an odd stride: lanes on different rows fall on different banks), but only the rows the
// block can touch: the phase moves by frac(step) per output, so at a step within a few hundred ppm of 1 the 1024 outputs of a block sit
// on a handful of adjacent rows (every lane of a wavefront reads the same row: an LDS broadcast), while at 2.4 -> 2.048 MS/s they sit on all
// of them and the whole table is staged.  Lane t produces the outputs t, t + 256, ... of the block: neighbouring lanes read neighbouring
// input samples (8-byte LDS reads, conflict-free near step 1) and store neighbouring 8-byte (complex float) or 2-byte (u8) results.
// The identity stream stages nothing: it copies, one 8-byte load and one store per sample.  Parameters are read through a pointer that is
// the same for the whole workgroup (scalar loads).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <new>
#include <vector>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "resample_core.h"
#include "channel_device.h"
#include "signal_bank.h"

namespace dabgpu {

constexpr int RS_ROW_STRIDE = RS_TAPS + 1;                                   // floats between staged rows

// the block's input window from index `first` (a word of rs_time) on
__device__ __forceinline__ ChWindow rs_window(const chf2* x, int64_t n_in, bool wrap, RsIndex first, int span) {
    ChWindow W;
    W.x = x; W.n_in = n_in; W.wrap = wrap; W.span = span;
    W.origin = wrap ? rs_mod(first, n_in) : rs_clamped(first);
    return W;
}

// sample `off` of the window alone (the copy path reads every input sample once: 8 bytes per lane)
__device__ __forceinline__ chf2 rs_load1(const ChWindow& W, int off) {
    int64_t j = W.origin + off;
    if (W.wrap) {
        if (j >= W.n_in) j = (W.span <= W.n_in) ? j - W.n_in : j % W.n_in;
        return ch_ld(W.x + j);
    }
    return (j >= 0 && j < W.n_in) ? ch_ld(W.x + j) : chf2{0.0f, 0.0f};
}

template <int OUT>
__global__ __launch_bounds__(256)
void resample_kernel(const dabgpu_resample_stream* __restrict__ params, const float* __restrict__ table, const uint64_t* __restrict__ d_pos,
                     const chf2* __restrict__ in, size_t in_stride, int64_t n_in, int wrap, uint32_t n_out, int tiles, uint8_t* __restrict__ out,
                     size_t out_stride_bytes, float scale, int window_pairs)
{
    extern __shared__ __attribute__((aligned(16))) ch_f4 rs_lds4[];          // [window_pairs] staged input, then the staged rows
    const int t = threadIdx.x;
    const uint32_t s = blockIdx.x / (uint32_t)tiles, tile = blockIdx.x % (uint32_t)tiles;
    const dabgpu_resample_stream& P = params[s];
    const uint32_t o0 = tile * (uint32_t)RS_BLK;                             // the block's first output inside the call
    const int cnt = (n_out - o0 < (uint32_t)RS_BLK) ? (int)(n_out - o0) : RS_BLK;
    const uint64_t m0 = *d_pos + o0;
    const chf2* x = in + (size_t)s * in_stride;
    uint8_t* orow = out + (size_t)s * out_stride_bytes;
    const RsTime ta = rs_time(P, m0), tb = rs_time(P, m0 + (uint64_t)(cnt - 1));

    auto store = [&](int i, chf2 y) {
        const size_t o = (size_t)o0 + (size_t)i;
        if constexpr (OUT == DABGPU_IQ_RAW_F32L) __builtin_nontemporal_store(ch_f2v{y.re, y.im}, reinterpret_cast<ch_f2v*>(orow + 8 * o));
        else *reinterpret_cast<uint16_t*>(orow + 2 * o) = (uint16_t)(ch_u8(y.re, scale) | (ch_u8(y.im, scale) << 8));
    };

    if (rs_identity(P)) {                                                    // y = gain * x[n(m0) + i]
        const ChWindow W = rs_window(x, n_in, wrap != 0, rs_index(ta), RS_BLK);
        for (int i = t; i < cnt; i += 256) store(i, rs_finish(P, rs_load1(W, i)));
        return;
    }

    // the input window: LDS sample i = x[base + i], base even-aligned in LDS pairs through lds_shift
    const RsIndex first = rs_before(rs_index(ta), (uint64_t)(RS_TAPS / 2 - 1));
    const int lds_shift = (int)(first.n & 1);
    const RsIndex base = rs_before(first, (uint64_t)lds_shift);
    const int count = ((int)(tb.n - ta.n) + RS_TAPS + lds_shift + 1) & ~1;   // <= 2 * window_pairs (dabgpu_resample_plan)
    {
        const ChWindow W = rs_window(x, n_in, wrap != 0, base, count);
        for (int i = t; i < count / 2; i += 256) {
            chf2 a, b;
            ch_load2(W, 2 * i, a, b);
            rs_lds4[i] = ch_f4{a.re, a.im, b.re, b.im};
        }
    }
    // the rows: from the row of the block's first phase (in the direction the phase moves) to the row behind its last, or the whole table
    float* rows = reinterpret_cast<float*>(rs_lds4 + window_pairs);
    const bool narrow = rs_rows_needed(P) < (uint32_t)(RS_L + 1);
    const bool rises = rs_phase_rises(P);
    const int r0 = narrow ? rs_row(rises ? ta.frac : tb.frac) : 0;
    const int n_slots = narrow ? rs_slot(rs_row(rises ? tb.frac : ta.frac), r0) + 2 : RS_L + 1;
    for (int i = t; i < n_slots * RS_TAPS; i += 256) {
        const int slot = i / RS_TAPS, j = i - slot * RS_TAPS;
        rows[slot * RS_ROW_STRIDE + j] = table[(size_t)rs_slot_row(slot, r0) * RS_TAPS + j];
    }
    __syncthreads();

    const chf2* lds = reinterpret_cast<const chf2*>(rs_lds4);
    for (int i = t; i < cnt; i += 256) {
        const RsTime tm = rs_time(P, m0 + (uint64_t)i);
        const chf2* xs = lds + (int)(tm.n - (uint64_t)(RS_TAPS / 2 - 1) - base.n);
        const float* h = rows + rs_slot(rs_row(tm.frac), r0) * RS_ROW_STRIDE;
        const chf2 z = rs_filter(rs_weight(tm.frac), [&](int j) { return h[j]; }, [&](int j) { return h[RS_ROW_STRIDE + j]; },
                                 [&](int j) { return xs[j]; });
        store(i, rs_finish(P, z));
    }
}

}  // namespace dabgpu

using namespace dabgpu;

struct dabgpu_resample_bank : SignalBank {        // d_mem: position (16 bytes) | table | parameters
    size_t n = 0;
    dabgpu_resample_geometry geom = {};
    uint64_t max_step_q62 = 0;
    float* d_table = nullptr;
    dabgpu_resample_stream* d_params = nullptr;
};

static int rs_launch(dabgpu_resample_bank* b, const float* d_in, size_t in_stride, size_t n_in, int wrap, size_t n_out, void* d_out, int out_format,
                     size_t out_stride_bytes, float u8_scale, hipStream_t s) {
    const int tiles = (int)((n_out + RS_BLK - 1) / RS_BLK);
    const unsigned grid = (unsigned)((size_t)tiles * b->n);
    const int window_pairs = (int)((b->geom.window_samples + 1u) / 2u);
    const chf2* in = reinterpret_cast<const chf2*>(d_in);
#define RS_GO(OUT)                                                                                                                          \
    hipLaunchKernelGGL((resample_kernel<OUT>), dim3(grid), dim3(256), b->geom.lds_bytes, s, b->d_params, b->d_table, b->d_pos, in, in_stride, \
                       (int64_t)n_in, wrap, (uint32_t)n_out, tiles, static_cast<uint8_t*>(d_out), out_stride_bytes, u8_scale, window_pairs)
    if (out_format == DABGPU_IQ_RAW_F32L) RS_GO(DABGPU_IQ_RAW_F32L); else RS_GO(DABGPU_IQ_RAW_U8);
#undef RS_GO
    sb_enqueue_advance(b->d_pos, n_out, s);
    return dabgpu_check_hip(hipGetLastError(), "resample_kernel launch");
}

extern "C" {

int dabgpu_resample_bank_create(dabgpu_ctx* c, size_t n_streams, const dabgpu_resample_stream* h_params, const dabgpu_resample_filter* design,
                                dabgpu_resample_bank** out) {
    if (!c || !out) { dabgpu_set_error("resample_bank_create: null context / result"); return DABGPU_ERR_INVALID_ARG; }
    *out = nullptr;
    if (!design) { dabgpu_set_error("resample_bank_create: null design"); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_resample_geometry g;
    const uint64_t max_step_q62 = dabgpu_host_resample_max_step_q62(design->max_step);
    int st = dabgpu_host_resample_plan("resample_bank_create", h_params, n_streams, max_step_q62, &g);
    if (st) return st;
    dabgpu_resample_bank* b = new (std::nothrow) dabgpu_resample_bank;
    if (!b) return DABGPU_ERR_HIP;
    b->ctx = c; b->n = n_streams; b->geom = g; b->max_step_q62 = max_step_q62;
    auto fail = [&](int status) { dabgpu_resample_bank_destroy(b); return status; };
    if ((st = dabgpu_bind_device(c))) return fail(st);
    if (g.lds_bytes > 48u * 1024u) {        // the whole table beside a wide window: raise the kernels' limit once, to the largest geometry there is
        constexpr int most = ((2 * RS_BLK + RS_TAPS + 2 + 1) & ~1) * 8 + (RS_L + 1) * RS_ROW_STRIDE * 4;
        if ((st = dabgpu_check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(resample_kernel<DABGPU_IQ_RAW_F32L>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, most), "hipFuncSetAttribute(resample_kernel)")) ||
            (st = dabgpu_check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(resample_kernel<DABGPU_IQ_RAW_U8>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, most), "hipFuncSetAttribute(resample_kernel)")))
            return fail(st);
    }
    const size_t table_bytes = sizeof(design->table);
    static_assert(sizeof(dabgpu_resample_filter::table) % 16 == 0, "the parameters behind the table stay 8-byte aligned");
    uint8_t* payload;
    if ((st = sb_alloc(b, table_bytes + n_streams * sizeof(dabgpu_resample_stream), "resample", &payload))) return fail(st);
    b->d_table = reinterpret_cast<float*>(payload);
    b->d_params = reinterpret_cast<dabgpu_resample_stream*>(payload + table_bytes);
    if ((st = dabgpu_stage_h2d(c, b->d_table, design->table, table_bytes, c->stream))) return fail(st);
    if ((st = dabgpu_stage_h2d(c, b->d_params, h_params, n_streams * sizeof(dabgpu_resample_stream), c->stream))) return fail(st);
    if ((st = dabgpu_check_hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize(resample_bank_create)"))) return fail(st);
    *out = b;
    return DABGPU_OK;
}

void dabgpu_resample_bank_destroy(dabgpu_resample_bank* b) {
    if (!dabgpu_destroy_begin(b, b ? b->ctx : nullptr)) return;
    delete b;
}

int dabgpu_resample_bank_set_params(dabgpu_resample_bank* b, const dabgpu_resample_stream* h_params, void* stream) {
    if (!b) { dabgpu_set_error("resample_bank_set_params: null bank"); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_resample_geometry g;
    int st = dabgpu_host_resample_plan("resample_bank_set_params", h_params, b->n, b->max_step_q62, &g);
    if (st || (st = dabgpu_host_resample_fits(b->geom, g))) return st;      // (b->geom stays: captured calls launch with it)
    DABGPU_BIND(b->ctx);
    return dabgpu_stage_h2d(b->ctx, b->d_params, h_params, b->n * sizeof(dabgpu_resample_stream), (hipStream_t)stream);
}

int dabgpu_resample_bank_seek(dabgpu_resample_bank* b, uint64_t position, void* stream) {
    return sb_seek(b, "resample_bank_seek", position, (uint64_t)DABGPU_CHANNEL_MAX_POSITION, "2^62", stream);
}

int dabgpu_resample_bank_apply(dabgpu_resample_bank* b, const float* d_in, size_t in_stride_samples, size_t n_in, int wrap, size_t n_out, void* d_out,
                               int out_format, size_t out_stride_bytes, float u8_scale, void* stream) {
    if (!b) { dabgpu_set_error("resample_bank_apply: null bank"); return DABGPU_ERR_INVALID_ARG; }
    const int st = dabgpu_host_channel_check_apply("resample_bank_apply", b->n, d_in, in_stride_samples, n_in, n_out, d_out, out_format, &out_stride_bytes,
                                                   u8_scale);
    if (st || n_out == 0) return st;
    DABGPU_BIND(b->ctx);
    return rs_launch(b, d_in, in_stride_samples, n_in, wrap, n_out, d_out, out_format, out_stride_bytes, u8_scale, (hipStream_t)stream);
}

int dabgpu_resample_bank_apply_host_sync(dabgpu_resample_bank* b, const float* h_in, size_t in_stride_samples, size_t n_in, int wrap, size_t n_out,
                                         void* h_out, int out_format, size_t out_stride_bytes, float u8_scale) {
    if (!b) { dabgpu_set_error("resample_bank_apply_host_sync: null bank"); return DABGPU_ERR_INVALID_ARG; }
    const int st = dabgpu_host_channel_check_apply("resample_bank_apply_host_sync", b->n, h_in, in_stride_samples, n_in, n_out, h_out, out_format,
                                                   &out_stride_bytes, u8_scale, false);
    if (st || n_out == 0) return st;
    return sb_host_round_trip(b, b->n, b->n, false, h_in, in_stride_samples, n_in, n_out, h_out, out_format, out_stride_bytes,
                              [&](const float* d_in, size_t d_in_stride, void* d_out, size_t d_out_stride, hipStream_t s) {
                                  return rs_launch(b, d_in, d_in_stride, n_in, wrap, n_out, d_out, out_format, d_out_stride, u8_scale, s);
                              });
}

}  // extern "C"
