// channelise.hip -- the channeliser on the device (include/dabgpu.h, "Channeliser"): SPLIT, a frequency-translating, integer-decimating
// bank (one wideband stream in, up to 8 block streams out), and COMBINE, its transpose.  Every arithmetic step is channelise_core.h's;
// this file is where the samples and the coefficients come from and go to.
//
// Split: one 128-thread workgroup per (wideband stream, tile of 512 outputs), looping over the stream's channels.  The tile's raw window
// -- (512 + 72) block-rate positions of D wideband samples -- goes to LDS ONCE per stream (wrap and zero-fill resolved there, the loads
// of channel_device.h): the HBM bytes of a call are the input once plus the outputs.  Per channel the window is rotated into a second LDS
// buffer; a channel with both oscillator words 0 filters the raw buffer.  Both buffers are laid out by residue: window sample i sits in
// plane i mod 4 D at index i / 4 D, planes 147 samples apart.  Lane l produces the four consecutive outputs 4 l .. 4 l + 3; tap
// j = a D + r of output m reads the sample at block-rate position m + a of residue r, so for a fixed tap and output the 64 lanes of a
// wavefront read neighbouring 8-byte words of one plane (conflict-free; a stride of D samples would collide on the 64 banks for even D),
// and the seven samples a lane loads per residue and four steps of `a` serve its four outputs: 4 x 4 x 2 fmaf per 7 reads.  The
// coefficient of a tap is the same for every lane: it is read through the table pointer at a uniform index (scalar loads).
// D = 1, the mixer, stages nothing: every lane reads its input sample once and rotates it per channel.
//
// Combine: one 128-thread workgroup per (wideband stream, tile of 128 block-rate positions = 128 D wideband samples).  Wideband sample
// q D + rho takes the 72 block samples q - 71 .. q under the taps rho + (71 - k) D: lane l owns position q0 + l and its D residues, so
// one 8-byte LDS read (neighbouring lanes, neighbouring words) serves 2 D fmaf and the coefficient is again uniform.  Each channel's
// window of 128 + 71 block samples is staged in turn; the tile is accumulated in registers and stored once.
//
// Parameters, the position and `start` are read through pointers that are the same for the whole workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <new>
#include <vector>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "channelise_core.h"
#include "channel_device.h"
#include "signal_bank.h"

namespace dabgpu {

constexpr int CS_THREADS = 128;
constexpr int CS_RUN = 4;                                                    // consecutive outputs of a lane (split)
constexpr int CS_TILE = DABGPU_CHANNELISER_SPLIT_TILE;
constexpr int CS_ROWS = DABGPU_CHANNELISER_COMBINE_ROWS;
constexpr int CS_UNITS = (CS_TILE + CS_TPP) / CS_RUN;                         // 146 indices of a plane are staged and read
constexpr int CS_PLANE = CS_UNITS + 1;                                       // samples between planes (odd)
static_assert(CS_TILE == CS_THREADS * CS_RUN && CS_TPP % CS_RUN == 0 && CS_ROWS == CS_THREADS, "tile shape");

// sample `off` of the window alone
__device__ __forceinline__ chf2 cs_load1(const ChWindow& W, int off) {
    int64_t j = W.origin + off;
    if (W.wrap) {
        if (j >= W.n_in) j = (W.span <= W.n_in) ? j - W.n_in : j % W.n_in;
        return ch_ld(W.x + j);
    }
    return (j >= 0 && j < W.n_in) ? ch_ld(W.x + j) : chf2{0.0f, 0.0f};
}

__device__ __forceinline__ void cs_store(float* row, size_t o, chf2 y) {
    __builtin_nontemporal_store(ch_f2v{y.re, y.im}, reinterpret_cast<ch_f2v*>(row) + o);
}

template <int D>
__global__ __launch_bounds__(CS_THREADS)
void channelise_split_kernel(const dabgpu_channeliser_channel* __restrict__ channels, const uint32_t* __restrict__ first_of, const float* __restrict__ table,
                             const uint64_t* __restrict__ d_pos, const int64_t* __restrict__ d_start, const chf2* __restrict__ in, size_t in_stride,
                             int64_t n_in, int wrap, uint32_t n_out, int tiles, float* __restrict__ out, size_t out_stride_bytes)
{
    const int t = threadIdx.x;
    const uint32_t s = blockIdx.x / (uint32_t)tiles, tile = blockIdx.x % (uint32_t)tiles;
    const uint32_t c0 = first_of[s], c1 = first_of[s + 1];
    if (c0 == c1) return;
    const uint32_t o0 = tile * (uint32_t)CS_TILE;                            // the tile's first output inside the call
    const int cnt = (n_out - o0 < (uint32_t)CS_TILE) ? (int)(n_out - o0) : CS_TILE;
    const int64_t start = *d_start;
    const int64_t n_first = cs_split_first(D, *d_pos + o0, start);           // the wideband index of window sample 0
    const chf2* x = in + (size_t)s * in_stride;

    if constexpr (D == 1) {
        const ChWindow W = ch_window(x, n_in, wrap != 0, (uint64_t)n_first, CS_TILE);
        const float h0 = table[0];
        for (int i = t; i < cnt; i += CS_THREADS) {
            const chf2 v = cs_load1(W, i);
            for (uint32_t c = c0; c < c1; c++) {
                const dabgpu_channeliser_channel C = channels[c];
                const chf2 acc = cs_tap(cs_chain_start(), h0, cs_mix_down(C, v, (uint64_t)(n_first + i)));
                cs_store(reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(out) + (size_t)c * out_stride_bytes), (size_t)o0 + (size_t)i, cs_scale(C.gain, acc));
            }
        }
    } else {
        constexpr int DR = D * CS_RUN, BUF = DR * CS_PLANE, WIN = DR * CS_UNITS;
        extern __shared__ __attribute__((aligned(16))) ch_f2v cs_lds[];      // [BUF] the raw window, [BUF] the rotated one
        ch_f2v* raw = cs_lds;
        ch_f2v* rot = cs_lds + BUF;
        {
            const ChWindow W = ch_window(x, n_in, wrap != 0, (uint64_t)n_first, WIN);
            for (int p = t; p < WIN / 2; p += CS_THREADS) {
                chf2 a, b;
                ch_load2(W, 2 * p, a, b);
                const int i0 = 2 * p, i1 = 2 * p + 1;
                raw[(i0 % DR) * CS_PLANE + i0 / DR] = ch_f2v{a.re, a.im};
                raw[(i1 % DR) * CS_PLANE + i1 / DR] = ch_f2v{b.re, b.im};
            }
        }
        __syncthreads();
        for (uint32_t c = c0; c < c1; c++) {
            const dabgpu_channeliser_channel C = channels[c];
            const bool mixes = cs_mixes(C);
            if (mixes) {
                for (int e = t; e < BUF; e += CS_THREADS) {
                    const int plane = e / CS_PLANE, u = e - plane * CS_PLANE;
                    if (u < CS_UNITS) {
                        const ch_f2v v = raw[e];
                        const chf2 r = cs_mix_down(C, chf2{v.x, v.y}, (uint64_t)(n_first + (int64_t)(u * DR + plane)));
                        rot[e] = ch_f2v{r.re, r.im};
                    }
                }
                __syncthreads();
            }
            const ch_f2v* src = (mixes ? rot : raw) + t;                     // index u of lane t at a = 0
            chf2 acc[CS_RUN];
#pragma unroll
            for (int i = 0; i < CS_RUN; i++) acc[i] = cs_chain_start();
            for (int a0 = 0; a0 < CS_TPP; a0 += CS_RUN) {
                // block-rate positions 4 (t + a0 / 4) + e, e = 0 .. 6, of every residue
                chf2 sm[D][2 * CS_RUN - 1];
#pragma unroll
                for (int r = 0; r < D; r++) {
#pragma unroll
                    for (int e = 0; e < 2 * CS_RUN - 1; e++) {
                        const ch_f2v v = src[((e % CS_RUN) * D + r) * CS_PLANE + a0 / CS_RUN + e / CS_RUN];
                        sm[r][e] = chf2{v.x, v.y};
                    }
                }
#pragma unroll
                for (int k = 0; k < CS_RUN; k++) {
#pragma unroll
                    for (int r = 0; r < D; r++) {
                        const float h = table[(a0 + k) * D + r];
#pragma unroll
                        for (int i = 0; i < CS_RUN; i++) acc[i] = cs_tap(acc[i], h, sm[r][k + i]);
                    }
                }
            }
            float* row = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(out) + (size_t)c * out_stride_bytes);
#pragma unroll
            for (int i = 0; i < CS_RUN; i++)
                if (CS_RUN * t + i < cnt) cs_store(row, (size_t)o0 + (size_t)(CS_RUN * t + i), cs_scale(C.gain, acc[i]));
            if (mixes) __syncthreads();                                      // the next channel rotates into the same buffer
        }
    }
}

template <int D, int OUT>
__global__ __launch_bounds__(CS_THREADS)
void channelise_combine_kernel(const dabgpu_channeliser_channel* __restrict__ channels, const uint32_t* __restrict__ first_of,
                               const float* __restrict__ table, const uint64_t* __restrict__ d_pos, const int64_t* __restrict__ d_start,
                               const chf2* __restrict__ in, size_t in_stride, int64_t n_in, int wrap, uint32_t n_out, int tiles,
                               uint8_t* __restrict__ out, size_t out_stride_bytes, float scale)
{
    constexpr int NT = cs_phase_taps(D), COUNT = (CS_ROWS + NT - 1 + 1) & ~1;
    extern __shared__ __attribute__((aligned(16))) ch_f2v cs_lds[];          // [COUNT] block samples q0 - (NT - 1) .. of the channel in turn
    const int t = threadIdx.x;
    const uint32_t s = blockIdx.x / (uint32_t)tiles, tile = blockIdx.x % (uint32_t)tiles;
    const uint32_t c0 = first_of[s], c1 = first_of[s + 1];
    const int64_t start = *d_start, pos = (int64_t)*d_pos;
    const int64_t q0 = cs_floor_div(cs_combine_t(D, pos, start), D) + (int64_t)tile * CS_ROWS, q = q0 + t;
    const int64_t n0 = q * D + start - cs_peak(D);                           // the wideband sample of (q, rho = 0)

    chf2 y[D];
#pragma unroll
    for (int rho = 0; rho < D; rho++) y[rho] = chf2{0.0f, 0.0f};
    for (uint32_t c = c0; c < c1; c++) {
        const dabgpu_channeliser_channel C = channels[c];
        if (c != c0) __syncthreads();
        {
            const ChWindow W = ch_window(in + (size_t)c * in_stride, n_in, wrap != 0, (uint64_t)(q0 - (NT - 1)), COUNT);
            for (int p = t; p < COUNT / 2; p += CS_THREADS) {
                chf2 a, b;
                ch_load2(W, 2 * p, a, b);
                cs_lds[2 * p] = ch_f2v{a.re, a.im};
                cs_lds[2 * p + 1] = ch_f2v{b.re, b.im};
            }
        }
        __syncthreads();
        chf2 acc[D];
#pragma unroll
        for (int rho = 0; rho < D; rho++) acc[rho] = cs_chain_start();
#pragma unroll
        for (int k = 0; k < NT; k++) {
            const ch_f2v v = cs_lds[t + k];
#pragma unroll
            for (int rho = 0; rho < D; rho++) acc[rho] = cs_tap(acc[rho], table[cs_combine_tap(D, rho, k)], chf2{v.x, v.y});
        }
#pragma unroll
        for (int rho = 0; rho < D; rho++) {
            const chf2 term = cs_combine_finish(C, D, acc[rho], (uint64_t)(n0 + rho));
            y[rho] = (c == c0) ? term : cs_add(y[rho], term);
        }
    }
    uint8_t* orow = out + (size_t)s * out_stride_bytes;
#pragma unroll
    for (int rho = 0; rho < D; rho++) {
        const int64_t i = n0 + rho - pos;
        if (i >= 0 && i < (int64_t)n_out) {
            if constexpr (OUT == DABGPU_IQ_RAW_F32L) cs_store(reinterpret_cast<float*>(orow), (size_t)i, y[rho]);
            else *reinterpret_cast<uint16_t*>(orow + 2 * (size_t)i) = (uint16_t)(ch_u8(y[rho].re, scale) | (ch_u8(y[rho].im, scale) << 8));
        }
    }
}

}  // namespace dabgpu

using namespace dabgpu;

struct dabgpu_channeliser_bank : SignalBank {     // d_mem: position (16 bytes) | table | start (16 bytes) | first_of | channels
    size_t n_streams = 0, capacity = 0, n_channels = 0;                      // channels the bank has room for / of the list in force
    int decim = 1;
    dabgpu_channeliser_geometry geom = {};
    float* d_table = nullptr;
    int64_t* d_start = nullptr;
    uint32_t* d_first = nullptr;
    dabgpu_channeliser_channel* d_channels = nullptr;
    size_t first_bytes = 0;
};

// start | first_of | channels as one block, as it lies on the device
static int cs_upload(dabgpu_channeliser_bank* b, const char* who, const dabgpu_channeliser_channel* h_channels, size_t n_channels, int64_t start,
                     hipStream_t s) {
    std::vector<uint8_t> block(16 + b->first_bytes + b->capacity * sizeof(dabgpu_channeliser_channel), 0);
    dabgpu_channeliser_geometry g;
    const int st = dabgpu_host_channeliser_plan(who, h_channels, n_channels, b->n_streams, start, b->decim, &g, reinterpret_cast<uint32_t*>(block.data() + 16));
    if (st) return st;
    memcpy(block.data(), &start, sizeof(start));
    memcpy(block.data() + 16 + b->first_bytes, h_channels, n_channels * sizeof(dabgpu_channeliser_channel));
    const int up = dabgpu_stage_h2d(b->ctx, b->d_start, block.data(), block.size(), s);
    if (up == DABGPU_OK) b->n_channels = n_channels;
    return up;
}

#define CS_EACH_D(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

static int cs_launch_split(dabgpu_channeliser_bank* b, const float* d_in, size_t in_stride, size_t n_in, int wrap, size_t n_out, float* d_out,
                           size_t out_stride_bytes, hipStream_t s) {
    uint32_t tiles;
    const int st = dabgpu_host_channeliser_tiles("channeliser_bank_split", n_out, CS_TILE, b->n_streams, &tiles);
    if (st) return st;
    const unsigned grid = (unsigned)((size_t)tiles * b->n_streams);
    const chf2* in = reinterpret_cast<const chf2*>(d_in);
    switch (b->decim) {
#define CS_GO(DD)                                                                                                                            \
    case DD: hipLaunchKernelGGL((channelise_split_kernel<DD>), dim3(grid), dim3(CS_THREADS), b->geom.split_lds_bytes, s, b->d_channels, b->d_first, \
                                b->d_table, b->d_pos, b->d_start, in, in_stride, (int64_t)n_in, wrap, (uint32_t)n_out, (int)tiles, d_out,       \
                                out_stride_bytes); break;
        CS_EACH_D(CS_GO)
#undef CS_GO
    }
    sb_enqueue_advance(b->d_pos, n_out, s);
    return dabgpu_check_hip(hipGetLastError(), "channelise_split_kernel launch");
}

static int cs_launch_combine(dabgpu_channeliser_bank* b, const float* d_in, size_t in_stride, size_t n_in, int wrap, size_t n_out, void* d_out,
                             int out_format, size_t out_stride_bytes, float u8_scale, hipStream_t s) {
    // (a call may begin inside a tile: up to D - 1 samples of the first tile lie before it)
    uint32_t tiles;
    const int st = dabgpu_host_channeliser_tiles("channeliser_bank_combine", n_out + (size_t)(b->decim - 1), b->geom.combine_tile, b->n_streams, &tiles);
    if (st) return st;
    const unsigned grid = (unsigned)((size_t)tiles * b->n_streams);
    const chf2* in = reinterpret_cast<const chf2*>(d_in);
    switch (b->decim) {
#define CS_GO2(DD, OUT)                                                                                                                       \
    hipLaunchKernelGGL((channelise_combine_kernel<DD, OUT>), dim3(grid), dim3(CS_THREADS), b->geom.combine_lds_bytes, s, b->d_channels, b->d_first, \
                       b->d_table, b->d_pos, b->d_start, in, in_stride, (int64_t)n_in, wrap, (uint32_t)n_out, (int)tiles, static_cast<uint8_t*>(d_out), \
                       out_stride_bytes, u8_scale)
#define CS_GO(DD) case DD: if (out_format == DABGPU_IQ_RAW_F32L) CS_GO2(DD, DABGPU_IQ_RAW_F32L); else CS_GO2(DD, DABGPU_IQ_RAW_U8); break;
        CS_EACH_D(CS_GO)
#undef CS_GO
#undef CS_GO2
    }
    sb_enqueue_advance(b->d_pos, n_out, s);
    return dabgpu_check_hip(hipGetLastError(), "channelise_combine_kernel launch");
}

extern "C" {

int dabgpu_channeliser_bank_create(dabgpu_ctx* c, const dabgpu_channeliser_channel* h_channels, size_t n_channels, size_t n_streams, int64_t start,
                                   const dabgpu_channeliser_filter* design, dabgpu_channeliser_bank** out) {
    if (!c || !out) { dabgpu_set_error("channeliser_bank_create: null context / result"); return DABGPU_ERR_INVALID_ARG; }
    *out = nullptr;
    if (!design) { dabgpu_set_error("channeliser_bank_create: null design"); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_channeliser_geometry g;
    int st = dabgpu_host_channeliser_plan("channeliser_bank_create", h_channels, n_channels, n_streams, start, design->decim, &g, nullptr);
    if (st) return st;
    dabgpu_channeliser_bank* b = new (std::nothrow) dabgpu_channeliser_bank;
    if (!b) return DABGPU_ERR_HIP;
    b->ctx = c; b->n_streams = n_streams; b->capacity = n_channels; b->decim = design->decim; b->geom = g;
    b->first_bytes = ((n_streams + 1) * sizeof(uint32_t) + 15) & ~(size_t)15;
    auto fail = [&](int status) { dabgpu_channeliser_bank_destroy(b); return status; };
    if ((st = dabgpu_bind_device(c))) return fail(st);
    if (g.split_lds_bytes > 48u * 1024u) {
        const void* fn = nullptr;
        switch (b->decim) {
#define CS_FN(DD) case DD: fn = reinterpret_cast<const void*>(channelise_split_kernel<DD>); break;
            CS_EACH_D(CS_FN)
#undef CS_FN
        }
        if ((st = dabgpu_check_hip(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.split_lds_bytes),
                                   "hipFuncSetAttribute(channelise_split_kernel)")))
            return fail(st);
    }
    const size_t table_bytes = sizeof(design->table), params_bytes = 16 + b->first_bytes + n_channels * sizeof(dabgpu_channeliser_channel);
    static_assert(sizeof(dabgpu_channeliser_filter::table) % 16 == 0 && sizeof(dabgpu_channeliser_channel) == 24, "the layout of the bank's block");
    uint8_t* payload;
    if ((st = sb_alloc(b, table_bytes + params_bytes, "channeliser", &payload))) return fail(st);
    b->d_table = reinterpret_cast<float*>(payload);
    b->d_start = reinterpret_cast<int64_t*>(payload + table_bytes);
    b->d_first = reinterpret_cast<uint32_t*>(payload + table_bytes + 16);
    b->d_channels = reinterpret_cast<dabgpu_channeliser_channel*>(payload + table_bytes + 16 + b->first_bytes);
    if ((st = dabgpu_stage_h2d(c, b->d_table, design->table, table_bytes, c->stream))) return fail(st);
    if ((st = cs_upload(b, "channeliser_bank_create", h_channels, n_channels, start, c->stream))) return fail(st);
    if ((st = dabgpu_check_hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize(channeliser_bank_create)"))) return fail(st);
    *out = b;
    return DABGPU_OK;
}

void dabgpu_channeliser_bank_destroy(dabgpu_channeliser_bank* b) {
    if (!dabgpu_destroy_begin(b, b ? b->ctx : nullptr)) return;
    delete b;
}

int dabgpu_channeliser_bank_set_params(dabgpu_channeliser_bank* b, const dabgpu_channeliser_channel* h_channels, size_t n_channels, int64_t start,
                                       void* stream) {
    if (!b) { dabgpu_set_error("channeliser_bank_set_params: null bank"); return DABGPU_ERR_INVALID_ARG; }
    if (n_channels > b->capacity) {                                         // (the room for the list is fixed at creation: captured calls read it)
        dabgpu_set_error("channeliser_bank_set_params: %zu channels, the bank was created with %zu", n_channels, b->capacity); return DABGPU_ERR_INVALID_ARG;
    }
    DABGPU_BIND(b->ctx);
    return cs_upload(b, "channeliser_bank_set_params", h_channels, n_channels, start, (hipStream_t)stream);
}

int dabgpu_channeliser_bank_seek(dabgpu_channeliser_bank* b, uint64_t position, void* stream) {
    return sb_seek(b, "channeliser_bank_seek", position, (uint64_t)DABGPU_CHANNELISER_MAX_POSITION, "2^58", stream);
}

int dabgpu_channeliser_bank_split(dabgpu_channeliser_bank* b, const float* d_in, size_t in_stride_samples, size_t n_in, int wrap, size_t n_out,
                                  float* d_out, size_t out_stride_bytes, void* stream) {
    if (!b) { dabgpu_set_error("channeliser_bank_split: null bank"); return DABGPU_ERR_INVALID_ARG; }
    // (the buffer rules of the channel bank; its grid rule is passed one row: this kernel's own grid is checked by cs_launch_split)
    const int st = dabgpu_host_channel_check_apply("channeliser_bank_split", 1, d_in, in_stride_samples, n_in, n_out, d_out, DABGPU_IQ_RAW_F32L,
                                                   &out_stride_bytes, 1.0f);
    if (st || n_out == 0) return st;
    DABGPU_BIND(b->ctx);
    return cs_launch_split(b, d_in, in_stride_samples, n_in, wrap, n_out, d_out, out_stride_bytes, (hipStream_t)stream);
}

int dabgpu_channeliser_bank_combine(dabgpu_channeliser_bank* b, const float* d_in, size_t in_stride_samples, size_t n_in, int wrap, size_t n_out,
                                    void* d_out, int out_format, size_t out_stride_bytes, float u8_scale, void* stream) {
    if (!b) { dabgpu_set_error("channeliser_bank_combine: null bank"); return DABGPU_ERR_INVALID_ARG; }
    const int st = dabgpu_host_channel_check_apply("channeliser_bank_combine", 1, d_in, in_stride_samples, n_in, n_out, d_out, out_format,
                                                   &out_stride_bytes, u8_scale);                       // (the grid: cs_launch_combine)
    if (st || n_out == 0) return st;
    DABGPU_BIND(b->ctx);
    return cs_launch_combine(b, d_in, in_stride_samples, n_in, wrap, n_out, d_out, out_format, out_stride_bytes, u8_scale, (hipStream_t)stream);
}

// the host forms zero the output rows first (split: the rows of streams without a channel)
int dabgpu_channeliser_bank_split_host_sync(dabgpu_channeliser_bank* b, const float* h_in, size_t in_stride_samples, size_t n_in, int wrap, size_t n_out,
                                            float* h_out, size_t out_stride_bytes) {
    if (!b) { dabgpu_set_error("channeliser_bank_split_host_sync: null bank"); return DABGPU_ERR_INVALID_ARG; }
    // (the grid: cs_launch_split)
    const int st = dabgpu_host_channel_check_apply("channeliser_bank_split_host_sync", 1, h_in, in_stride_samples, n_in, n_out, h_out, DABGPU_IQ_RAW_F32L,
                                                   &out_stride_bytes, 1.0f, false);
    if (st || n_out == 0) return st;
    return sb_host_round_trip(b, b->n_streams, b->n_channels, true, h_in, in_stride_samples, n_in, n_out, h_out, DABGPU_IQ_RAW_F32L, out_stride_bytes,
                              [&](const float* d_in, size_t d_in_stride, void* d_out, size_t d_out_stride, hipStream_t s) {
                                  return cs_launch_split(b, d_in, d_in_stride, n_in, wrap, n_out, static_cast<float*>(d_out), d_out_stride, s);
                              });
}

int dabgpu_channeliser_bank_combine_host_sync(dabgpu_channeliser_bank* b, const float* h_in, size_t in_stride_samples, size_t n_in, int wrap, size_t n_out,
                                              void* h_out, int out_format, size_t out_stride_bytes, float u8_scale) {
    if (!b) { dabgpu_set_error("channeliser_bank_combine_host_sync: null bank"); return DABGPU_ERR_INVALID_ARG; }
    // (the grid: cs_launch_combine)
    const int st = dabgpu_host_channel_check_apply("channeliser_bank_combine_host_sync", 1, h_in, in_stride_samples, n_in, n_out, h_out, out_format,
                                                   &out_stride_bytes, u8_scale, false);
    if (st || n_out == 0) return st;
    return sb_host_round_trip(b, b->n_channels, b->n_streams, true, h_in, in_stride_samples, n_in, n_out, h_out, out_format, out_stride_bytes,
                              [&](const float* d_in, size_t d_in_stride, void* d_out, size_t d_out_stride, hipStream_t s) {
                                  return cs_launch_combine(b, d_in, d_in_stride, n_in, wrap, n_out, d_out, out_format, d_out_stride, u8_scale, s);
                              });
}

}  // extern "C"
