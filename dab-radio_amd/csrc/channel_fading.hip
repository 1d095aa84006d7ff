// channel_fading.hip -- the channel model's fading kernel (include/dabgpu.h, "Channel model, fading taps"): the staged kernel of channel.hip
// -- same tiles, same staging, same stores -- with a gain phase in front of the sample loop.  Every arithmetic step is channel_core.h's.
//
// Gain phase: the tile touches the grid points (T0 >> 6) .. ((T0 + hi' - 1) >> 6) + 1, hi' = hi rounded up to the 4 samples a thread may
// compute: at most 18, because tiles are aligned to 4 and not to 64.  One 16-lane group per (grid point, fading tap): lane n evaluates
// diffuse oscillator n, four register exchanges (v += v of lane ^ 1, ^ 2, ^ 4, ^ 8) are the definition's pairwise tree, lane 0 adds the
// line of sight and writes G to LDS at [point][tap] behind the staged input (8 taps x 8 bytes = 64 bytes a point: the 4 writes of a
// wavefront go to consecutive 8-byte slots; in the sample loop the 32 lanes of a half wavefront cover at most 128 samples = 3 grid
// intervals, whose slots of one tap lie 16 banks apart, and lanes on one interval read one address).  The table row and the kinds come
// through workgroup-uniform pointers; the oscillators of a lane's (tap, n) through ordinary loads.  The barrier behind the staging loop
// covers the gains.  Per sample pair and fading tap: two 8-byte LDS reads, two interpolations, two complex products.  A stream without
// a fading tap runs no gain phase and sums its taps exactly as the plain kernel does.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "channel_core.h"
#include "channel_device.h"

namespace dabgpu {

template <int OUT>
__global__ __launch_bounds__(256)
void channel_fading_kernel(const dabgpu_channel_stream* __restrict__ params, const dabgpu_channel_fading_stream* __restrict__ tables,
                           const uint64_t* __restrict__ d_pos, const chf2* __restrict__ in, size_t in_stride, int64_t n_in, int wrap, uint32_t n_out,
                           int tiles, int gain_off, uint8_t* __restrict__ out, size_t out_stride_bytes, float scale)
{
    extern __shared__ __attribute__((aligned(16))) ch_f4 ch_lds4[];
    constexpr int SPT = (OUT == DABGPU_IQ_RAW_F32L) ? 2 : 4;            // samples per thread and pass
    const int t = threadIdx.x;
    const uint32_t s = blockIdx.x / (uint32_t)tiles, tile = blockIdx.x % (uint32_t)tiles;
    const dabgpu_channel_stream& P = params[s];
    const dabgpu_channel_fading_stream& F = tables[s];
    const uint64_t pos = *d_pos;
    const uint64_t T0 = (pos & ~(uint64_t)3) + (uint64_t)tile * CH_BLK;       // absolute number of the tile's first sample
    const uint64_t rel0 = T0 - pos;                                          // -3 .. 0 (as unsigned) for tile 0
    const int lo = (tile == 0) ? (int)(pos & 3) : 0;
    const int64_t left = (int64_t)n_out - (int64_t)rel0;                      // samples from T0 to the call's end
    if (left <= lo) return;
    const int hi = left < CH_BLK ? (int)left : CH_BLK;
    const chf2* x = in + (size_t)s * in_stride;
    uint8_t* orow = out + (size_t)s * out_stride_bytes;
    const bool aligned = (pos & (uint64_t)(SPT - 1)) == 0;

    const chf2* lds = reinterpret_cast<const chf2*>(ch_lds4);
    chf2* ldsg = reinterpret_cast<chf2*>(ch_lds4) + gain_off;                 // G of (grid point p, tap k) at [p * 8 + k]
    const int halo = ch_stream_halo(P);
    const uint64_t base = T0 - (uint64_t)P.start - (uint64_t)halo;
    const int lds_shift = (int)(base & 1);                                   // LDS sample i = x[T0 - start - halo - lds_shift + i]
    const int count = (hi + halo + lds_shift + 1) & ~1;                      // <= CH_BLK + halo + 2 <= gain_off
    const ChWindow W = ch_window(x, n_in, wrap != 0, base - (uint64_t)lds_shift, count);
    for (int i = t; i < count / 2; i += 256) {
        chf2 a, b;
        ch_load2(W, 2 * i, a, b);
        ch_lds4[i] = ch_f4{a.re, a.im, b.re, b.im};
    }

    const uint32_t mask = ch_fading_mask(F, P.n_taps);
    const uint64_t j0 = T0 >> CH_FADE_GRID_SHIFT;
    if (mask != 0) {
        int nf = 0;
        uint32_t order = 0;                                                  // nibble f = the f-th fading tap
        for (int k = 0; k < DABGPU_CHANNEL_MAX_TAPS; k++)
            if ((mask >> k) & 1u) { order |= (uint32_t)k << (4 * nf); nf++; }
        const int npts = (int)(((T0 + (uint64_t)(((hi + 3) & ~3) - 1)) >> CH_FADE_GRID_SHIFT) - j0) + 2;     // <= CH_FADE_MAX_POINTS
        const int total = npts * nf * 16;                                    // a multiple of 16: a 16-lane group is live or idle as a whole
        for (int first = 0; first < total; first += 256) {                   // (the same trip count for every lane: all take part in the exchanges)
            const int i = first + t;
            const bool live = i < total;
            const int g = live ? (i >> 4) : 0, n = i & 15;
            const int p = g / nf, f = g - p * nf;
            const int k = (int)((order >> (4 * f)) & 7u);
            const dabgpu_channel_fading_tap& T = F.tap[k];
            const uint64_t j = j0 + (uint64_t)p;
            const chf2 cs = ch_fading_osc(T, n, j);
            float c = cs.re, sn = cs.im;
#pragma unroll
            for (int stride = 1; stride < 16; stride <<= 1) {
                const float c2 = __shfl_xor(c, stride), s2 = __shfl_xor(sn, stride);
                c = c + c2; sn = sn + s2;
            }
            if (live && n == 0) {
                const chf2 los = (T.amp_los != 0.0f) ? ch_fading_osc(T, 16, j) : chf2{0.0f, 0.0f};
                ldsg[p * DABGPU_CHANNEL_MAX_TAPS + k] = ch_fading_combine(T.amp_diffuse, T.amp_los, chf2{c, sn}, los);
            }
        }
    }
    __syncthreads();

    const bool noisy = P.noise_sigma != 0.0f;
    for (int q = t; q < CH_BLK / SPT; q += 256) {
        const int n0 = SPT * q;                                              // tile-local number of the thread's first sample
        if (n0 + SPT <= lo || n0 >= hi) continue;
        chf2 y[SPT];
#pragma unroll
        for (int h = 0; h < SPT; h += 2) {
            const uint64_t m = T0 + (uint64_t)(n0 + h);                      // even: m and m + 1 lie between the same two grid points
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            if (noisy) ch_noise_words(P.seed, s, m >> 1, w);
            const int li = n0 + h + halo + lds_shift;
            const chf2* G = ldsg + (int)((m >> CH_FADE_GRID_SHIFT) - j0) * DABGPU_CHANNEL_MAX_TAPS;
            const chf2 z0 = ch_paths_fading(P, mask, [&](int k) { return ch_fading_interp(G[k], G[DABGPU_CHANNEL_MAX_TAPS + k], m); },
                                            [&](int k) { return lds[li - P.tap_delay[k]]; });
            const chf2 z1 = ch_paths_fading(P, mask, [&](int k) { return ch_fading_interp(G[k], G[DABGPU_CHANNEL_MAX_TAPS + k], m + 1); },
                                            [&](int k) { return lds[li + 1 - P.tap_delay[k]]; });
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

// the fading kernel of a call on the tiles and the grid of ch_launch (channel.hip), which adds the position's advance behind it
void ch_launch_fading(const dabgpu_channel_stream* d_params, const dabgpu_channel_fading_stream* d_tables, const uint64_t* d_pos,
                      const dabgpu_channel_geometry& geom, int tiles, unsigned grid, const float* d_in, size_t in_stride, size_t n_in, int wrap, size_t n_out,
                      void* d_out, int out_format, size_t out_stride_bytes, float u8_scale, hipStream_t s) {
    const int gain_off = CH_BLK + (int)geom.halo + 2;
    const chf2* in = reinterpret_cast<const chf2*>(d_in);
    if (out_format == DABGPU_IQ_RAW_F32L)
        hipLaunchKernelGGL((channel_fading_kernel<DABGPU_IQ_RAW_F32L>), dim3(grid), dim3(256), geom.lds_bytes, s, d_params, d_tables, d_pos, in, in_stride,
                           (int64_t)n_in, wrap, (uint32_t)n_out, tiles, gain_off, static_cast<uint8_t*>(d_out), out_stride_bytes, u8_scale);
    else
        hipLaunchKernelGGL((channel_fading_kernel<DABGPU_IQ_RAW_U8>), dim3(grid), dim3(256), geom.lds_bytes, s, d_params, d_tables, d_pos, in, in_stride,
                           (int64_t)n_in, wrap, (uint32_t)n_out, tiles, gain_off, static_cast<uint8_t*>(d_out), out_stride_bytes, u8_scale);
}

}  // namespace dabgpu
