// channel_device.h -- what the channel kernels (channel.hip, channel_fading.hip) share on the device: the tile constants and the loads of
// a tile's input window with wrap and zero-fill resolved.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dabgpu.h"
#include "channel_core.h"

namespace dabgpu {

constexpr int CH_BLK = DABGPU_CHANNEL_BLOCK;
typedef float ch_f4 __attribute__((ext_vector_type(4)));
typedef float ch_f2v __attribute__((ext_vector_type(2)));

// where a tile's input comes from: x[origin + off], off < span.  wrap: origin is already reduced into [0, n_in); otherwise it is the
// plain index, clamped far enough outside the input that origin + off cannot overflow
struct ChWindow { const chf2* x; int64_t n_in, origin; int span; bool wrap; };

__device__ __forceinline__ chf2 ch_ld(const chf2* p) { const ch_f2v v = *reinterpret_cast<const ch_f2v*>(p); return chf2{v.x, v.y}; }

// samples off and off + 1 of the window
__device__ __forceinline__ void ch_load2(const ChWindow& W, int off, chf2& a, chf2& b) {
    int64_t j = W.origin + off;
    const chf2 zero = chf2{0.0f, 0.0f};
    if (W.wrap) {
        if (j >= W.n_in) j = (W.span <= W.n_in) ? j - W.n_in : j % W.n_in;
        const int64_t j1 = (j + 1 == W.n_in) ? 0 : j + 1;
        if (!(j & 1) && j1 == j + 1) {
            const ch_f4 v = *reinterpret_cast<const ch_f4*>(W.x + j);
            a = chf2{v.x, v.y}; b = chf2{v.z, v.w};
        } else { a = ch_ld(W.x + j); b = ch_ld(W.x + j1); }
    } else {
        if (j >= 0 && j + 1 < W.n_in && !(j & 1)) {
            const ch_f4 v = *reinterpret_cast<const ch_f4*>(W.x + j);
            a = chf2{v.x, v.y}; b = chf2{v.z, v.w};
        } else {
            a = (j >= 0 && j < W.n_in) ? ch_ld(W.x + j) : zero;
            b = (j + 1 >= 0 && j + 1 < W.n_in) ? ch_ld(W.x + j + 1) : zero;
        }
    }
}

__device__ __forceinline__ ChWindow ch_window(const chf2* x, int64_t n_in, bool wrap, uint64_t first, int span) {
    ChWindow W;
    W.x = x; W.n_in = n_in; W.wrap = wrap; W.span = span;
    int64_t o = (int64_t)first;
    if (wrap) { o %= n_in; if (o < 0) o += n_in; }
    else o = o < -((int64_t)1 << 41) ? -((int64_t)1 << 41) : (o > ((int64_t)1 << 41) ? ((int64_t)1 << 41) : o);
    W.origin = o;
    return W;
}

}  // namespace dabgpu
