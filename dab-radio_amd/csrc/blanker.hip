// blanker.hip -- the impulse blanker on the device (include/dabgpu.h, "Impulse blanker"): a greatest-of cell-averaging detector on block
// powers that zeroes bursts in a bank of independent streams.  Every arithmetic step is blanker_core.h's; this file is where the samples
// come from and go to.
//
// One 256-thread workgroup per (stream, tile of DABGPU_BLANKER_BLOCK = 1024 samples = 32 blocks = one mask word), tiles aligned to
// ABSOLUTE sample numbers (multiples of 1024), so a block, a mask word and the 16 bytes of a load belong to the same threads wherever
// the stream position stands; a call that starts at an odd position stores sample by sample.
// A thread owns two neighbouring samples (one 16-byte load where the input index is even), 16 lanes own a block: the pair's energies are
// added in the thread and the four further levels of blanker_core.h's tree are a butterfly across the 16 lanes (a float addition is
// commutative bit for bit, so every lane ends with the tree's value).  The tile's own 32 blocks take two such passes, whose samples stay
// in registers; the stream's reach either side (gap + window + guard blocks) takes ceil(reach / 16) passes each, whose samples are
// dropped.  The powers go to LDS; 32 + 2 guard threads form the window sums and flags there, and every thread ORs the flags around its
// block.  Then the kept samples, or zeros, are stored with one non-temporal 16-byte store per thread and pass.  A tile with nothing
// flagged is a copy; the halo is the only traffic above one, and it is its neighbours' core, so it comes from L2 as a rule.
// The stream's parameters are read through a pointer that is the same for the whole workgroup (scalar loads).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <new>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "blanker_core.h"
#include "channel_device.h"
#include "signal_bank.h"

namespace dabgpu {

constexpr int BLK_TILE = DABGPU_BLANKER_BLOCK;
constexpr int BLK_TILE_BLOCKS = BLK_TILE / BLK_LEN;                     // 32: the bits of a mask word
constexpr int BLK_PASS_BLOCKS = 256 * 2 / BLK_LEN;                      // 16 blocks per pass of the workgroup
static_assert(BLK_TILE_BLOCKS == 32 && BLK_TILE == 2 * 256 * 2, "a tile is one mask word and two passes of 256 threads x 2 samples");

// blocks [j0, j0 + 16) of the window, as far as they lie below j_end: the thread's two samples (zeros beyond j_end), the block's power to
// pw[].  Every lane of the workgroup runs the butterfly.
__device__ __forceinline__ void blk_pass(const ChWindow& W, int t, int j0, int j_end, float* pw, chf2& a, chf2& b) {
    const int j = j0 + (t >> 4);
    a = b = chf2{0.0f, 0.0f};
    if (j < j_end) ch_load2(W, j0 * BLK_LEN + 2 * t, a, b);
    float e = blk_energy(a) + blk_energy(b);
    e = e + __shfl_xor(e, 1);
    e = e + __shfl_xor(e, 2);
    e = e + __shfl_xor(e, 4);
    e = e + __shfl_xor(e, 8);
    if ((t & 15) == 0 && j < j_end) pw[j] = e * BLK_INV_LEN;
}

__global__ __launch_bounds__(256)
void blanker_kernel(const dabgpu_blanker_stream* __restrict__ params, const uint64_t* __restrict__ d_pos, const chf2* __restrict__ in,
                    size_t in_stride, int64_t n_in, uint32_t n_out, int tiles, uint8_t* __restrict__ out, size_t out_stride_bytes,
                    uint32_t* __restrict__ mask, size_t mask_stride, int bank_reach)
{
    extern __shared__ __attribute__((aligned(16))) float blk_lds[];
    const int t = threadIdx.x;
    const uint32_t s = blockIdx.x / (uint32_t)tiles, tile = blockIdx.x % (uint32_t)tiles;
    const dabgpu_blanker_stream& P = params[s];
    const uint64_t pos = *d_pos;
    const uint64_t T0 = (pos & ~(uint64_t)(BLK_TILE - 1)) + (uint64_t)tile * BLK_TILE;   // absolute number of the tile's first sample
    const uint64_t rel0 = T0 - pos;                                          // -1023 .. 0 (as unsigned) for tile 0
    const int lo = (tile == 0) ? (int)(pos & (uint64_t)(BLK_TILE - 1)) : 0;  // samples of this tile inside the call: tile-local [lo, hi)
    const int64_t left = (int64_t)n_out - (int64_t)rel0;
    uint32_t* word = mask ? mask + (size_t)s * mask_stride + tile : nullptr;
    if (left <= lo) {                                                        // a tile past the call's end: its word is written all the same
        if (word && t == 0) *word = 0u;
        return;
    }
    const int hi = left < BLK_TILE ? (int)left : BLK_TILE;
    const chf2* x = in + (size_t)s * in_stride;
    uint8_t* orow = out + (size_t)s * out_stride_bytes;
    const bool even = (pos & 1) == 0;
    const bool on = P.enabled != 0;
    const int r = on ? blk_reach(P) : 0, g = P.guard;                        // r <= bank_reach (the planner, _set_params)
    float* pw = blk_lds;                                                     // power of block (T0 >> 5) - r + j, j < 32 + 2 r
    int* fl = reinterpret_cast<int*>(blk_lds + BLK_TILE_BLOCKS + 2 * bank_reach);        // flag of block (T0 >> 5) - g + i, i < 32 + 2 g
    const int n_blocks = BLK_TILE_BLOCKS + 2 * r;
    const ChWindow W = ch_window(x, n_in, false, T0 - (uint64_t)P.start - (uint64_t)(r * BLK_LEN), n_blocks * BLK_LEN);

    chf2 y[2][2];
    blk_pass(W, t, r, n_blocks, pw, y[0][0], y[0][1]);
    blk_pass(W, t, r + BLK_PASS_BLOCKS, n_blocks, pw, y[1][0], y[1][1]);
    uint32_t bits = 0;
    if (on) {
        chf2 a, b;
        for (int j0 = 0; j0 < r; j0 += BLK_PASS_BLOCKS) blk_pass(W, t, j0, r, pw, a, b);
        for (int j0 = r + BLK_TILE_BLOCKS; j0 < n_blocks; j0 += BLK_PASS_BLOCKS) blk_pass(W, t, j0, n_blocks, pw, a, b);
        __syncthreads();
        if (t < BLK_TILE_BLOCKS + 2 * g) {
            const int c = r - g + t;
            fl[t] = blk_flag(P, [&](int j) { return pw[c + j]; }) ? 1 : 0;
        }
        __syncthreads();
        bool mine = false;                                                   // of block t of the tile, where its first sample is in the call
        if (t < BLK_TILE_BLOCKS) mine = blk_blank(P, [&](int j) { return fl[t + g + j] != 0; }) && BLK_LEN * t >= lo && BLK_LEN * t < hi;
        bits = (uint32_t)__ballot(mine);                                     // (wave 0 holds threads 0 .. 63)
    }
    if (word && t == 0) *word = bits;

#pragma unroll
    for (int c = 0; c < 2; c++) {
        const int n0 = 2 * 256 * c + 2 * t;                                  // tile-local number of the thread's first sample
        if (n0 + 2 <= lo || n0 >= hi) continue;
        if (on && blk_blank(P, [&](int j) { return fl[(n0 >> BLK_SHIFT) + g + j] != 0; })) y[c][0] = y[c][1] = chf2{0.0f, 0.0f};
        const size_t o = (size_t)(rel0 + (uint64_t)n0);                      // sample of n0 in the call (meaningful where n0 >= lo)
        if (even && n0 >= lo && n0 + 2 <= hi) {
            __builtin_nontemporal_store(ch_f4{y[c][0].re, y[c][0].im, y[c][1].re, y[c][1].im}, reinterpret_cast<ch_f4*>(orow + 8 * o));
        } else {
#pragma unroll
            for (int h = 0; h < 2; h++)
                if (n0 + h >= lo && n0 + h < hi) *reinterpret_cast<ch_f2v*>(orow + 8 * (o + h)) = ch_f2v{y[c][h].re, y[c][h].im};
        }
    }
}

}  // namespace dabgpu

using namespace dabgpu;

struct dabgpu_blanker_bank : SignalBank {         // d_mem: position (16 bytes) | parameters
    size_t n = 0;
    dabgpu_blanker_geometry geom = {};
    dabgpu_blanker_stream* d_params = nullptr;
    DeviceBuffer<uint32_t> d_mask;                // host form: the mask words (grow only)
};

static int blk_launch(dabgpu_blanker_bank* b, const float* d_in, size_t in_stride, size_t n_in, size_t n_out, void* d_out, size_t out_stride_bytes,
                      uint32_t* d_mask, size_t mask_stride, hipStream_t s) {
    const int tiles = (int)dabgpu_blanker_mask_words(n_out);
    const unsigned grid = (unsigned)((size_t)tiles * b->n);
    hipLaunchKernelGGL(blanker_kernel, dim3(grid), dim3(256), b->geom.lds_bytes, s, b->d_params, b->d_pos, reinterpret_cast<const chf2*>(d_in), in_stride,
                       (int64_t)n_in, (uint32_t)n_out, tiles, static_cast<uint8_t*>(d_out), out_stride_bytes, d_mask, mask_stride, (int)b->geom.reach_blocks);
    sb_enqueue_advance(b->d_pos, n_out, s);
    return dabgpu_check_hip(hipGetLastError(), "blanker_kernel launch");
}

extern "C" {

int dabgpu_blanker_bank_create(dabgpu_ctx* c, size_t n_streams, const dabgpu_blanker_stream* h_params, dabgpu_blanker_bank** out) {
    if (!c || !out) { dabgpu_set_error("blanker_bank_create: null context / result"); return DABGPU_ERR_INVALID_ARG; }
    *out = nullptr;
    dabgpu_blanker_geometry g;
    int st = dabgpu_host_blanker_plan("blanker_bank_create", h_params, n_streams, &g);
    if (st) return st;
    dabgpu_blanker_bank* b = new (std::nothrow) dabgpu_blanker_bank;
    if (!b) return DABGPU_ERR_HIP;
    b->ctx = c; b->n = n_streams; b->geom = g;
    auto fail = [&](int status) { dabgpu_blanker_bank_destroy(b); return status; };
    if ((st = dabgpu_bind_device(c))) return fail(st);
    uint8_t* payload;
    if ((st = sb_alloc(b, n_streams * sizeof(dabgpu_blanker_stream), "blanker", &payload))) return fail(st);
    b->d_params = reinterpret_cast<dabgpu_blanker_stream*>(payload);
    if ((st = dabgpu_stage_h2d(c, b->d_params, h_params, n_streams * sizeof(dabgpu_blanker_stream), c->stream))) return fail(st);
    if ((st = dabgpu_check_hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize(blanker_bank_create)"))) return fail(st);
    *out = b;
    return DABGPU_OK;
}

void dabgpu_blanker_bank_destroy(dabgpu_blanker_bank* b) {
    if (!dabgpu_destroy_begin(b, b ? b->ctx : nullptr)) return;
    delete b;
}

int dabgpu_blanker_bank_set_params(dabgpu_blanker_bank* b, const dabgpu_blanker_stream* h_params, void* stream) {
    if (!b) { dabgpu_set_error("blanker_bank_set_params: null bank"); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_blanker_geometry g;
    int st = dabgpu_host_blanker_plan("blanker_bank_set_params", h_params, b->n, &g);
    if (st || (st = dabgpu_host_blanker_fits(b->geom, g))) return st;        // (b->geom stays: captured calls launch with it)
    DABGPU_BIND(b->ctx);
    return dabgpu_stage_h2d(b->ctx, b->d_params, h_params, b->n * sizeof(dabgpu_blanker_stream), (hipStream_t)stream);
}

int dabgpu_blanker_bank_seek(dabgpu_blanker_bank* b, uint64_t position, void* stream) {
    return sb_seek(b, "blanker_bank_seek", position, (uint64_t)DABGPU_BLANKER_MAX_POSITION, "2^62", stream);
}

int dabgpu_blanker_bank_apply(dabgpu_blanker_bank* b, const float* d_in, size_t in_stride_samples, size_t n_in, size_t n_out, void* d_out,
                              size_t out_stride_bytes, uint32_t* d_mask, size_t mask_stride_words, void* stream) {
    if (!b) { dabgpu_set_error("blanker_bank_apply: null bank"); return DABGPU_ERR_INVALID_ARG; }
    const int st = dabgpu_host_blanker_check_apply("blanker_bank_apply", b->n, d_in, in_stride_samples, n_in, n_out, d_out, &out_stride_bytes, d_mask,
                                                   &mask_stride_words);
    if (st) return st;
    DABGPU_BIND(b->ctx);
    if (n_out == 0 && !d_mask) return DABGPU_OK;
    return blk_launch(b, d_in, in_stride_samples, n_in, n_out, d_out, out_stride_bytes, d_mask, mask_stride_words, (hipStream_t)stream);
}

int dabgpu_blanker_bank_apply_host_sync(dabgpu_blanker_bank* b, const float* h_in, size_t in_stride_samples, size_t n_in, size_t n_out, void* h_out,
                                        size_t out_stride_bytes, uint32_t* h_mask, size_t mask_stride_words) {
    if (!b) { dabgpu_set_error("blanker_bank_apply_host_sync: null bank"); return DABGPU_ERR_INVALID_ARG; }
    int st = dabgpu_host_blanker_check_apply("blanker_bank_apply_host_sync", b->n, h_in, in_stride_samples, n_in, n_out, h_out, &out_stride_bytes, h_mask,
                                             &mask_stride_words, false);
    if (st) return st;
    const size_t words = dabgpu_blanker_mask_words(n_out);
    if (n_out == 0) {                                                        // nothing to launch: the words are written all the same
        for (size_t i = 0; h_mask && i < b->n; i++) h_mask[i * mask_stride_words] = h_mask[i * mask_stride_words + 1] = 0u;
        return DABGPU_OK;
    }
    return sb_host_round_trip(b, b->n, b->n, false, h_in, in_stride_samples, n_in, n_out, h_out, DABGPU_IQ_RAW_F32L, out_stride_bytes,
                              [&](const float* d_in, size_t d_in_stride, void* d_out, size_t d_out_stride, hipStream_t s) {
                                  int st2;
                                  if (h_mask && b->d_mask.needs(b->n * words)) {
                                      if (b->d_mask && (st2 = dabgpu_check_hip(hipDeviceSynchronize(), "hipDeviceSynchronize(blanker mask)"))) return st2;
                                      if ((st2 = b->d_mask.regrow(b->n * words, "hipMalloc(blanker mask)"))) return st2;
                                  }
                                  uint32_t* d_mask = h_mask ? b->d_mask.get() : nullptr;
                                  if ((st2 = blk_launch(b, d_in, d_in_stride, n_in, n_out, d_out, d_out_stride, d_mask, words, s))) return st2;
                                  if (!h_mask) return (int)DABGPU_OK;
                                  return dabgpu_check_hip(hipMemcpy2DAsync(h_mask, mask_stride_words * 4, d_mask, words * 4, words * 4, b->n,
                                                                           hipMemcpyDeviceToHost, s), "hipMemcpy2DAsync(blanker mask)");
                              });
}

}  // extern "C"
