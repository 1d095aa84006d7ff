// The impulse blanker on the CPU: dab-radio_amd/csrc/blanker_core.h -- the functions the kernel is made of -- compiled with g++ into a
// shared object (tests/blanker_model.py, build_host_model), with plain loops where the kernel has its grid, its lane butterfly and its LDS.
// tests/test_blanker_model.py holds it against the independent numpy model, tests/test_gpu_blanker.py holds the device against it bit for
// bit.
#include <stdint.h>
#include <string.h>
#include <vector>

#include "dabgpu.h"
#include "blanker_core.h"

using namespace dabgpu;

extern "C" {

// p of blocks [b0, b0 + count) of one stream
void blm_powers(const float* in, int64_t n_in, int64_t start, int64_t b0, int64_t count, float* out) {
    for (int64_t j = 0; j < count; j++) out[j] = blk_power(reinterpret_cast<const chf2*>(in), n_in, start, b0 + j);
}

// flag and blank of blocks [b0, b0 + count) of one stream (either may be null), one byte each
void blm_decide(const dabgpu_blanker_stream* P, const float* in, int64_t n_in, int64_t b0, int64_t count, uint8_t* flag, uint8_t* blank) {
    const int r = blk_reach(*P), g = P->guard;
    std::vector<float> p((size_t)(count + 2 * r));                           // block b0 - r + j
    blm_powers(in, n_in, P->start, b0 - r, count + 2 * r, p.data());
    std::vector<uint8_t> f((size_t)(count + 2 * g));                         // block b0 - g + i
    for (int64_t i = 0; i < count + 2 * g; i++) f[i] = blk_flag(*P, [&](int j) { return p[i + (r - g) + j]; }) ? 1 : 0;
    for (int64_t i = 0; i < count; i++) {
        if (flag) flag[i] = f[i + g];
        if (blank) blank[i] = blk_blank(*P, [&](int j) { return f[i + g + j] != 0; }) ? 1 : 0;
    }
}

// dabgpu_blanker_bank_apply at stream position `pos`; mask may be null, mask_stride in words (>= n_out / 1024 + 2)
void blm_apply(const dabgpu_blanker_stream* params, uint32_t n_streams, const float* in, size_t in_stride, int64_t n_in, uint64_t pos, uint64_t n_out,
               void* out, size_t out_stride_bytes, uint32_t* mask, size_t mask_stride) {
    const uint64_t words = n_out / DABGPU_BLANKER_BLOCK + 2;
    for (uint32_t s = 0; s < n_streams; s++) {
        const dabgpu_blanker_stream& P = params[s];
        const chf2* x = reinterpret_cast<const chf2*>(in) + (size_t)s * in_stride;
        uint8_t* row = static_cast<uint8_t*>(out) + (size_t)s * out_stride_bytes;
        uint32_t* w = mask ? mask + (size_t)s * mask_stride : nullptr;
        for (uint64_t j = 0; w && j < words; j++) w[j] = 0u;
        if (n_out == 0) continue;
        const int64_t b0 = (int64_t)(pos >> BLK_SHIFT), b1 = (int64_t)((pos + n_out - 1) >> BLK_SHIFT);
        std::vector<uint8_t> blank((size_t)(b1 - b0 + 1), 0);
        if (P.enabled) blm_decide(&P, reinterpret_cast<const float*>(x), n_in, b0, b1 - b0 + 1, nullptr, blank.data());
        for (uint64_t i = 0; i < n_out; i++) {
            const int64_t m = (int64_t)(pos + i);
            chf2 y = blk_input(x, n_in, P.start, m);
            if (blank[(size_t)((m >> BLK_SHIFT) - b0)]) y = chf2{0.0f, 0.0f};
            memcpy(row + 8 * i, &y, 8);
        }
        for (int64_t b = b0; w && b <= b1; b++) {
            const uint64_t first = (uint64_t)b << BLK_SHIFT;                 // the bit belongs to the call that holds the block's first sample
            if (!blank[(size_t)(b - b0)] || first < pos || first >= pos + n_out) continue;
            const uint64_t tile = (first >> 10) - (pos >> 10);
            w[tile] |= 1u << (uint32_t)(b & 31);
        }
    }
}

}  // extern "C"
