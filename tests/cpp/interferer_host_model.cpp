// The interferer on the CPU: dab-radio_amd/csrc/interferer_core.h -- the functions the kernel is made of -- compiled with g++ into a shared
// object (tests/interferer_model.py, build_host_model), with plain loops where the kernel has its grid, its LDS staging and its stepped gate.
// tests/test_interferer_model.py holds it against the independent numpy model, tests/test_gpu_interferer.py holds the device against it
// bit for bit.
#include <stdint.h>
#include <string.h>

#include "interferer_core.h"

using namespace dabgpu;

extern "C" {

void itm_philox(uint32_t k0, uint32_t k1, const uint32_t* ctr, uint32_t* out) { ch_philox4x32_10(k0, k1, ctr[0], ctr[1], ctr[2], ctr[3], out); }
void itm_noise_words(uint64_t seed, uint32_t s, uint32_t k, uint64_t pair, uint32_t* out) { itf_noise_words(seed, s, k, pair, out); }

// g[n0 .. n0 + count) of source k of stream s (n wraps as an unsigned 64-bit number)
void itm_gauss(uint64_t seed, uint32_t s, uint32_t k, uint64_t n0, uint64_t count, float* out) {
    for (uint64_t i = 0; i < count; i++) {
        const chf2 g = itf_gauss(seed, s, k, n0 + i);
        out[2 * i] = g.re; out[2 * i + 1] = g.im;
    }
}

uint64_t itm_gate_rem(uint64_t m, int64_t offset, uint64_t period) { return itf_gate_rem(m, offset, period); }
uint64_t itm_gate_step(uint64_t rem0, uint32_t k, uint64_t period) { return itf_gate_step(rem0, k, period); }

// dabgpu_interferer_bank_apply at stream position `pos`; in may be null
void itm_apply(const dabgpu_interferer_stream* params, uint32_t n_streams, const dabgpu_interferer_shape* shapes, const float* in, size_t in_stride,
               uint64_t pos, uint64_t n_out, void* out, int out_format, size_t out_stride_bytes, float scale) {
    for (uint32_t s = 0; s < n_streams; s++) {
        const chf2* x = in ? reinterpret_cast<const chf2*>(in) + (size_t)s * in_stride : nullptr;
        uint8_t* row = static_cast<uint8_t*>(out) + (size_t)s * out_stride_bytes;
        for (uint64_t i = 0; i < n_out; i++) {
            const chf2 y = itf_sample(params[s], shapes, s, pos + i, x ? x[i] : chf2{0.0f, 0.0f});
            if (out_format == DABGPU_IQ_RAW_F32L) memcpy(row + 8 * i, &y, 8);
            else { row[2 * i] = (uint8_t)ch_u8(y.re, scale); row[2 * i + 1] = (uint8_t)ch_u8(y.im, scale); }
        }
    }
}

}  // extern "C"
