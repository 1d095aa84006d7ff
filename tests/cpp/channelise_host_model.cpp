// The channeliser on the CPU: dab-radio_amd/csrc/channelise_core.h -- the functions the kernels are made of -- compiled with g++ into a
// shared object together with the planner (dabgpu_host_logic.cpp: dabgpu_channeliser_design makes the table), with plain loops where the
// kernels have their grid and their LDS staging (tests/channelise_model.py, build_host_model).  tests/test_channelise_model.py holds it
// against the independent numpy model, tests/test_gpu_channelise.py holds the device against it bit for bit.
#include <stdint.h>
#include <string.h>
#include <vector>

#include "channelise_core.h"

using namespace dabgpu;

extern "C" {

// dabgpu_channeliser_bank_split at position `pos`: in [n_streams] rows in_stride apart (0: shared), out [n_channels] rows of n_out complex float.
// cs_split_sample per output, except that v_c[n] = cs_mix_down(x[n], n) of the absolute indices the call reads is computed once per channel
// (as the kernel rotates its window once) instead of once per tap: the same function of the same (sample, n), then the same chain.
void csm_split(const dabgpu_channeliser_channel* ch, uint32_t n_channels, int decim, const float* table, const float* in, size_t in_stride, int64_t n_in,
               int wrap, uint64_t pos, int64_t start, uint64_t n_out, float* out, size_t out_stride_bytes) {
    if (n_out == 0) return;
    const int K = cs_taps(decim);
    const int64_t first = cs_split_first(decim, pos, start);
    const size_t span = (size_t)(n_out - 1) * (size_t)decim + (size_t)K;
    std::vector<chf2> v(span);
    for (uint32_t c = 0; c < n_channels; c++) {
        const chf2* x = reinterpret_cast<const chf2*>(in) + (size_t)ch[c].stream * in_stride;
        uint8_t* row = reinterpret_cast<uint8_t*>(out) + (size_t)c * out_stride_bytes;
        for (size_t i = 0; i < span; i++) v[i] = cs_mix_down(ch[c], cs_fetch(x, n_in, wrap != 0, first + (int64_t)i), (uint64_t)(first + (int64_t)i));
        for (uint64_t m = 0; m < n_out; m++) {
            chf2 acc = cs_chain_start();
            for (int j = 0; j < K; j++) acc = cs_tap(acc, table[j], v[(size_t)m * (size_t)decim + (size_t)j]);
            const chf2 y = cs_scale(ch[c].gain, acc);
            memcpy(row + 8 * m, &y, 8);
        }
    }
}

// one output through cs_split_sample itself (tests/test_channelise_model.py holds csm_split against it)
void csm_split_sample(const dabgpu_channeliser_channel* ch, int decim, const float* table, const float* in, int64_t n_in, int wrap, uint64_t m, int64_t start,
                      float* out) {
    const chf2 y = cs_split_sample(*ch, decim, table, reinterpret_cast<const chf2*>(in), n_in, wrap != 0, m, start);
    memcpy(out, &y, 8);
}

// dabgpu_channeliser_bank_combine at position `pos`: in [n_channels] rows, out [n_streams] rows of n_out samples
void csm_combine(const dabgpu_channeliser_channel* ch, uint32_t n_channels, uint32_t n_streams, int decim, const float* table, const float* in,
                 size_t in_stride, int64_t n_in, int wrap, uint64_t pos, int64_t start, uint64_t n_out, void* out, int out_format, size_t out_stride_bytes,
                 float scale) {
    uint32_t c0 = 0;
    for (uint32_t s = 0; s < n_streams; s++) {
        uint32_t c1 = c0;
        while (c1 < n_channels && ch[c1].stream == s) c1++;
        uint8_t* row = static_cast<uint8_t*>(out) + (size_t)s * out_stride_bytes;
        for (uint64_t i = 0; i < n_out; i++) {
            const chf2 y = cs_combine_sample(ch, c0, c1, decim, table, reinterpret_cast<const chf2*>(in), in_stride, n_in, wrap != 0, (int64_t)(pos + i), start);
            if (out_format == DABGPU_IQ_RAW_F32L) memcpy(row + 8 * i, &y, 8);
            else { row[2 * i] = (uint8_t)ch_u8(y.re, scale); row[2 * i + 1] = (uint8_t)ch_u8(y.im, scale); }
        }
        c0 = c1;
    }
}

}  // extern "C"
