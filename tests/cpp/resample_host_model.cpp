// The resampler on the CPU: dab-radio_amd/csrc/resample_core.h -- the functions the kernel is made of -- compiled with g++ into a shared
// object together with the planner (dabgpu_host_logic.cpp: dabgpu_resample_design makes the table), with plain loops where the kernel has
// its grid and its LDS staging (tests/resample_model.py, build_host_model).  tests/test_resample_model.py holds it against the independent
// numpy model, tests/test_gpu_resample.py holds the device against it bit for bit.
#include <stdint.h>
#include <string.h>

#include "resample_core.h"

using namespace dabgpu;

extern "C" {

// T(m): the index word, its sign and the fraction of rs_time, the row and the weight taken from the fraction
void rsm_time(const dabgpu_resample_stream* P, uint64_t m, uint64_t* n, int32_t* neg, uint64_t* frac, int32_t* row, float* weight) {
    const RsTime t = rs_time(*P, m);
    *n = t.n; *neg = t.neg ? 1 : 0; *frac = t.frac; *row = rs_row(t.frac); *weight = rs_weight(t.frac);
}

int64_t rsm_mod(uint64_t n, int neg, int64_t n_in) { return rs_mod(RsIndex{n, neg != 0}, n_in); }
uint32_t rsm_rows_needed(const dabgpu_resample_stream* P) { return rs_rows_needed(*P); }

// dabgpu_resample_bank_apply at stream position `pos`
void rsm_apply(const dabgpu_resample_stream* params, uint32_t n_streams, const float* table, const float* in, size_t in_stride, int64_t n_in, int wrap,
               uint64_t pos, uint64_t n_out, void* out, int out_format, size_t out_stride_bytes, float scale) {
    for (uint32_t s = 0; s < n_streams; s++) {
        const chf2* x = reinterpret_cast<const chf2*>(in) + (size_t)s * in_stride;
        uint8_t* row = static_cast<uint8_t*>(out) + (size_t)s * out_stride_bytes;
        for (uint64_t i = 0; i < n_out; i++) {
            const chf2 y = rs_sample(params[s], table, x, n_in, wrap != 0, pos + i);
            if (out_format == DABGPU_IQ_RAW_F32L) memcpy(row + 8 * i, &y, 8);
            else { row[2 * i] = (uint8_t)ch_u8(y.re, scale); row[2 * i + 1] = (uint8_t)ch_u8(y.im, scale); }
        }
    }
}

}  // extern "C"
