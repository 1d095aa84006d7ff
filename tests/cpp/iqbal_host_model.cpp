// The IQ balance bank on the CPU: dab-radio_amd/csrc/iqbal_core.h -- the functions the kernels are made of -- compiled with g++ into a
// shared object (tests/iqbal_model.py, build_host_model), with plain loops where the kernels have their grid, their lane butterfly and their
// LDS.  tests/test_iqbal_model.py holds it against the independent numpy model, tests/test_gpu_iqbal.py holds the device against it bit for
// bit.
#include <stdint.h>
#include <string.h>
#include <vector>

#include "dabgpu.h"
#include "iqbal_core.h"

using namespace dabgpu;

extern "C" {

// z = a y + b conj(y) + c over n samples; k = a_re, a_im, b_re, b_im, c_re, c_im
void iqm_map(const float* k, const float* in, size_t n, float* out) {
    const iqb_coef K{chf2{k[0], k[1]}, chf2{k[2], k[3]}, chf2{k[4], k[5]}};
    for (size_t i = 0; i < n; i++) {
        const chf2 z = iqb_map(K, chf2{in[2 * i], in[2 * i + 1]});
        out[2 * i] = z.re; out[2 * i + 1] = z.im;
    }
}

// the five sums of n_tiles tiles of 1024 samples
void iqm_moments(const float* in, size_t n_tiles, float* out) {
    for (size_t j = 0; j < n_tiles; j++) {
        const iqb_moments m = iqb_tile_moments(reinterpret_cast<const chf2*>(in) + j * IQB_TILE);
        memcpy(out + 5 * j, m.m, sizeof(m.m));
    }
}

// n_tiles tiles (5 floats each) folded into the record's state in order, then the solve (n_tiles may be 0)
void iqm_fold_and_solve(const dabgpu_iqbal_stream* P, dabgpu_iqbal_record* R, const float* moments, int n_tiles) {
    iqb_fold_and_solve(*P, *R, n_tiles, [&](int j) { return moments + 5 * j; });
}

void iqm_reset(dabgpu_iqbal_record* R, size_t n) {
    for (size_t s = 0; s < n; s++) iqb_record_reset(R[s]);
}

// dabgpu_iqbal_bank_apply at stream position `pos` on the records `rec` (updated in place).  moments: null, or n / 1024 x 5 floats per
// stream.  Returns the samples the position advances by: n, or 0 where the device refuses (MEASURE off a tile edge: nothing is written).
uint64_t iqm_apply(const dabgpu_iqbal_stream* params, dabgpu_iqbal_record* rec, uint32_t n_streams, const float* in, size_t in_stride, uint64_t pos,
                   uint64_t n, void* out, int out_format, size_t out_stride_bytes, float scale, uint32_t flags, float* moments) {
    const bool measure = (flags & DABGPU_IQBAL_MEASURE) != 0, apply = (flags & DABGPU_IQBAL_APPLY) != 0;
    if (measure && (pos & (IQB_TILE - 1))) {
        for (uint32_t s = 0; s < n_streams; s++) rec[s].calls_refused++;
        return 0;
    }
    const int tiles = (int)(n / IQB_TILE);
    for (uint32_t s = 0; s < n_streams; s++) {
        const dabgpu_iqbal_stream& P = params[s];
        const chf2* x = reinterpret_cast<const chf2*>(in) + (size_t)s * in_stride;
        if (apply) {                                                         // with the coefficients as they stand before the fold
            const iqb_coef K = iqb_stream_coef(P, rec[s]);
            uint8_t* row = static_cast<uint8_t*>(out) + (size_t)s * out_stride_bytes;
            for (uint64_t i = 0; i < n; i++) {
                const chf2 z = P.mode == DABGPU_IQBAL_OFF ? x[i] : iqb_map(K, x[i]);
                if (out_format == DABGPU_IQ_RAW_F32L) memcpy(row + 8 * i, &z, 8);
                else { row[2 * i] = (uint8_t)ch_u8(z.re, scale); row[2 * i + 1] = (uint8_t)ch_u8(z.im, scale); }
            }
        }
        if (measure) {
            std::vector<float> m((size_t)tiles * 5);
            iqm_moments(reinterpret_cast<const float*>(x), (size_t)tiles, m.data());
            if (moments) memcpy(moments + (size_t)s * tiles * 5, m.data(), m.size() * 4);
            if (P.mode == DABGPU_IQBAL_TRACK) iqm_fold_and_solve(&P, &rec[s], m.data(), tiles);
        }
    }
    return n;
}

}  // extern "C"
