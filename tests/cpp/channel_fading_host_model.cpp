// The fading channel on the CPU: dab-radio_amd/csrc/channel_core.h -- the functions the fading kernel is made of -- compiled with g++
// into a shared object (tests/channel_fading_model.py, build_host_model), with plain loops where the kernel has its grid, its LDS and
// its 16-lane groups.  tests/test_channel_fading_model.py holds it against the independent numpy model, tests/test_gpu_channel_fading.py
// holds the device against it bit for bit.
#include <stdint.h>
#include <string.h>

#include "channel_core.h"

using namespace dabgpu;

extern "C" {

// G_j of one tap at grid points j0 .. j0 + n - 1
void chfm_grid_gain(const dabgpu_channel_fading_stream* row, int tap, uint64_t j0, uint64_t n, float* out) {
    for (uint64_t i = 0; i < n; i++) {
        const chf2 g = ch_fading_grid_gain(row->tap[tap], j0 + i);
        out[2 * i] = g.re; out[2 * i + 1] = g.im;
    }
}

// dabgpu_channel_bank_apply of a fading bank at stream position `pos` (the grid gains of a tap are kept while m stays between two points)
void chfm_apply(const dabgpu_channel_stream* params, const dabgpu_channel_fading_stream* tables, uint32_t n_streams, const float* in, size_t in_stride,
                int64_t n_in, int wrap, uint64_t pos, uint64_t n_out, void* out, int out_format, size_t out_stride_bytes, float scale) {
    for (uint32_t s = 0; s < n_streams; s++) {
        const dabgpu_channel_stream& P = params[s];
        const dabgpu_channel_fading_stream& F = tables[s];
        const uint32_t mask = ch_fading_mask(F, P.n_taps);
        const chf2* x = reinterpret_cast<const chf2*>(in) + (size_t)s * in_stride;
        uint8_t* row = static_cast<uint8_t*>(out) + (size_t)s * out_stride_bytes;
        chf2 g0[DABGPU_CHANNEL_MAX_TAPS], g1[DABGPU_CHANNEL_MAX_TAPS];
        uint64_t held = ~(uint64_t)0;
        for (uint64_t i = 0; i < n_out; i++) {
            const uint64_t m = pos + i, j = m >> CH_FADE_GRID_SHIFT;
            if (i == 0 || j != held) {
                for (int k = 0; k < P.n_taps; k++)
                    if ((mask >> k) & 1u) { g0[k] = ch_fading_grid_gain(F.tap[k], j); g1[k] = ch_fading_grid_gain(F.tap[k], j + 1); }
                held = j;
            }
            uint32_t w[4] = {0, 0, 0, 0};
            if (P.noise_sigma != 0.0f) ch_noise_words(P.seed, s, m >> 1, w);
            const chf2 z = ch_paths_fading(P, mask, [&](int k) { return ch_fading_interp(g0[k], g1[k], m); }, [&](int k) {
                const int64_t idx = ch_src_index(m, P.start, P.tap_delay[k], n_in, wrap != 0);
                return idx < 0 ? chf2{0.0f, 0.0f} : x[idx];
            });
            const chf2 y = ch_finish(P, m, z, w);
            if (out_format == DABGPU_IQ_RAW_F32L) memcpy(row + 8 * i, &y, 8);
            else { row[2 * i] = (uint8_t)ch_u8(y.re, scale); row[2 * i + 1] = (uint8_t)ch_u8(y.im, scale); }
        }
    }
}

}  // extern "C"
