// Host model of the channel-state weighted soft bits: the functions of dab-radio_amd/csrc/softbit_csi_core.h -- the same lines the
// demodulation kernel compiles -- behind a C interface for tests/softbit_model.py.  Built by the tests with g++ -ffp-contract=off.
#include <stddef.h>
#include <stdint.h>

#include "softbit_csi_core.h"

extern "C" {

float sbm_frame_power(const float* prs_useful) { return dabgpu::sb_frame_power(prs_useful); }
float sbm_scale(float level, float P) { return dabgpu::sb_scale(level, P); }
int sbm_level_ok(float level) { return dabgpu::sb_level_ok(level) ? 1 : 0; }
// d: n complex products; first[i] from +re d[i], second[i] from -im d[i]
void sbm_soft_bits(const float* d, size_t n, float k, int8_t* first, int8_t* second) {
    for (size_t i = 0; i < n; i++) {
        first[i] = (int8_t)dabgpu::sb_soft_bit(d[2 * i], k);
        second[i] = (int8_t)dabgpu::sb_soft_bit(-d[2 * i + 1], k);
    }
}

}  // extern "C"
