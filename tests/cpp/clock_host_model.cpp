// clock_host_model.cpp -- csrc/clock_core.h compiled for the host (tests/clock_model.py builds it with -ffp-contract=off, together with
// the host half of the library): the folded sum, the angle polynomial, the update and the de-rotation of one frame's DQPSK products, in
// the statements the kernels run.
#include <stddef.h>
#include <stdint.h>

#include "clock_core.h"

using namespace dabgpu;

extern "C" {

int64_t clkm_max_slope(void) { return CLK_MAX_SLOPE; }
int clkm_lag(void) { return CLK_LAG; }
int clkm_pairs(void) { return CLK_PAIRS; }
float clkm_atan_cycles(float t) { return clk_atan_cycles(t); }
void clkm_atan_cycles_many(const float* t, float* out, size_t n) { for (size_t i = 0; i < n; i++) out[i] = clk_atan_cycles(t[i]); }
void clkm_fold(const float* p, float* out) { const chf2 f = clk_fold(chf2{p[0], p[1]}); out[0] = f.re; out[1] = f.im; }

// steps 1 to 4: dq [75][1536] complex float -> A (re, im) and the number of dropped pairs
void clkm_sum(const float* dq, int64_t slope_in, float* corr, uint32_t* dropped) { clk_frame_sum(dq, slope_in, &corr[0], &corr[1], dropped); }
// one frame as the device writes it; dq is not read when sync_ok is 0
int clkm_estimate(const float* dq, int sync_ok, int64_t slope_in, float gain, int64_t* slope_out, int64_t* residual, float* corr) {
    const clk_update u = clk_estimate_frame(dq, sync_ok != 0, slope_in, gain, corr);
    if (slope_out) *slope_out = u.slope;
    if (residual) *residual = u.residual;
    return u.valid ? 1 : 0;
}
void clkm_derotate(const float* in, float* out, int64_t slope) { clk_derotate_frame(in, out, slope); }

}  // extern "C"
