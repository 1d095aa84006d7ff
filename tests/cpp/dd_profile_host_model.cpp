// dd_profile_host_model.cpp -- csrc/dd_profile_core.h compiled for the host (tests/dd_profile_model.py builds it with
// -ffp-contract=off, together with the host half of the library): the carrier sums, amplitude and noise of one frame's DQPSK products and
// the whole frame, in the statements the kernel runs.
#include <stddef.h>
#include <stdint.h>

#include "dd_profile_core.h"

using namespace dabgpu;

extern "C" {

float ddm_k1(void) { return DDP_K1; }
float ddm_k75(void) { return DDP_K75; }

// dq: [75][1536] complex float -> Q [1536], A [1536]
void ddm_carriers(const float* dq, float* Q, float* A) { ddp_frame_carriers(dq, Q, A); }

// one frame as the device writes it; dq is not read when sync_ok is 0
int ddm_frame(const float* dq, int sync_ok, const uint32_t* exclude, const float* profile_in, float alpha, float* profile_out, float* band_weight,
              float* mean_noise, float* carrier_noise, float* carrier_amplitude) {
    return ddp_frame(dq, sync_ok != 0, exclude, profile_in, alpha, profile_out, band_weight, mean_noise, carrier_noise, carrier_amplitude) ? 1 : 0;
}

}  // extern "C"
