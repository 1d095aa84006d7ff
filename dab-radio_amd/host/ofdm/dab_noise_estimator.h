// ofdm/dab_noise_estimator.h -- the noise estimate of one mode I frame (include/dabgpu.h, "Noise estimate"): the frame's NULL symbol and
// phase reference symbol become a calibrated noise power, the frame's signal power and the maximal-ratio weight 1 / noise power, which is
// what DAB_Diversity_Combiner::Combine takes as a branch's weight.  The reference has no such stage; the class follows the conventions of
// the other added classes: spans in, false for wrong sizes, exceptions for device failures.  Stateless: smoothing over frames is the caller's.
#pragma once
#include <complex>

#include "dabgpu.h"
#include "utility/span.h"

struct dabgpu_ctx;

class DAB_Noise_Estimator {
public:
    static constexpr size_t NB_SAMPLES = 2656 + 2552;       // NULL period + phase reference symbol
    DAB_Noise_Estimator();
    // null_and_prs: at least NB_SAMPLES + fine_time_offset samples, the NULL expected at its first sample and found fine_time_offset
    // (>= 0 here: nothing in front of the span can be read) samples later; freq_offset in cycles per sample, as the synchroniser reports
    // it.  false for a span that is too short or an offset outside [0, 1543]; out.valid = 0 (and weight 0: a dead branch) for a frame
    // without a finite estimate.
    bool Estimate(tcb::span<const std::complex<float>> null_and_prs, float freq_offset, int fine_time_offset, dabgpu_noise_record& out);

private:
    dabgpu_ctx* m_ctx;
};
