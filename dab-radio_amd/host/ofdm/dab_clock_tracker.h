// ofdm/dab_clock_tracker.h -- the sampling-clock tracker of one mode I receiver (include/dabgpu.h, "Sampling-clock tracker"): every
// frame's own DQPSK products give the slope of the phase ramp that a sampling-clock error leaves over the carriers, the slope is
// carried from frame to frame, and the products leave with the ramp taken out -- ahead of everything else that reads them (the
// profiles, DAB_Diversity_Combiner).  The reference has no such stage; the class follows the conventions of the other added classes:
// spans in, false for wrong sizes, exceptions for device failures.  The state survives a resynchronisation: a crystal does not change
// when the signal fades, so only Reset() forgets it.
#pragma once
#include <complex>
#include <cstdint>

#include "dabgpu.h"
#include "utility/span.h"

struct dabgpu_ctx;

class DAB_Clock_Tracker {
public:
    static constexpr size_t NB_PRODUCTS = 75 * 1536;            // one frame's products, symbol after symbol in carrier order
    explicit DAB_Clock_Tracker(float gain = 1.0f);              // a gain outside (0, 1]: std::invalid_argument
    // products: the frame's NB_PRODUCTS products (OFDM_Demod's DQPSK view, a branch's d_dqpsk), de-rotated IN PLACE by the slope as
    // this frame has updated it.  false: the span has another size (nothing happened), or the frame gave no usable measurement -- the
    // state is kept and the products are still de-rotated by it.  IsValid() tells the two apart.
    bool Track(tcb::span<std::complex<float>> products);
    bool IsValid() const { return m_valid; }                    // of the last Track
    double GetPpm() const { return dabgpu_clock_ppm(m_slope); } // the sign of dabgpu_simulate_transmitter --clock-ppm
    int64_t GetSlope() const { return m_slope; }
    tcb::span<const float> GetCorrelation() const { return {m_corr, 2}; }      // the folded sum A of the last Track (0, 0: skipped)
    bool SetGain(float gain);                                   // false (and no change) outside (0, 1]
    float GetGain() const { return m_gain; }
    void Reset() { m_slope = 0; m_valid = false; m_corr[0] = m_corr[1] = 0.0f; }

private:
    dabgpu_ctx* m_ctx;
    int64_t m_slope = 0;
    float m_gain;
    float m_corr[2] = {0.0f, 0.0f};
    bool m_valid = false;
};
