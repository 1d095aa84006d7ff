// dab/tx/dab_resampler.h -- one stream's resampler on the device (include/dabgpu.h, "Resampler"): an arbitrary ratio between 0.5 and 2 and
// a fractional delay -- a receiver's sampling-clock error behind DAB_Channel_Model, or a capture at 2.4, 2.56, 3.072 or 4.096 MS/s brought to
// the 2.048 MHz grid in front of OFDM_Demod.  The reference has no resampler; the class follows the conventions of DAB_Channel_Model: spans
// in, false for wrong buffer sizes, exceptions for device failures.  The stream position lives in the object (on the device): consecutive
// Apply calls continue the stream, Seek() repositions.  Input sample indices are absolute like the position: every call is given the same
// input (wrap = true: a transmission that repeats), or a window of it after SetParams with the offset moved by the window's origin
// (InputNeeded says which samples a call reads).
#pragma once
#include <complex>
#include <cstdint>
#include <vector>

#include "dabgpu.h"
#include "utility/span.h"

class DAB_Resampler {
public:
    // the widest parameters the object will carry: the filter is designed for max(params.step, 1) and later SetParams calls must fit the
    // window and the table rows of this step (dabgpu_resample_bank_set_params); passband_cycles = 0: the DAB block's 0.375
    explicit DAB_Resampler(const dabgpu_resample_stream& params, double passband_cycles = 0.0);
    ~DAB_Resampler();
    DAB_Resampler(const DAB_Resampler&) = delete;
    DAB_Resampler& operator=(const DAB_Resampler&) = delete;
    // input samples per output sample for two sample rates and a clock error, as dabgpu_resample_stream::step_q62
    static uint64_t StepWord(double in_rate_hz, double out_rate_hz, double ppm = 0.0) { return dabgpu_resample_step_q62(in_rate_hz, out_rate_hz, ppm); }
    // step 1, no offset, gain 1: the identity; set step_q62 and the offset from there
    static dabgpu_resample_stream Params(uint64_t step_q62, double offset_samples = 0.0, float gain = 1.0f);
    // the figure dabgpu_resample_design found for the table in use: worst passband deviation + worst alias leakage
    double DesignError() const { return m_error; }
    void SetParams(const dabgpu_resample_stream& params);
    void Seek(uint64_t position);
    uint64_t Position() const { return m_position; }
    // the input indices [first, first + count) the next Apply of n_out samples reads
    void InputNeeded(size_t n_out, int64_t& first, uint64_t& count) const;
    // out.size() samples from the current position; false for an empty input
    bool Apply(tcb::span<std::complex<float>> out, tcb::span<const std::complex<float>> in, bool wrap);
    // the same as u8 pairs through the modulator's quantiser: out.size() = 2 x samples
    bool ApplyU8(tcb::span<uint8_t> out, tcb::span<const std::complex<float>> in, bool wrap, float u8_scale);
private:
    dabgpu_resample_bank* m_bank = nullptr;
    dabgpu_resample_stream m_params;
    double m_error = 0.0;
    uint64_t m_position = 0;
};

// A stream through a DAB_Resampler, block by block: Process() is given the next samples of the input stream, whatever their count, and
// appends every output sample they complete (the last taps of an output may lie in the next block; samples in front of the stream are
// zero).  The outputs are those of one Apply over the whole input, whatever the blocks' sizes: the object keeps the input samples that
// outputs still to come read, and moves the resampler's offset with that window (DAB_Resampler::SetParams).
class DAB_Stream_Resampler {
public:
    // step_q62 = DAB_Resampler::StepWord(in_rate, out_rate, ppm); delay: a delay of the output in input samples, 0 <= delay < 1
    explicit DAB_Stream_Resampler(uint64_t step_q62, double delay = 0.0, double passband_cycles = 0.0);
    void Process(tcb::span<const std::complex<float>> in, std::vector<std::complex<float>>& out);
    // the same as u8 pairs through the modulator's quantiser (2 bytes appended per sample)
    void ProcessU8(tcb::span<const std::complex<float>> in, std::vector<uint8_t>& out, float u8_scale);
    double DesignError() const { return m_resampler.DesignError(); }
private:
    size_t Admit(tcb::span<const std::complex<float>> in);     // takes the block in; the outputs that are now complete (0: none yet)
    void Retire();                                             // drops the input that no later output reads
    dabgpu_resample_stream m_base;                             // the stream's parameters against absolute input indices
    DAB_Resampler m_resampler;
    std::vector<std::complex<float>> m_window;                 // input samples m_origin .. of the stream
    int64_t m_origin = 0;
};
