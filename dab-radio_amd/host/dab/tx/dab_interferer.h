// dab/tx/dab_interferer.h -- one stream's interferer on the device (include/dabgpu.h, "Interferer"): up to 4 sources -- tones, band-limited
// noise, gated bursts -- added to the samples between a channel (DAB_Channel_Model) and a receiver (OFDM_Demod).  The reference has no
// interferer; the class follows the conventions of DAB_Channel_Model: spans in, false for wrong buffer sizes, exceptions for device
// failures.  The stream position lives in the object (on the device): consecutive Apply calls continue the oscillators, the noise and the
// gates block by block, whatever the block length; Seek() repositions.
#pragma once
#include <complex>
#include <cstdint>
#include <vector>

#include "dabgpu.h"
#include "utility/span.h"

class DAB_Interferer {
public:
    // the widest parameters the object will carry (later SetParams calls must fit their shaped BAND sources) and the shapes its BAND
    // sources name by index (dabgpu_interferer_design), at most DABGPU_INTERFERER_MAX_SHAPES
    DAB_Interferer(const dabgpu_interferer_stream& params, tcb::span<const dabgpu_interferer_shape> shapes);
    ~DAB_Interferer();
    DAB_Interferer(const DAB_Interferer&) = delete;
    DAB_Interferer& operator=(const DAB_Interferer&) = delete;
    // cycles per sample of an offset in Hz at DAB's 2.048 MHz, as dabgpu_interferer_source::freq_q64 (DAB_Channel_Model::FrequencyWord)
    static uint64_t FrequencyWord(double hz) { return dabgpu_channel_freq_q64(hz / 2.048e6); }
    // amp of a source is_db dB above (below: negative) a signal of mean power signal_power: E|v|^2 = amp^2 while its gate is on
    static float Amplitude(double signal_power, double is_db);
    // the shape of a band width_hz wide at 2.048 MHz; throws for a width the design refuses
    static dabgpu_interferer_shape Shape(double width_hz);
    void SetParams(const dabgpu_interferer_stream& params);
    void Seek(uint64_t position);
    // out = in + the interferer, in.size() samples from the current position; false for sizes that differ.  An empty `in` with a non-empty
    // `out`: the interferer alone.  out may be in (in place)
    bool Apply(tcb::span<std::complex<float>> out, tcb::span<const std::complex<float>> in);
    // the same as u8 pairs through the modulator's quantiser: out.size() = 2 x samples
    bool ApplyU8(tcb::span<uint8_t> out, tcb::span<const std::complex<float>> in, float u8_scale);
private:
    dabgpu_interferer_bank* m_bank = nullptr;
};
