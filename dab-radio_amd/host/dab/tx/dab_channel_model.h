// dab/tx/dab_channel_model.h -- one stream's channel on the device (include/dabgpu.h, "Channel model"): up to 8 paths, carrier offset,
// timing offset, gain and white Gaussian noise between a transmitter (DAB_Channel_Encoder, OFDM_Modulator) and a receiver (OFDM_Demod).
// The reference has no channel model; the class follows the conventions of DAB_Channel_Encoder: spans in, false for wrong buffer
// sizes, exceptions for device failures.  The stream position lives in the object (on the device): consecutive Apply calls continue
// the oscillator and the noise sequence, Seek() repositions.  Input sample indices are absolute like the position: every call is given
// the same input (wrap = true: a transmission that repeats), or a window of it after SetParams with `start` moved by the window's origin.
#pragma once
#include <complex>
#include <cstdint>

#include "dabgpu.h"
#include "utility/span.h"

class DAB_Channel_Model {
public:
    // the widest parameters the object will carry: later SetParams calls must fit their delays (dabgpu_channel_bank_set_params)
    explicit DAB_Channel_Model(const dabgpu_channel_stream& params);
    ~DAB_Channel_Model();
    DAB_Channel_Model(const DAB_Channel_Model&) = delete;
    DAB_Channel_Model& operator=(const DAB_Channel_Model&) = delete;
    // cycles per sample of a carrier offset in Hz at DAB's 2.048 MHz, as dabgpu_channel_stream::freq_q64
    static uint64_t FrequencyWord(double hz) { return dabgpu_channel_freq_q64(hz / 2.048e6); }
    // noise_sigma for a signal-to-noise ratio in dB and the mean power of the channel's noiseless output
    static float NoiseSigma(double mean_power, double snr_db);
    void SetParams(const dabgpu_channel_stream& params);
    // Rayleigh / Rice taps with Doppler (include/dabgpu.h, "Channel model, fading taps"): the tables are planned from `spec` for the
    // parameters in force (stream 0) and planned again by every later SetParams.  The first call turns the object into a fading bank at
    // the position it has reached; a model that never calls it is the class of before.
    void SetFading(const dabgpu_channel_fading_spec& spec);
    void Seek(uint64_t position);
    // out.size() samples from the current position; false for an empty input
    bool Apply(tcb::span<std::complex<float>> out, tcb::span<const std::complex<float>> in, bool wrap);
    // the same as u8 pairs through the modulator's quantiser: out.size() = 2 x samples
    bool ApplyU8(tcb::span<uint8_t> out, tcb::span<const std::complex<float>> in, bool wrap, float u8_scale);
private:
    dabgpu_channel_bank* m_bank = nullptr;
    dabgpu_channel_stream m_created, m_params;   // of the constructor (the widest), and in force
    dabgpu_channel_fading_spec m_spec = {};
    bool m_fading = false;
    uint64_t m_position = 0;                 // the bank's position, followed on the host: SetFading recreates the bank there
};
