// ofdm/dab_iq_balancer.h -- one stream's IQ balance on the device (include/dabgpu.h, "IQ balance"): the DC term and the mirror image of a
// zero-IF front end, made (a FIXED stream: the simulator's impairment) or removed blindly (a TRACK stream) ahead of resampler, channeliser,
// blanker and OFDM_Demod.  The reference has nothing comparable; the classes follow the conventions of DAB_Blanker: spans in, exceptions for
// device failures.
#pragma once
#include <complex>
#include <cstdint>
#include <vector>

#include "dabgpu.h"
#include "utility/span.h"

// A thin owner over a bank of one stream.  The stream position and the estimator's record live in the object (on the device): consecutive
// Apply calls go on where the last one ended.
class DAB_IQ_Balancer {
public:
    // max_samples_per_call: the most a MEASURE call may hold (a multiple of 1024)
    DAB_IQ_Balancer(const dabgpu_iqbal_stream& params, size_t max_samples_per_call);
    ~DAB_IQ_Balancer();
    DAB_IQ_Balancer(const DAB_IQ_Balancer&) = delete;
    DAB_IQ_Balancer& operator=(const DAB_IQ_Balancer&) = delete;
    // dabgpu_iqbal_defaults(), with another memory where time_constant_samples > 0
    static dabgpu_iqbal_stream Defaults(double time_constant_samples = 0.0);
    // dabgpu_iqbal_impairment: the FIXED stream of a front end with these errors
    static dabgpu_iqbal_stream Impairment(double gain_db, double phase_deg, std::complex<double> dc = {0.0, 0.0});
    // what a corrector with this record leaves of the image it found: -20 log10 |w| dB is the front end's own rejection (+infinity for w = 0)
    static double FrontEndRejectionDb(const dabgpu_iqbal_record& record);
    void SetParams(const dabgpu_iqbal_stream& params);
    void Seek(uint64_t position);
    void Reset();
    // in.size() samples from the current position on; flags: DABGPU_IQBAL_MEASURE, DABGPU_IQBAL_APPLY or both.  With APPLY out.size() must
    // be in.size() (out may be the input's own memory); without it out is not touched.  false for an empty input or another out size.
    // A MEASURE call off a tile edge or of a count that is no multiple of 1024 throws, as every refusal of the library
    bool Apply(tcb::span<std::complex<float>> out, tcb::span<const std::complex<float>> in, uint32_t flags);
    // APPLY alone, the output as u8 pairs through the modulator's quantiser (out.size() must be 2 in.size())
    bool ApplyU8(tcb::span<uint8_t> out, tcb::span<const std::complex<float>> in, float u8_scale);
    dabgpu_iqbal_record State() const;
private:
    dabgpu_iqbal_bank* m_bank = nullptr;
};

// A stream through a DAB_IQ_Balancer, block by block: Process() is given the next samples of the input stream, whatever their count, and
// appends the output of every chunk they complete; a chunk is chunk_samples (a multiple of 1024; a mode-I frame at 2.048 MS/s by default)
// from absolute sample 0 on.  prime = true: a chunk is measured first and mapped with the coefficients that include it (two passes: the
// first chunk is corrected already); false: one pass, mapped with the coefficients of the chunks before it.  Flush() appends the rest at
// the end of the input: its whole tiles are measured (prime) and all of it is mapped.  The outputs do not depend on the blocks' sizes.
class DAB_Stream_IQ_Balancer {
public:
    explicit DAB_Stream_IQ_Balancer(const dabgpu_iqbal_stream& params, size_t chunk_samples = 196608, bool prime = true);
    void Process(tcb::span<const std::complex<float>> in, std::vector<std::complex<float>>& out);
    void Flush(std::vector<std::complex<float>>& out);
    dabgpu_iqbal_record State() const { return m_balancer.State(); }
    uint64_t Chunks() const { return m_chunks; }               // whole chunks emitted so far
private:
    void Emit(size_t n, bool whole_tiles, std::vector<std::complex<float>>& out);    // the first n samples of m_pending
    DAB_IQ_Balancer m_balancer;
    std::vector<std::complex<float>> m_pending;                // input samples not yet emitted
    size_t m_chunk;
    uint64_t m_emitted = 0, m_chunks = 0;
    bool m_prime, m_flushed = false;
};
