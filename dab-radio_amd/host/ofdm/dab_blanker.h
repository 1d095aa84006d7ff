// ofdm/dab_blanker.h -- one stream's impulse blanker on the device (include/dabgpu.h, "Impulse blanker"): zeroes bursts in the samples
// ahead of OFDM_Demod.  The reference has no blanker; the classes follow the conventions of DAB_Interferer and DAB_Stream_Resampler: spans
// in, exceptions for device failures.
#pragma once
#include <complex>
#include <cstdint>
#include <vector>

#include "dabgpu.h"
#include "utility/span.h"

// A thin owner over a bank of one stream.  The stream position lives in the object (on the device): consecutive Apply calls go on where
// the last one ended; the input is indexed absolutely (sample i of `in` is absolute sample params.start + i).
class DAB_Blanker {
public:
    // the widest parameters the object will carry (later SetParams calls must fit their gap + window + guard)
    explicit DAB_Blanker(const dabgpu_blanker_stream& params);
    ~DAB_Blanker();
    DAB_Blanker(const DAB_Blanker&) = delete;
    DAB_Blanker& operator=(const DAB_Blanker&) = delete;
    // dabgpu_blanker_defaults() with another threshold
    static dabgpu_blanker_stream Defaults(float threshold = 3.0f);
    void SetParams(const dabgpu_blanker_stream& params);
    void Seek(uint64_t position);
    // out.size() samples from the current position on, read from `in` (absolute indices; samples outside it are 0); mask (may be empty):
    // dabgpu_blanker_mask_words(out.size()) words.  false for an empty input or a mask of another size
    bool Apply(tcb::span<std::complex<float>> out, tcb::span<const std::complex<float>> in, tcb::span<uint32_t> mask = {});
private:
    dabgpu_blanker_bank* m_bank = nullptr;
};

// A stream through a DAB_Blanker, block by block: Process() is given the next samples of the input stream, whatever their count, and
// appends every output sample whose decision they complete -- whole blocks of 32, gap + window + guard blocks (800 samples with the
// defaults) behind the input.  Flush() appends the rest at the end of the input, decided with zeros behind it.  The outputs are those of
// one bank call over the whole input, whatever the blocks' sizes: the object keeps the input samples that outputs still to come read, and
// moves the bank's `start` with that window.  The first sample given to Process() is sample 0 of the stream: params.start must be 0 (the
// constructor throws otherwise), and Flush() ends the stream: Process() after it throws (blocks are whole only up to the flush).
class DAB_Stream_Blanker {
public:
    explicit DAB_Stream_Blanker(const dabgpu_blanker_stream& params);
    void Process(tcb::span<const std::complex<float>> in, std::vector<std::complex<float>>& out);
    void Flush(std::vector<std::complex<float>>& out);
    uint64_t BlankedBlocks() const { return m_blanked; }       // of the blocks emitted so far
    uint64_t TotalBlocks() const { return m_total; }
private:
    void Emit(uint64_t end, std::vector<std::complex<float>>& out);   // output samples m_emitted .. end
    dabgpu_blanker_stream m_params;                            // start = 0: the first sample given to Process is sample 0
    DAB_Blanker m_blanker;
    std::vector<std::complex<float>> m_window;                 // input samples m_origin .. m_received of the stream
    std::vector<uint32_t> m_mask;
    uint64_t m_origin = 0, m_received = 0, m_emitted = 0, m_blanked = 0, m_total = 0;
    uint64_t m_reach;                                          // samples
    bool m_flushed = false;
};
