// dab/tx/dab_channeliser.h -- one wideband stream's channeliser on the device (include/dabgpu.h, "Channeliser"): SPLIT turns a capture at
// D x the block rate into up to 8 block streams at their frequency offsets (in front of DAB_Resampler / OFDM_Demod), COMBINE puts up to 8
// block streams at their offsets and levels onto one wideband stream (behind DAB_Channel_Model).  The reference has no channeliser; the
// class follows the conventions of DAB_Resampler: spans in, false for wrong buffer sizes, exceptions for device failures.  The position
// lives in the object (on the device) and counts the output samples of the calls made: consecutive calls continue the stream, Seek()
// repositions.  Input sample indices are absolute like the position: every call is given the same input (wrap = true: a transmission that
// repeats), or a window of it after SetParams with `start` and the phases moved by the window's origin (DAB_Stream_Channeliser does that).
#pragma once
#include <complex>
#include <cstdint>
#include <vector>

#include "dabgpu.h"
#include "utility/span.h"

class DAB_Channeliser {
public:
    // channels: at most 8, their `stream` 0; the bank keeps room for this many.  Edges 0: the DAB block's 0.375 / 0.4609375
    DAB_Channeliser(int decim, const std::vector<dabgpu_channeliser_channel>& channels, int64_t start = 0, double passband_cycles = 0.0,
                    double stopband_cycles = 0.0);
    ~DAB_Channeliser();
    DAB_Channeliser(const DAB_Channeliser&) = delete;
    DAB_Channeliser& operator=(const DAB_Channeliser&) = delete;
    // the largest decimation <= 8 that leaves at least 2.048 MS/s (0: none)
    static int DecimFor(double rate_hz) { return dabgpu_channeliser_decim_for(rate_hz); }
    // a channel offset_hz from the centre of a capture at rate_hz; level_db: its gain as 10^(level_db / 20)
    static dabgpu_channeliser_channel Channel(double offset_hz, double rate_hz, double level_db = 0.0, uint64_t phase0_q64 = 0);
    // the figure dabgpu_channeliser_design found for the table in use: worst passband deviation + worst stopband level
    double DesignError() const { return m_error; }
    int Decim() const { return m_decim; }
    size_t Channels() const { return m_channels.size(); }
    void SetParams(const std::vector<dabgpu_channeliser_channel>& channels, int64_t start);
    void Seek(uint64_t position);
    uint64_t Position() const { return m_position; }
    // the wideband indices [first, first + count) the next Split of n_out samples reads
    void InputNeeded(size_t n_out, int64_t& first, uint64_t& count) const;
    // out = Channels() rows of n_out block samples, back to back; false for an empty input or a size that is no multiple of the rows
    bool Split(tcb::span<std::complex<float>> out, tcb::span<const std::complex<float>> in, bool wrap);
    // in = Channels() rows of block samples, back to back; out.size() wideband samples from the current position
    bool Combine(tcb::span<std::complex<float>> out, tcb::span<const std::complex<float>> in, bool wrap);
    // the same as u8 pairs through the modulator's quantiser: out.size() = 2 x samples
    bool CombineU8(tcb::span<uint8_t> out, tcb::span<const std::complex<float>> in, bool wrap, float u8_scale);
private:
    dabgpu_channeliser_bank* m_bank = nullptr;
    std::vector<dabgpu_channeliser_channel> m_channels;
    int64_t m_start = 0;
    int m_decim = 1;
    double m_error = 0.0;
    uint64_t m_position = 0;
};

// A wideband stream through a DAB_Channeliser, block by block: Process() is given the next samples of the capture, whatever their count,
// and appends to every channel's vector the block samples they complete (the last taps of an output may lie in the next block; samples in
// front of the stream are zero).  The outputs are those of one Split over the whole input, whatever the blocks' sizes: the object keeps the
// K - 1 input samples that outputs still to come read, and moves `start` and every channel's phase with that window, so the oscillators
// keep counting the stream's own sample indices.  Every Process() call that completes an output replaces the channel list on the device,
// waits for it, and copies the retained window to the device again (the host form of the split): right for a file tool's blocks of a
// hundred thousand samples, costly for blocks of a few samples -- a caller with small blocks should gather them first.
class DAB_Stream_Channeliser {
public:
    DAB_Stream_Channeliser(int decim, const std::vector<dabgpu_channeliser_channel>& channels, double passband_cycles = 0.0, double stopband_cycles = 0.0);
    void Process(tcb::span<const std::complex<float>> in, std::vector<std::vector<std::complex<float>>>& out);
    double DesignError() const { return m_channeliser.DesignError(); }
    size_t Channels() const { return m_base.size(); }
private:
    std::vector<dabgpu_channeliser_channel> m_base;            // the channels against absolute input indices
    DAB_Channeliser m_channeliser;
    std::vector<std::complex<float>> m_window;                 // input samples m_origin .. of the stream
    std::vector<std::complex<float>> m_rows;
    int64_t m_origin = 0;
};

// The other direction, block by block: Process() is given the next n samples of EVERY block stream (Channels() rows of n samples, back to
// back) and appends every wideband sample they complete: sample i needs the block samples up to floor((i + P) / D), so a call's last
// P samples' worth come with the next call; block samples in front of the streams are zero.  The outputs are those of one Combine over the
// whole rows, whatever the blocks' sizes: the object keeps the 71 block samples per row that later outputs still read and moves `start`
// with that window (the oscillators count wideband output samples, which the position carries).  The cost note above holds here too.
class DAB_Stream_Combiner {
public:
    DAB_Stream_Combiner(int decim, const std::vector<dabgpu_channeliser_channel>& channels, double passband_cycles = 0.0, double stopband_cycles = 0.0);
    void Process(tcb::span<const std::complex<float>> rows, std::vector<std::complex<float>>& out);
    // the same as u8 pairs through the modulator's quantiser (2 bytes appended per sample)
    void ProcessU8(tcb::span<const std::complex<float>> rows, std::vector<uint8_t>& out, float u8_scale);
    double DesignError() const { return m_channeliser.DesignError(); }
    size_t Channels() const { return m_base.size(); }
private:
    size_t Admit(tcb::span<const std::complex<float>> rows);   // takes the rows in, lays the windows out; the outputs now complete (0: none yet)
    void Retire();                                             // drops the block samples that no later output reads
    std::vector<dabgpu_channeliser_channel> m_base;
    DAB_Channeliser m_channeliser;
    std::vector<std::vector<std::complex<float>>> m_window;    // per row: block samples m_origin .. of the stream
    std::vector<std::complex<float>> m_flat;
    int64_t m_origin = 0;
};
