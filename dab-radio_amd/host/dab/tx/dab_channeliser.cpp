// dab/tx/dab_channeliser.cpp -- see dab_channeliser.h
#include "./dab_channeliser.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>

#include "dab/dabgpu_shared_context.h"
#include "./dabgpu_tx_check.h"

static void check(int st, const char* what) { dabgpu_tx_check("DAB_Channeliser", st, what); }

DAB_Channeliser::DAB_Channeliser(int decim, const std::vector<dabgpu_channeliser_channel>& channels, int64_t start, double passband_cycles,
                                 double stopband_cycles)
    : m_channels(channels), m_start(start), m_decim(decim) {
    dabgpu_tx_check_abi("DAB_Channeliser");
    auto design = std::make_unique<dabgpu_channeliser_filter>();
    check(dabgpu_channeliser_design(decim, passband_cycles, stopband_cycles, design.get()), "dabgpu_channeliser_design");
    m_error = design->error;
    check(dabgpu_channeliser_bank_create(dabgpu_shared_context(), channels.data(), channels.size(), 1, start, design.get(), &m_bank),
          "dabgpu_channeliser_bank_create");
}

DAB_Channeliser::~DAB_Channeliser() { dabgpu_channeliser_bank_destroy(m_bank); }

dabgpu_channeliser_channel DAB_Channeliser::Channel(double offset_hz, double rate_hz, double level_db, uint64_t phase0_q64) {
    dabgpu_channeliser_channel C = {};
    C.freq_q64 = dabgpu_channeliser_freq_q64(offset_hz, rate_hz);
    C.phase0_q64 = phase0_q64;
    C.gain = (float)std::pow(10.0, level_db / 20.0);
    C.stream = 0;
    return C;
}

void DAB_Channeliser::SetParams(const std::vector<dabgpu_channeliser_channel>& channels, int64_t start) {
    check(dabgpu_channeliser_bank_set_params(m_bank, channels.data(), channels.size(), start, nullptr), "dabgpu_channeliser_bank_set_params");
    check(dabgpu_synchronize(dabgpu_shared_context(), nullptr), "dabgpu_synchronize");
    m_channels = channels;
    m_start = start;
}

void DAB_Channeliser::Seek(uint64_t position) {
    check(dabgpu_channeliser_bank_seek(m_bank, position, nullptr), "dabgpu_channeliser_bank_seek");
    check(dabgpu_synchronize(dabgpu_shared_context(), nullptr), "dabgpu_synchronize");
    m_position = position;
}

void DAB_Channeliser::InputNeeded(size_t n_out, int64_t& first, uint64_t& count) const {
    check(dabgpu_channeliser_input_needed(m_decim, m_position, m_start, n_out, &first, &count), "dabgpu_channeliser_input_needed");
}

bool DAB_Channeliser::Split(tcb::span<std::complex<float>> out, tcb::span<const std::complex<float>> in, bool wrap) {
    const size_t rows = m_channels.size();
    if (in.empty() || rows == 0 || out.size() % rows) return false;
    const size_t n_out = out.size() / rows;
    check(dabgpu_channeliser_bank_split_host_sync(m_bank, reinterpret_cast<const float*>(in.data()), 0, in.size(), wrap ? 1 : 0, n_out,
                                                  reinterpret_cast<float*>(out.data()), 0), "dabgpu_channeliser_bank_split_host_sync");
    m_position += n_out;
    return true;
}

bool DAB_Channeliser::Combine(tcb::span<std::complex<float>> out, tcb::span<const std::complex<float>> in, bool wrap) {
    const size_t rows = m_channels.size();
    if (in.empty() || rows == 0 || in.size() % rows) return false;
    const size_t n_in = in.size() / rows;
    check(dabgpu_channeliser_bank_combine_host_sync(m_bank, reinterpret_cast<const float*>(in.data()), rows > 1 ? n_in : 0, n_in, wrap ? 1 : 0, out.size(),
                                                    out.data(), DABGPU_IQ_RAW_F32L, 0, 1.0f), "dabgpu_channeliser_bank_combine_host_sync");
    m_position += out.size();
    return true;
}

bool DAB_Channeliser::CombineU8(tcb::span<uint8_t> out, tcb::span<const std::complex<float>> in, bool wrap, float u8_scale) {
    const size_t rows = m_channels.size();
    if (in.empty() || rows == 0 || in.size() % rows || (out.size() & 1)) return false;
    const size_t n_in = in.size() / rows;
    check(dabgpu_channeliser_bank_combine_host_sync(m_bank, reinterpret_cast<const float*>(in.data()), rows > 1 ? n_in : 0, n_in, wrap ? 1 : 0,
                                                    out.size() / 2, out.data(), DABGPU_IQ_RAW_U8, 0, u8_scale), "dabgpu_channeliser_bank_combine_host_sync");
    m_position += out.size() / 2;
    return true;
}

// ---- DAB_Stream_Channeliser ----
DAB_Stream_Channeliser::DAB_Stream_Channeliser(int decim, const std::vector<dabgpu_channeliser_channel>& channels, double passband_cycles,
                                               double stopband_cycles)
    : m_base(channels), m_channeliser(decim, channels, 0, passband_cycles, stopband_cycles) {}

void DAB_Stream_Channeliser::Process(tcb::span<const std::complex<float>> in, std::vector<std::vector<std::complex<float>>>& out) {
    m_window.insert(m_window.end(), in.begin(), in.end());
    out.resize(m_base.size());
    const int64_t D = m_channeliser.Decim(), K = D == 1 ? 1 : DABGPU_CHANNELISER_TAPS_PER_PHASE * D, P = D == 1 ? 0 : K / 2 - 1;
    const int64_t end = m_origin + (int64_t)m_window.size();                 // first input index not yet here
    const int64_t position = (int64_t)m_channeliser.Position();
    // output m reads the inputs m D - P .. m D - P + K - 1: complete while m D - P + K <= end
    const int64_t last = (end - K + P >= 0) ? (end - K + P) / D : -1;
    if (last < position) return;
    const size_t n = (size_t)(last - position + 1);
    // window sample 0 = stream sample m_origin: `start` moves by the origin, and so does every oscillator's phase
    std::vector<dabgpu_channeliser_channel> now = m_base;
    for (auto& C : now) C.phase0_q64 += (uint64_t)m_origin * C.freq_q64;
    m_channeliser.SetParams(now, -m_origin);
    m_rows.resize(n * m_base.size());
    m_channeliser.Split(m_rows, m_window, false);
    for (size_t c = 0; c < m_base.size(); c++) out[c].insert(out[c].end(), m_rows.begin() + (long)(c * n), m_rows.begin() + (long)((c + 1) * n));
    // what the next output still reads begins at (position + n) D - P
    const int64_t first = (position + (int64_t)n) * D - P;
    if (first > m_origin) {
        const size_t drop = std::min((size_t)(first - m_origin), m_window.size());
        m_window.erase(m_window.begin(), m_window.begin() + (long)drop);
        m_origin += (int64_t)drop;
    }
}

// ---- DAB_Stream_Combiner ----
DAB_Stream_Combiner::DAB_Stream_Combiner(int decim, const std::vector<dabgpu_channeliser_channel>& channels, double passband_cycles, double stopband_cycles)
    : m_base(channels), m_channeliser(decim, channels, 0, passband_cycles, stopband_cycles), m_window(channels.size()) {}

size_t DAB_Stream_Combiner::Admit(tcb::span<const std::complex<float>> rows) {
    const size_t C = m_base.size();
    if (C == 0 || rows.size() % C) throw std::runtime_error("DAB_Stream_Combiner: the rows' size is no multiple of the channel count");
    const size_t n = rows.size() / C;
    for (size_t c = 0; c < C; c++) m_window[c].insert(m_window[c].end(), rows.begin() + (long)(c * n), rows.begin() + (long)((c + 1) * n));
    const int64_t D = m_channeliser.Decim(), P = D == 1 ? 0 : DABGPU_CHANNELISER_TAPS_PER_PHASE * D / 2 - 1;
    const int64_t end = m_origin + (int64_t)m_window[0].size();              // first block sample not yet here
    // wideband sample i reads block samples up to floor((i + P) / D): complete while that is below `end`
    const int64_t total = end * D - P, position = (int64_t)m_channeliser.Position();
    if (total <= position || m_window[0].empty()) return 0;
    const size_t len = m_window[0].size();
    m_flat.resize(C * len);
    for (size_t c = 0; c < C; c++) std::copy(m_window[c].begin(), m_window[c].end(), m_flat.begin() + (long)(c * len));
    m_channeliser.SetParams(m_base, m_origin * D);                           // window sample 0 = block sample m_origin = wideband sample m_origin D
    return (size_t)(total - position);
}

void DAB_Stream_Combiner::Retire() {
    const int64_t D = m_channeliser.Decim(), NT = D == 1 ? 1 : DABGPU_CHANNELISER_TAPS_PER_PHASE, P = D == 1 ? 0 : NT * D / 2 - 1;
    const int64_t t = (int64_t)m_channeliser.Position() + P;                 // >= 0
    const int64_t first = t / D - (NT - 1);                                  // the earliest block sample the next output reads
    if (first > m_origin) {
        const size_t drop = std::min((size_t)(first - m_origin), m_window[0].size());
        for (auto& w : m_window) w.erase(w.begin(), w.begin() + (long)drop);
        m_origin += (int64_t)drop;
    }
}

void DAB_Stream_Combiner::Process(tcb::span<const std::complex<float>> rows, std::vector<std::complex<float>>& out) {
    const size_t n = Admit(rows);
    if (n == 0) return;
    const size_t at = out.size();
    out.resize(at + n);
    m_channeliser.Combine(tcb::span<std::complex<float>>(out.data() + at, n), m_flat, false);
    Retire();
}

void DAB_Stream_Combiner::ProcessU8(tcb::span<const std::complex<float>> rows, std::vector<uint8_t>& out, float u8_scale) {
    const size_t n = Admit(rows);
    if (n == 0) return;
    const size_t at = out.size();
    out.resize(at + 2 * n);
    m_channeliser.CombineU8(tcb::span<uint8_t>(out.data() + at, 2 * n), m_flat, false, u8_scale);
    Retire();
}
