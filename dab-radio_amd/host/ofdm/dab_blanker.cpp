// ofdm/dab_blanker.cpp -- see dab_blanker.h
#include "./dab_blanker.h"

#include "dab/dabgpu_shared_context.h"
#include "dab/tx/dabgpu_tx_check.h"

static void check(int st, const char* what) { dabgpu_tx_check("DAB_Blanker", st, what); }

DAB_Blanker::DAB_Blanker(const dabgpu_blanker_stream& params) {
    dabgpu_tx_check_abi("DAB_Blanker");
    check(dabgpu_blanker_bank_create(dabgpu_shared_context(), 1, &params, &m_bank), "dabgpu_blanker_bank_create");
}

DAB_Blanker::~DAB_Blanker() { dabgpu_blanker_bank_destroy(m_bank); }

dabgpu_blanker_stream DAB_Blanker::Defaults(float threshold) {
    dabgpu_blanker_stream P = dabgpu_blanker_defaults();
    P.threshold = threshold;
    return P;
}

void DAB_Blanker::SetParams(const dabgpu_blanker_stream& params) {
    check(dabgpu_blanker_bank_set_params(m_bank, &params, nullptr), "dabgpu_blanker_bank_set_params");
    check(dabgpu_synchronize(dabgpu_shared_context(), nullptr), "dabgpu_synchronize");
}

void DAB_Blanker::Seek(uint64_t position) {
    check(dabgpu_blanker_bank_seek(m_bank, position, nullptr), "dabgpu_blanker_bank_seek");
    check(dabgpu_synchronize(dabgpu_shared_context(), nullptr), "dabgpu_synchronize");
}

bool DAB_Blanker::Apply(tcb::span<std::complex<float>> out, tcb::span<const std::complex<float>> in, tcb::span<uint32_t> mask) {
    if (in.empty() || (!mask.empty() && mask.size() != dabgpu_blanker_mask_words(out.size()))) return false;
    check(dabgpu_blanker_bank_apply_host_sync(m_bank, reinterpret_cast<const float*>(in.data()), 0, in.size(), out.size(), out.data(), 0,
                                              mask.empty() ? nullptr : mask.data(), 0), "dabgpu_blanker_bank_apply_host_sync");
    return true;
}

// ---- DAB_Stream_Blanker ----
// the stream's own first sample is absolute sample 0: the window below is what moves `start`, so the caller's must be 0
static const dabgpu_blanker_stream& stream_params(const dabgpu_blanker_stream& params) {
    if (params.start != 0) throw std::runtime_error("DAB_Stream_Blanker: start must be 0 (the first sample given to Process is sample 0 of the stream)");
    return params;
}

DAB_Stream_Blanker::DAB_Stream_Blanker(const dabgpu_blanker_stream& params)
    : m_params(stream_params(params)), m_blanker(params),
      m_reach(params.enabled ? (uint64_t)(params.gap + params.window + params.guard) * DABGPU_BLANKER_POWER_BLOCK : 0) {}

void DAB_Stream_Blanker::Emit(uint64_t end, std::vector<std::complex<float>>& out) {
    if (end <= m_emitted) return;
    const size_t n = (size_t)(end - m_emitted), at = out.size();
    dabgpu_blanker_stream P = m_params;                        // the window begins at absolute sample m_origin of this stream
    P.start = (int64_t)m_origin;
    m_blanker.SetParams(P);
    out.resize(at + n);
    m_mask.assign(dabgpu_blanker_mask_words(n), 0u);
    if (!m_blanker.Apply({out.data() + at, n}, m_window, m_mask)) throw std::runtime_error("DAB_Stream_Blanker: nothing to read");
    for (uint32_t w : m_mask) m_blanked += (uint64_t)__builtin_popcount(w);
    m_total += (n + DABGPU_BLANKER_POWER_BLOCK - 1) / DABGPU_BLANKER_POWER_BLOCK;     // (m_emitted is a multiple of 32)
    m_emitted = end;
    // what the outputs still to come read: from `reach` before the block of the next output on
    const uint64_t keep = m_emitted > m_reach ? m_emitted - m_reach : 0;
    if (keep > m_origin) {
        m_window.erase(m_window.begin(), m_window.begin() + (size_t)(keep - m_origin));
        m_origin = keep;
    }
}

void DAB_Stream_Blanker::Process(tcb::span<const std::complex<float>> in, std::vector<std::complex<float>>& out) {
    if (m_flushed) throw std::runtime_error("DAB_Stream_Blanker: Process after Flush (the stream has ended; make a new object for another)");
    m_window.insert(m_window.end(), in.begin(), in.end());
    m_received += in.size();
    // a block is decided once the input holds `reach` samples behind its end
    const uint64_t whole = m_received & ~(uint64_t)(DABGPU_BLANKER_POWER_BLOCK - 1);
    if (whole > m_reach) Emit(whole - m_reach, out);
}

void DAB_Stream_Blanker::Flush(std::vector<std::complex<float>>& out) {
    Emit(m_received, out);
    m_flushed = true;
}
