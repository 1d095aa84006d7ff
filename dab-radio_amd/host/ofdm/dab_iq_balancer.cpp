// ofdm/dab_iq_balancer.cpp -- see dab_iq_balancer.h
#include "./dab_iq_balancer.h"

#include <cmath>
#include <limits>
#include <stdexcept>

#include "dab/dabgpu_shared_context.h"
#include "dab/tx/dabgpu_tx_check.h"

static void check(int st, const char* what) { dabgpu_tx_check("DAB_IQ_Balancer", st, what); }

DAB_IQ_Balancer::DAB_IQ_Balancer(const dabgpu_iqbal_stream& params, size_t max_samples_per_call) {
    dabgpu_tx_check_abi("DAB_IQ_Balancer");
    check(dabgpu_iqbal_bank_create(dabgpu_shared_context(), 1, &params, max_samples_per_call, &m_bank), "dabgpu_iqbal_bank_create");
}

DAB_IQ_Balancer::~DAB_IQ_Balancer() { dabgpu_iqbal_bank_destroy(m_bank); }

dabgpu_iqbal_stream DAB_IQ_Balancer::Defaults(double time_constant_samples) {
    dabgpu_iqbal_stream P = dabgpu_iqbal_defaults();
    if (time_constant_samples > 0.0) {
        P.forget = dabgpu_iqbal_forget(time_constant_samples);
        if (P.forget == 0.0f) throw std::runtime_error("DAB_IQ_Balancer: the time constant must be at least one tile of 1024 samples");
    }
    return P;
}

dabgpu_iqbal_stream DAB_IQ_Balancer::Impairment(double gain_db, double phase_deg, std::complex<double> dc) {
    dabgpu_iqbal_stream P;
    check(dabgpu_iqbal_impairment(gain_db, phase_deg, dc.real(), dc.imag(), &P), "dabgpu_iqbal_impairment");
    return P;
}

double DAB_IQ_Balancer::FrontEndRejectionDb(const dabgpu_iqbal_record& record) {
    const double w = std::hypot((double)record.w_re, (double)record.w_im);
    return w > 0.0 ? -20.0 * std::log10(w) : std::numeric_limits<double>::infinity();
}

void DAB_IQ_Balancer::SetParams(const dabgpu_iqbal_stream& params) {
    check(dabgpu_iqbal_bank_set_params(m_bank, &params, nullptr), "dabgpu_iqbal_bank_set_params");
    check(dabgpu_synchronize(dabgpu_shared_context(), nullptr), "dabgpu_synchronize");
}

void DAB_IQ_Balancer::Seek(uint64_t position) {
    check(dabgpu_iqbal_bank_seek(m_bank, position, nullptr), "dabgpu_iqbal_bank_seek");
    check(dabgpu_synchronize(dabgpu_shared_context(), nullptr), "dabgpu_synchronize");
}

void DAB_IQ_Balancer::Reset() {
    check(dabgpu_iqbal_bank_reset(m_bank, nullptr), "dabgpu_iqbal_bank_reset");
    check(dabgpu_synchronize(dabgpu_shared_context(), nullptr), "dabgpu_synchronize");
}

bool DAB_IQ_Balancer::Apply(tcb::span<std::complex<float>> out, tcb::span<const std::complex<float>> in, uint32_t flags) {
    const bool apply = (flags & DABGPU_IQBAL_APPLY) != 0;
    if (in.empty() || (apply && out.size() != in.size())) return false;
    check(dabgpu_iqbal_bank_apply_host_sync(m_bank, reinterpret_cast<const float*>(in.data()), 0, in.size(), apply ? out.data() : nullptr,
                                            DABGPU_IQ_RAW_F32L, 0, 1.0f, flags), "dabgpu_iqbal_bank_apply_host_sync");
    return true;
}

bool DAB_IQ_Balancer::ApplyU8(tcb::span<uint8_t> out, tcb::span<const std::complex<float>> in, float u8_scale) {
    if (in.empty() || out.size() != 2 * in.size()) return false;
    check(dabgpu_iqbal_bank_apply_host_sync(m_bank, reinterpret_cast<const float*>(in.data()), 0, in.size(), out.data(), DABGPU_IQ_RAW_U8, 0, u8_scale,
                                            DABGPU_IQBAL_APPLY), "dabgpu_iqbal_bank_apply_host_sync");
    return true;
}

dabgpu_iqbal_record DAB_IQ_Balancer::State() const {
    dabgpu_iqbal_record R;
    check(dabgpu_iqbal_bank_read_state_host_sync(m_bank, &R), "dabgpu_iqbal_bank_read_state_host_sync");
    return R;
}

// ---- DAB_Stream_IQ_Balancer ----
static size_t chunk_checked(size_t chunk_samples) {
    if (chunk_samples == 0 || (chunk_samples & (DABGPU_IQBAL_TILE - 1)))
        throw std::runtime_error("DAB_Stream_IQ_Balancer: chunk_samples must be a multiple of 1024");
    return chunk_samples;
}

DAB_Stream_IQ_Balancer::DAB_Stream_IQ_Balancer(const dabgpu_iqbal_stream& params, size_t chunk_samples, bool prime)
    : m_balancer(params, chunk_checked(chunk_samples)), m_chunk(chunk_samples), m_prime(prime) {}

void DAB_Stream_IQ_Balancer::Emit(size_t n, bool whole_tiles, std::vector<std::complex<float>>& out) {
    if (n == 0) return;
    const size_t at = out.size(), tiles = n & ~(size_t)(DABGPU_IQBAL_TILE - 1);
    const tcb::span<const std::complex<float>> in{m_pending.data(), n};
    out.resize(at + n);
    const tcb::span<std::complex<float>> dst{out.data() + at, n};
    bool ok = true;
    if (m_prime) {
        if (tiles) {                                           // measured first, then mapped from the same position on
            ok = m_balancer.Apply({}, {m_pending.data(), tiles}, DABGPU_IQBAL_MEASURE);
            m_balancer.Seek(m_emitted);
        }
        ok = ok && m_balancer.Apply(dst, in, DABGPU_IQBAL_APPLY);
    } else if (whole_tiles) {
        ok = m_balancer.Apply(dst, in, DABGPU_IQBAL_MEASURE | DABGPU_IQBAL_APPLY);
    } else {                                                   // the stream's end: its whole tiles in one pass, the rest mapped only
        if (tiles) ok = m_balancer.Apply({dst.data(), tiles}, {m_pending.data(), tiles}, DABGPU_IQBAL_MEASURE | DABGPU_IQBAL_APPLY);
        if (n > tiles) ok = ok && m_balancer.Apply({dst.data() + tiles, n - tiles}, {m_pending.data() + tiles, n - tiles}, DABGPU_IQBAL_APPLY);
    }
    if (!ok) throw std::runtime_error("DAB_Stream_IQ_Balancer: nothing to read");
    m_emitted += n;
    m_pending.erase(m_pending.begin(), m_pending.begin() + (ptrdiff_t)n);
}

void DAB_Stream_IQ_Balancer::Process(tcb::span<const std::complex<float>> in, std::vector<std::complex<float>>& out) {
    if (m_flushed) throw std::runtime_error("DAB_Stream_IQ_Balancer: Process after Flush (the stream has ended; make a new object for another)");
    m_pending.insert(m_pending.end(), in.begin(), in.end());
    while (m_pending.size() >= m_chunk) {
        Emit(m_chunk, true, out);
        m_chunks++;
    }
}

void DAB_Stream_IQ_Balancer::Flush(std::vector<std::complex<float>>& out) {
    Emit(m_pending.size(), false, out);
    m_flushed = true;
}
