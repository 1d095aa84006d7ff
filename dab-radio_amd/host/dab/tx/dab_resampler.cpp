// dab/tx/dab_resampler.cpp -- see dab_resampler.h
#include "./dab_resampler.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>

#include "dab/dabgpu_shared_context.h"
#include "./dabgpu_tx_check.h"

static void check(int st, const char* what) { dabgpu_tx_check("DAB_Resampler", st, what); }

DAB_Resampler::DAB_Resampler(const dabgpu_resample_stream& params, double passband_cycles) : m_params(params) {
    dabgpu_tx_check_abi("DAB_Resampler");
    // max_step: the step as a double rounded up (the planner compares words), at least 1; a step outside [0.5, 2] is the planner's to refuse
    double max_step = std::nextafter(dabgpu_resample_step(params.step_q62), 4.0);
    max_step = max_step <= 1.0 ? 1.0 : (max_step > 2.0 ? 2.0 : max_step);
    auto design = std::make_unique<dabgpu_resample_filter>();
    check(dabgpu_resample_design(max_step, passband_cycles, design.get()), "dabgpu_resample_design");
    m_error = design->error;
    check(dabgpu_resample_bank_create(dabgpu_shared_context(), 1, &params, design.get(), &m_bank), "dabgpu_resample_bank_create");
}

DAB_Resampler::~DAB_Resampler() { dabgpu_resample_bank_destroy(m_bank); }

dabgpu_resample_stream DAB_Resampler::Params(uint64_t step_q62, double offset_samples, float gain) {
    dabgpu_resample_stream P = {};
    const double whole = std::floor(offset_samples);
    P.step_q62 = step_q62;
    P.offset_samples = (int64_t)whole;
    const double frac = std::ldexp(offset_samples - whole, 62);              // in [0, 2^62]
    P.offset_frac_q62 = frac >= 0x1p62 ? ((uint64_t)1 << 62) - 1 : (uint64_t)frac;
    P.gain = gain;
    return P;
}

void DAB_Resampler::SetParams(const dabgpu_resample_stream& params) {
    check(dabgpu_resample_bank_set_params(m_bank, &params, nullptr), "dabgpu_resample_bank_set_params");
    check(dabgpu_synchronize(dabgpu_shared_context(), nullptr), "dabgpu_synchronize");
    m_params = params;
}

void DAB_Resampler::Seek(uint64_t position) {
    check(dabgpu_resample_bank_seek(m_bank, position, nullptr), "dabgpu_resample_bank_seek");
    check(dabgpu_synchronize(dabgpu_shared_context(), nullptr), "dabgpu_synchronize");
    m_position = position;
}

void DAB_Resampler::InputNeeded(size_t n_out, int64_t& first, uint64_t& count) const {
    check(dabgpu_resample_input_needed(&m_params, m_position, n_out, &first, &count), "dabgpu_resample_input_needed");
}

bool DAB_Resampler::Apply(tcb::span<std::complex<float>> out, tcb::span<const std::complex<float>> in, bool wrap) {
    if (in.empty()) return false;
    check(dabgpu_resample_bank_apply_host_sync(m_bank, reinterpret_cast<const float*>(in.data()), 0, in.size(), wrap ? 1 : 0, out.size(), out.data(),
                                               DABGPU_IQ_RAW_F32L, 0, 1.0f), "dabgpu_resample_bank_apply_host_sync");
    m_position += out.size();
    return true;
}

bool DAB_Resampler::ApplyU8(tcb::span<uint8_t> out, tcb::span<const std::complex<float>> in, bool wrap, float u8_scale) {
    if (in.empty() || (out.size() & 1)) return false;
    check(dabgpu_resample_bank_apply_host_sync(m_bank, reinterpret_cast<const float*>(in.data()), 0, in.size(), wrap ? 1 : 0, out.size() / 2, out.data(),
                                               DABGPU_IQ_RAW_U8, 0, u8_scale), "dabgpu_resample_bank_apply_host_sync");
    m_position += out.size() / 2;
    return true;
}

// ---- DAB_Stream_Resampler ----
static dabgpu_resample_stream stream_params(uint64_t step_q62, double delay) {
    if (!(delay >= 0.0 && delay < 1.0)) throw std::runtime_error("DAB_Stream_Resampler: the delay is a fraction of a sample, 0 <= delay < 1");
    // a delay of d samples: output m is taken d earlier in the input, T(m) = m * step - d = -1 + (1 - d) + m * step
    return delay == 0.0 ? DAB_Resampler::Params(step_q62) : DAB_Resampler::Params(step_q62, -delay);
}

DAB_Stream_Resampler::DAB_Stream_Resampler(uint64_t step_q62, double delay, double passband_cycles)
    : m_base(stream_params(step_q62, delay)), m_resampler(m_base, passband_cycles) {}

size_t DAB_Stream_Resampler::Admit(tcb::span<const std::complex<float>> in) {
    m_window.insert(m_window.end(), in.begin(), in.end());
    const int64_t end = m_origin + (int64_t)m_window.size();                 // first input index not yet here
    const uint64_t position = m_resampler.Position();
    auto fits = [&](size_t n) {
        int64_t first; uint64_t count;
        check(dabgpu_resample_input_needed(&m_base, position, n, &first, &count), "dabgpu_resample_input_needed");
        return first + (int64_t)count <= end;
    };
    // a guess from the step as a double, then exact: the span of n outputs is monotone in n
    const double step = dabgpu_resample_step(m_base.step_q62);
    const double guess = ((double)end - (double)m_base.offset_samples) / step - (double)position;
    size_t n = guess > 64.0 ? (size_t)(guess - 64.0) : 0;
    if (n > 0 && !fits(n)) { size_t lo = 0; while (n - lo > 1) { const size_t mid = lo + (n - lo) / 2; if (fits(mid)) lo = mid; else n = mid; } n = lo; }
    while (fits(n + 1)) n++;
    return n;
}

void DAB_Stream_Resampler::Retire() {
    int64_t first; uint64_t count;
    check(dabgpu_resample_input_needed(&m_base, m_resampler.Position(), 1, &first, &count), "dabgpu_resample_input_needed");
    if (first > m_origin) {
        const size_t drop = std::min((size_t)(first - m_origin), m_window.size());
        m_window.erase(m_window.begin(), m_window.begin() + (long)drop);
        m_origin += (int64_t)drop;
    }
}

void DAB_Stream_Resampler::Process(tcb::span<const std::complex<float>> in, std::vector<std::complex<float>>& out) {
    const size_t n = Admit(in);
    if (n == 0) return;
    dabgpu_resample_stream now = m_base;
    now.offset_samples = m_base.offset_samples - m_origin;                   // window sample 0 = stream sample m_origin
    m_resampler.SetParams(now);
    const size_t at = out.size();
    out.resize(at + n);
    m_resampler.Apply(tcb::span<std::complex<float>>(out.data() + at, n), m_window, false);
    Retire();
}

void DAB_Stream_Resampler::ProcessU8(tcb::span<const std::complex<float>> in, std::vector<uint8_t>& out, float u8_scale) {
    const size_t n = Admit(in);
    if (n == 0) return;
    dabgpu_resample_stream now = m_base;
    now.offset_samples = m_base.offset_samples - m_origin;
    m_resampler.SetParams(now);
    const size_t at = out.size();
    out.resize(at + 2 * n);
    m_resampler.ApplyU8(tcb::span<uint8_t>(out.data() + at, 2 * n), m_window, false, u8_scale);
    Retire();
}
