// ofdm/ofdm_modulator.cpp -- see ofdm_modulator.h.  Reference cited: src/ofdm/ofdm_modulator.cpp.
#include "./ofdm_modulator.h"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "dabgpu.h"
#include "dab/dabgpu_shared_context.h"

OFDM_Modulator::OFDM_Modulator(
    const OFDM_Params& params,
    tcb::span<const std::complex<float>> prs_fft_ref)
:   m_params(params),
    m_frame_out_size(params.nb_null_period + params.nb_symbol_period*params.nb_frame_symbols),
    m_data_in_size((params.nb_frame_symbols-1)*params.nb_data_carriers*2/8)
{
    // the kernels exist for the four DAB geometries (src/ofdm/dab_ofdm_params_ref.cpp:11-60)
    for (int mode = 1; mode <= 4 && m_mode == 0; mode++) {
        int g[9];
        if (dabgpu_get_ofdm_params(mode, g) != DABGPU_OK) continue;
        if ((int)params.nb_frame_symbols == g[0] && (int)params.nb_symbol_period == g[1] && (int)params.nb_null_period == g[2] &&
            (int)params.nb_fft == g[3] && (int)params.nb_cyclic_prefix == g[4] && (int)params.nb_data_carriers == g[5]) m_mode = mode;
    }
    if (m_mode == 0) throw std::runtime_error("OFDM_Modulator: the MI355X kernels implement the DAB transmission modes I-IV only");
    if (prs_fft_ref.size() < params.nb_fft) throw std::runtime_error("OFDM_Modulator: PRS reference too small");
    if (dabgpu_abi_version() != DABGPU_ABI_VERSION)
        throw std::runtime_error("OFDM_Modulator: libdabgpu.so implements ABI version " + std::to_string(dabgpu_abi_version()) +
                                 ", this class was built for " + std::to_string(DABGPU_ABI_VERSION));
    m_prs_fft_ref.resize(m_params.nb_fft);
    std::copy_n(prs_fft_ref.begin(), m_params.nb_fft, m_prs_fft_ref.begin());
}

OFDM_Modulator::~OFDM_Modulator() = default;

bool OFDM_Modulator::ProcessBlock(
    tcb::span<std::complex<float>> frame_out_buf,
    tcb::span<const uint8_t> data_in_buf)
{
    // invalid buffer sizes (ofdm_modulator.cpp:54-63)
    if (data_in_buf.size() != m_data_in_size) return false;
    if (frame_out_buf.size() != m_frame_out_size) return false;
    if (!m_tii.empty()) {
        dabgpu_tii_tx list[DABGPU_TII_MAX_TX] = {};
        std::copy(m_tii.begin(), m_tii.end(), list);
        const uint8_t count = (uint8_t)m_tii.size();
        const int st = dabgpu_ofdm_modulate_frames_tii_host_sync(
            dabgpu_shared_context(), m_mode, data_in_buf.data(), DABGPU_TX_PAYLOAD_REFERENCE, 1,
            reinterpret_cast<const float*>(m_prs_fft_ref.data()), 0.0f,
            reinterpret_cast<float*>(frame_out_buf.data()), DABGPU_IQ_RAW_F32L, list, &count);
        if (st != DABGPU_OK)
            throw std::runtime_error(std::string("OFDM_Modulator: dabgpu_ofdm_modulate_frames_tii_host_sync: ") + dabgpu_strerror(st) + " -- " + dabgpu_last_error());
        return true;
    }
    const int st = dabgpu_ofdm_modulate_frames_host_sync(
        dabgpu_shared_context(), m_mode, data_in_buf.data(), DABGPU_TX_PAYLOAD_REFERENCE, 1,
        reinterpret_cast<const float*>(m_prs_fft_ref.data()), 0.0f,
        reinterpret_cast<float*>(frame_out_buf.data()), DABGPU_IQ_RAW_F32L);
    if (st != DABGPU_OK)
        throw std::runtime_error(std::string("OFDM_Modulator: dabgpu_ofdm_modulate_frames_host_sync: ") + dabgpu_strerror(st) + " -- " + dabgpu_last_error());
    return true;
}

void OFDM_Modulator::SetTII(tcb::span<const dabgpu_tii_tx> transmitters)
{
    if (transmitters.empty()) { m_tii.clear(); return; }
    if (m_mode != 1) throw std::runtime_error("OFDM_Modulator: TII is defined for transmission mode I only");
    if (transmitters.size() > DABGPU_TII_MAX_TX) throw std::runtime_error("OFDM_Modulator: " + std::to_string(transmitters.size()) + " transmitters (at most 4)");
    dabgpu_tii_tx list[DABGPU_TII_MAX_TX] = {};
    std::copy(transmitters.begin(), transmitters.end(), list);
    const uint8_t count = (uint8_t)transmitters.size();
    const int st = dabgpu_tii_validate(list, &count, 1);
    if (st != DABGPU_OK) throw std::runtime_error(std::string("OFDM_Modulator: dabgpu_tii_validate: ") + dabgpu_strerror(st) + " -- " + dabgpu_last_error());
    m_tii.assign(transmitters.begin(), transmitters.end());
}
