// dab/tx/dab_channel_model.cpp -- see dab_channel_model.h
#include "./dab_channel_model.h"

#include <cmath>
#include <stdexcept>
#include <string>

#include "dab/dabgpu_shared_context.h"
#include "./dabgpu_tx_check.h"

static void check(int st, const char* what) { dabgpu_tx_check("DAB_Channel_Model", st, what); }

DAB_Channel_Model::DAB_Channel_Model(const dabgpu_channel_stream& params) : m_created(params), m_params(params) {
    dabgpu_tx_check_abi("DAB_Channel_Model");
    check(dabgpu_channel_bank_create(dabgpu_shared_context(), 1, &params, &m_bank), "dabgpu_channel_bank_create");
}

DAB_Channel_Model::~DAB_Channel_Model() { dabgpu_channel_bank_destroy(m_bank); }

float DAB_Channel_Model::NoiseSigma(double mean_power, double snr_db) { return (float)std::sqrt(mean_power / (2.0 * std::pow(10.0, snr_db / 10.0))); }

void DAB_Channel_Model::SetParams(const dabgpu_channel_stream& params) {
    dabgpu_channel_fading_stream table;
    if (m_fading) check(dabgpu_channel_fading_plan(&params, &m_spec, 1, &table), "dabgpu_channel_fading_plan");
    check(dabgpu_channel_bank_set_params(m_bank, &params, nullptr), "dabgpu_channel_bank_set_params");
    if (m_fading) check(dabgpu_channel_bank_set_fading(m_bank, &table, nullptr), "dabgpu_channel_bank_set_fading");
    check(dabgpu_synchronize(dabgpu_shared_context(), nullptr), "dabgpu_synchronize");
    m_params = params;
}

void DAB_Channel_Model::SetFading(const dabgpu_channel_fading_spec& spec) {
    dabgpu_channel_fading_stream table;
    check(dabgpu_channel_fading_plan(&m_params, &spec, 1, &table), "dabgpu_channel_fading_plan");
    if (m_fading) {
        check(dabgpu_channel_bank_set_fading(m_bank, &table, nullptr), "dabgpu_channel_bank_set_fading");
    } else {
        // the kernel and the LDS size of a bank are fixed when it is created: a fading bank takes the plain one's place and position
        dabgpu_channel_bank* bank = nullptr;
        check(dabgpu_channel_bank_create_fading(dabgpu_shared_context(), 1, &m_created, &table, &bank), "dabgpu_channel_bank_create_fading");
        dabgpu_channel_bank_destroy(m_bank);
        m_bank = bank;
        check(dabgpu_channel_bank_set_params(m_bank, &m_params, nullptr), "dabgpu_channel_bank_set_params");
        check(dabgpu_channel_bank_set_fading(m_bank, &table, nullptr), "dabgpu_channel_bank_set_fading");
        check(dabgpu_channel_bank_seek(m_bank, m_position, nullptr), "dabgpu_channel_bank_seek");
    }
    check(dabgpu_synchronize(dabgpu_shared_context(), nullptr), "dabgpu_synchronize");
    m_spec = spec;
    m_fading = true;
}

void DAB_Channel_Model::Seek(uint64_t position) {
    check(dabgpu_channel_bank_seek(m_bank, position, nullptr), "dabgpu_channel_bank_seek");
    check(dabgpu_synchronize(dabgpu_shared_context(), nullptr), "dabgpu_synchronize");
    m_position = position;
}

bool DAB_Channel_Model::Apply(tcb::span<std::complex<float>> out, tcb::span<const std::complex<float>> in, bool wrap) {
    if (in.empty()) return false;
    check(dabgpu_channel_bank_apply_host_sync(m_bank, reinterpret_cast<const float*>(in.data()), 0, in.size(), wrap ? 1 : 0, out.size(), out.data(),
                                              DABGPU_IQ_RAW_F32L, 0, 1.0f), "dabgpu_channel_bank_apply_host_sync");
    m_position += out.size();
    return true;
}

bool DAB_Channel_Model::ApplyU8(tcb::span<uint8_t> out, tcb::span<const std::complex<float>> in, bool wrap, float u8_scale) {
    if (in.empty() || (out.size() & 1)) return false;
    check(dabgpu_channel_bank_apply_host_sync(m_bank, reinterpret_cast<const float*>(in.data()), 0, in.size(), wrap ? 1 : 0, out.size() / 2, out.data(),
                                              DABGPU_IQ_RAW_U8, 0, u8_scale), "dabgpu_channel_bank_apply_host_sync");
    m_position += out.size() / 2;
    return true;
}
