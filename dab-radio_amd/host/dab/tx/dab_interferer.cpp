// dab/tx/dab_interferer.cpp -- see dab_interferer.h
#include "./dab_interferer.h"

#include <cmath>

#include "dab/dabgpu_shared_context.h"
#include "./dabgpu_tx_check.h"

static void check(int st, const char* what) { dabgpu_tx_check("DAB_Interferer", st, what); }

DAB_Interferer::DAB_Interferer(const dabgpu_interferer_stream& params, tcb::span<const dabgpu_interferer_shape> shapes) {
    dabgpu_tx_check_abi("DAB_Interferer");
    check(dabgpu_interferer_bank_create(dabgpu_shared_context(), 1, &params, shapes.empty() ? nullptr : shapes.data(), (int)shapes.size(), &m_bank),
          "dabgpu_interferer_bank_create");
}

DAB_Interferer::~DAB_Interferer() { dabgpu_interferer_bank_destroy(m_bank); }

float DAB_Interferer::Amplitude(double signal_power, double is_db) { return (float)std::sqrt(signal_power * std::pow(10.0, is_db / 10.0)); }

dabgpu_interferer_shape DAB_Interferer::Shape(double width_hz) {
    dabgpu_interferer_shape H;
    check(dabgpu_interferer_design(width_hz / 2.048e6, &H), "dabgpu_interferer_design");
    return H;
}

void DAB_Interferer::SetParams(const dabgpu_interferer_stream& params) {
    check(dabgpu_interferer_bank_set_params(m_bank, &params, nullptr), "dabgpu_interferer_bank_set_params");
    check(dabgpu_synchronize(dabgpu_shared_context(), nullptr), "dabgpu_synchronize");
}

void DAB_Interferer::Seek(uint64_t position) {
    check(dabgpu_interferer_bank_seek(m_bank, position, nullptr), "dabgpu_interferer_bank_seek");
    check(dabgpu_synchronize(dabgpu_shared_context(), nullptr), "dabgpu_synchronize");
}

bool DAB_Interferer::Apply(tcb::span<std::complex<float>> out, tcb::span<const std::complex<float>> in) {
    if (!in.empty() && in.size() != out.size()) return false;
    check(dabgpu_interferer_bank_apply_host_sync(m_bank, in.empty() ? nullptr : reinterpret_cast<const float*>(in.data()), 0, out.size(), out.data(),
                                                 DABGPU_IQ_RAW_F32L, 0, 1.0f), "dabgpu_interferer_bank_apply_host_sync");
    return true;
}

bool DAB_Interferer::ApplyU8(tcb::span<uint8_t> out, tcb::span<const std::complex<float>> in, float u8_scale) {
    if ((out.size() & 1) || (!in.empty() && in.size() != out.size() / 2)) return false;
    check(dabgpu_interferer_bank_apply_host_sync(m_bank, in.empty() ? nullptr : reinterpret_cast<const float*>(in.data()), 0, out.size() / 2, out.data(),
                                                 DABGPU_IQ_RAW_U8, 0, u8_scale), "dabgpu_interferer_bank_apply_host_sync");
    return true;
}
