// ofdm/dab_symbol_profile.cpp -- over dabgpu_sym_profile_host_sync
#include "./dab_symbol_profile.h"

#include <stdexcept>
#include <string>

#include "../dab/dabgpu_shared_context.h"

DAB_Symbol_Profile::DAB_Symbol_Profile() : m_ctx(dabgpu_shared_context()) {}

bool DAB_Symbol_Profile::Update(tcb::span<const std::complex<float>> products, tcb::span<float> out_weights) {
    if (products.size() != NB_PRODUCTS || out_weights.size() != NB_SYMBOLS) return false;
    uint32_t valid = 0;
    const int st = dabgpu_sym_profile_host_sync(m_ctx, reinterpret_cast<const float*>(products.data()), out_weights.data(), m_noise.data(), &m_ref, &valid);
    if (st != DABGPU_OK) throw std::runtime_error(std::string("DAB_Symbol_Profile: ") + dabgpu_strerror(st) + " -- " + dabgpu_last_error());
    m_valid = valid != 0;
    return true;
}
