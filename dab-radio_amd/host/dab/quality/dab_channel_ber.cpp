// dab/quality/dab_channel_ber.cpp -- over dabgpu_ber_fib_group_host_sync / dabgpu_ber_codeword_host_sync
#include "./dab_channel_ber.h"

#include <stdexcept>
#include <string>

#include "../dabgpu_shared_context.h"

DAB_Channel_BER::DAB_Channel_BER() : m_ctx(dabgpu_shared_context()) {}

void DAB_Channel_BER::Add(int status, const dabgpu_ber_result& r) {
    if (status != DABGPU_OK) throw std::runtime_error(std::string("DAB_Channel_BER: ") + dabgpu_strerror(status) + " -- " + dabgpu_last_error());
    m_bits += r.n_bits;
    m_errors += r.n_errors;
}

bool DAB_Channel_BER::MeasureFIBGroup(tcb::span<const viterbi_bit_t> encoded_bits, tcb::span<const uint8_t> decoded_bytes, dabgpu_ber_result& out) {
    if (encoded_bits.size() != DABGPU_NB_FIB_GROUP_BITS || decoded_bytes.size() != 96) return false;
    Add(dabgpu_ber_fib_group_host_sync(m_ctx, encoded_bits.data(), decoded_bytes.data(), &out), out);
    return true;
}

bool DAB_Channel_BER::MeasureSubchannel(const dabgpu_subchannel& subchannel, tcb::span<const viterbi_bit_t> deinterleaved_bits,
                                        tcb::span<const uint8_t> decoded_bytes, dabgpu_ber_result& out) {
    int pi[4], lx[4], nb = 0;
    if (dabgpu_subchannel_validate(&subchannel) != DABGPU_OK || dabgpu_subchannel_plan(&subchannel, pi, lx, &nb) < 0) return false;
    if (deinterleaved_bits.size() != (size_t)subchannel.length * 64 || decoded_bytes.size() != (size_t)nb) return false;
    Add(dabgpu_ber_codeword_host_sync(m_ctx, &subchannel, deinterleaved_bits.data(), decoded_bytes.data(), &out), out);
    return true;
}
