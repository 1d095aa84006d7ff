// ofdm/dab_symbol_profile.h -- the symbol noise profile of one mode I receiver (include/dabgpu.h, "Symbol noise profile"): every frame's
// own DQPSK products become one noise figure per product row and the rows' relative weights against the frame's median, which is what
// DAB_Diversity_Combiner::Combine takes as a branch's symbol weights.  It answers wideband bursts that last a symbol or longer, which
// the blanker, DAB_Noise_Profile and DAB_DD_Profile cannot.  The reference has no such stage; the class follows the conventions of the
// other added classes: spans in, false for wrong sizes, exceptions for device failures.  The estimator keeps no state from frame to
// frame; the object only remembers the last frame's figures.
#pragma once
#include <array>
#include <complex>
#include <cstdint>

#include "dabgpu.h"
#include "utility/span.h"

struct dabgpu_ctx;

class DAB_Symbol_Profile {
public:
    static constexpr size_t NB_SYMBOLS = DABGPU_SYM_PROFILE_SYMBOLS;
    static constexpr size_t NB_PRODUCTS = NB_SYMBOLS * 1536;    // one frame's products, symbol after symbol in carrier order
    DAB_Symbol_Profile();
    // products: the frame's NB_PRODUCTS products (OFDM_Demod's DQPSK view, a branch's d_dqpsk).  false for a span of another size.
    // true: out_weights holds the 75 symbol weights -- all zero, with IsValid() false, for a frame without a usable measurement.
    bool Update(tcb::span<const std::complex<float>> products, tcb::span<float> out_weights);
    bool IsValid() const { return m_valid; }                // of the last Update
    float GetRefNoise() const { return m_ref; }             // q_ref of the last Update (0: skipped)
    tcb::span<const float> GetSymbolNoise() const { return {m_noise.data(), m_noise.size()}; }     // q of the last Update

private:
    dabgpu_ctx* m_ctx;
    std::array<float, NB_SYMBOLS> m_noise{};
    bool m_valid = false;
    float m_ref = 0.0f;
};
