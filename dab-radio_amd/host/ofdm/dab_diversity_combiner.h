// ofdm/dab_diversity_combiner.h -- receive diversity behind K mode I demodulators (include/dabgpu.h, "Receive diversity"): the DQPSK products
// of the branches' frames (OFDM_Demod::GetFrameDataVec() under SetSoftDecision(DABGPU_SOFT_CSI, L), one level for all) and their scales
// (OFDM_Demod::GetSoftScale()) become one frame of soft bits for the decoders.  The reference has no such stage; the class follows the
// conventions of the other added classes: spans in, false for wrong sizes, exceptions for device failures.  Pairing the frames of the
// branches (which frame of receiver A is which of receiver B) is the caller's.
#pragma once
#include <complex>
#include <cstdint>
#include <vector>

#include "dabgpu.h"
#include "utility/span.h"
#include "viterbi_config.h"

struct dabgpu_ctx;

class DAB_Diversity_Combiner {
public:
    explicit DAB_Diversity_Combiner(int nb_branches);       // 1 .. DABGPU_DIVERSITY_MAX_BRANCHES, else std::invalid_argument
    int GetTotalBranches() const { return m_nb_branches; }
    // products[b]: the 75 x 1536 products of branch b's frame (an empty span: the branch has no frame, it is dead); scales[b] its k;
    // weights: empty (every weight 1) or one per branch, 1 / noise power for maximal-ratio combining; out_bits: 230400 soft bits,
    // DABGPU_BITS_NATURAL unless SetBitsLayout says otherwise.  false for wrong sizes.
    bool Combine(tcb::span<const tcb::span<const std::complex<float>>> products, tcb::span<const float> scales, tcb::span<const float> weights,
                 tcb::span<viterbi_bit_t> out_bits);
    // the same with band weights (include/dabgpu.h, "Banded receive diversity"): band_weights[b] = the 128 band weights of branch b's frame
    // (DAB_Noise_Profile::Update's) or an empty span for a branch without a table, which then takes weights[b] (1 without weights); for a
    // branch with a table weights[b] is not looked at.  false for wrong sizes.
    bool Combine(tcb::span<const tcb::span<const std::complex<float>>> products, tcb::span<const float> scales, tcb::span<const float> weights,
                 tcb::span<const tcb::span<const float>> band_weights, tcb::span<viterbi_bit_t> out_bits);
    // the same with symbol weights on top (include/dabgpu.h, "Symbol-weighted receive diversity"): symbol_weights[b] = the 75 symbol
    // weights of branch b's frame (DAB_Symbol_Profile::Update's) or an empty span for a branch without them; band_weights as above, or an
    // empty span of spans for no band table at all.  false for wrong sizes.
    bool Combine(tcb::span<const tcb::span<const std::complex<float>>> products, tcb::span<const float> scales, tcb::span<const float> weights,
                 tcb::span<const tcb::span<const float>> band_weights, tcb::span<const tcb::span<const float>> symbol_weights,
                 tcb::span<viterbi_bit_t> out_bits);
    void SetBitsLayout(int bits_layout) { m_layout = bits_layout; }
    float GetScale() const { return m_scale; }              // k of the last frame combined (0: erased)
    uint32_t GetLiveMask() const { return m_live_mask; }    // bit b: branch b took part in it

private:
    using Tables = tcb::span<const tcb::span<const float>>;
    // the body of the three overloads; a null table: the overload has none, and the narrower entry point is the one called
    bool CombineTables(tcb::span<const tcb::span<const std::complex<float>>> products, tcb::span<const float> scales, tcb::span<const float> weights,
                       const Tables* band_weights, const Tables* symbol_weights, tcb::span<viterbi_bit_t> out_bits);
    dabgpu_ctx* m_ctx;
    int m_nb_branches;
    int m_layout = DABGPU_BITS_NATURAL;
    float m_scale = 0.0f;
    uint32_t m_live_mask = 0;
};
