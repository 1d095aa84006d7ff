// ofdm/dab_diversity_combiner.cpp -- over dabgpu_diversity_combine_host_sync, dabgpu_diversity_combine_banded_host_sync and
// dabgpu_diversity_combine_symbols_host_sync: one body, each overload its own entry point
#include "./dab_diversity_combiner.h"

#include <stdexcept>
#include <string>

#include "../dab/dabgpu_shared_context.h"

DAB_Diversity_Combiner::DAB_Diversity_Combiner(int nb_branches) : m_ctx(dabgpu_shared_context()), m_nb_branches(nb_branches) {
    if (nb_branches < 1 || nb_branches > DABGPU_DIVERSITY_MAX_BRANCHES) throw std::invalid_argument("DAB_Diversity_Combiner: 1 .. 8 branches");
}

bool DAB_Diversity_Combiner::Combine(tcb::span<const tcb::span<const std::complex<float>>> products, tcb::span<const float> scales,
                                     tcb::span<const float> weights, tcb::span<viterbi_bit_t> out_bits) {
    return CombineTables(products, scales, weights, nullptr, nullptr, out_bits);
}

bool DAB_Diversity_Combiner::Combine(tcb::span<const tcb::span<const std::complex<float>>> products, tcb::span<const float> scales,
                                     tcb::span<const float> weights, tcb::span<const tcb::span<const float>> band_weights,
                                     tcb::span<viterbi_bit_t> out_bits) {
    if (band_weights.size() != (size_t)m_nb_branches) return false;
    return CombineTables(products, scales, weights, &band_weights, nullptr, out_bits);
}

bool DAB_Diversity_Combiner::Combine(tcb::span<const tcb::span<const std::complex<float>>> products, tcb::span<const float> scales,
                                     tcb::span<const float> weights, tcb::span<const tcb::span<const float>> band_weights,
                                     tcb::span<const tcb::span<const float>> symbol_weights, tcb::span<viterbi_bit_t> out_bits) {
    if (symbol_weights.size() != (size_t)m_nb_branches) return false;
    return CombineTables(products, scales, weights, &band_weights, &symbol_weights, out_bits);
}

// band_weights / symbol_weights null: the overload has no such argument, and the call is the narrower entry point's.  Given, a table is
// empty (the three-table overload's band_weights only: no band array at all) or has one span per branch
bool DAB_Diversity_Combiner::CombineTables(tcb::span<const tcb::span<const std::complex<float>>> products, tcb::span<const float> scales,
                                           tcb::span<const float> weights, const Tables* band_weights, const Tables* symbol_weights,
                                           tcb::span<viterbi_bit_t> out_bits) {
    const size_t n = (size_t)m_nb_branches, frame = (size_t)(DABGPU_NB_FRAME_SYMBOLS - 1) * DABGPU_NB_DATA_CARRIERS;
    const bool banded = band_weights && !band_weights->empty();
    if (products.size() != n || scales.size() != n || (!weights.empty() && weights.size() != n) || (banded && band_weights->size() != n) ||
        out_bits.size() != DABGPU_NB_FRAME_BITS)
        return false;
    const float *ptr[DABGPU_DIVERSITY_MAX_BRANCHES], *band[DABGPU_DIVERSITY_MAX_BRANCHES], *sym[DABGPU_DIVERSITY_MAX_BRANCHES];
    int valid[DABGPU_DIVERSITY_MAX_BRANCHES];
    for (size_t b = 0; b < n; b++) {
        if (!products[b].empty() && products[b].size() != frame) return false;
        if (banded && !(*band_weights)[b].empty() && (*band_weights)[b].size() != DABGPU_NOISE_PROFILE_BANDS) return false;
        if (symbol_weights && !(*symbol_weights)[b].empty() && (*symbol_weights)[b].size() != DABGPU_SYM_PROFILE_SYMBOLS) return false;
        valid[b] = products[b].empty() ? 0 : 1;
        ptr[b] = products[b].empty() ? nullptr : reinterpret_cast<const float*>(products[b].data());
        band[b] = (!banded || (*band_weights)[b].empty()) ? nullptr : (*band_weights)[b].data();
        sym[b] = (!symbol_weights || (*symbol_weights)[b].empty()) ? nullptr : (*symbol_weights)[b].data();
    }
    const float* const w = weights.empty() ? nullptr : weights.data();
    const int st = symbol_weights ? dabgpu_diversity_combine_symbols_host_sync(m_ctx, ptr, scales.data(), w, valid, m_nb_branches, m_layout, out_bits.data(),
                                                                               &m_scale, &m_live_mask, banded ? band : nullptr, sym)
                   : band_weights ? dabgpu_diversity_combine_banded_host_sync(m_ctx, ptr, scales.data(), w, valid, m_nb_branches, m_layout, out_bits.data(),
                                                                              &m_scale, &m_live_mask, band)
                                  : dabgpu_diversity_combine_host_sync(m_ctx, ptr, scales.data(), w, valid, m_nb_branches, m_layout, out_bits.data(), &m_scale,
                                                                       &m_live_mask);
    if (st != DABGPU_OK) throw std::runtime_error(std::string("DAB_Diversity_Combiner: ") + dabgpu_strerror(st) + " -- " + dabgpu_last_error());
    return true;
}
