// Host model of the channel encoder's kernel (dab-radio_amd/csrc/dab_encode.hip): the same per-item functions (dab_encode_core.h) and
// the same planner, with loops where the kernel has threads.  tests/test_tx_encode_core.py builds it (with sanitizers) and compares
// whole frames with the oracle composition, so the word-parallel arithmetic and the ring bookkeeping are checked without a device.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "dab_encode_core.h"

using namespace dabgpu;

struct tx_model {
    dabgpu_tx_plan plan;
    int n_sub;
    std::vector<uint32_t> ring, prbs;
    uint32_t count;
};

extern "C" {

tx_model* tx_model_create(const dabgpu_subchannel* subs, int n_sub) {
    tx_model* m = new tx_model;
    if (dabgpu_host_tx_plan(subs, n_sub, &m->plan)) { delete m; return nullptr; }
    m->n_sub = n_sub;
    m->ring.assign((size_t)16 * m->plan.ring_slot_dwords, 0);
    m->count = 0;
    dabgpu_vit_tables vt;
    dabgpu_host_fill_vit_tables(&vt);
    m->prbs.assign(TX_PRBS_WORDS, 0);
    for (int j = 0; j < TX_PRBS_WORDS; j++)
        for (int k = 0; k < 4; k++) m->prbs[(size_t)j] |= (uint32_t)vt.prbs[(4 * j + k) % 511] << (8 * k);
    return m;
}
void tx_model_destroy(tx_model* m) { delete m; }
void tx_model_reset(tx_model* m) { std::fill(m->ring.begin(), m->ring.end(), 0u); m->count = 0; }

// fib [F][4][3][30], payload [F][4][cif_in_bytes] (4-byte aligned) -> out [F][28800]
void tx_model_encode(tx_model* m, const uint8_t* fib, const uint8_t* payload, uint32_t F, uint8_t* out) {
    const dabgpu_tx_plan& P = m->plan;
    for (uint32_t f = 0; f < F; f++) {
        uint8_t* o = out + (size_t)f * 28800;
        const uint32_t slot0 = 4u * ((m->count + f) & 3u);
        {   // FIC workgroup
            const dabgpu_tx_sub_plan& S = P.subs[(size_t)m->n_sub];
            uint32_t in[96], cw[288];
            memset(cw, 0, sizeof(cw));
            for (int t = 0; t < 12; t++) {
                const uint8_t* b = fib + ((size_t)f * 12 + t) * 30;
                uint8_t* d = reinterpret_cast<uint8_t*>(in) + 32 * t;
                uint32_t crc = 0xFFFFu;
                for (int k = 0; k < 30; k++) { d[k] = b[k]; crc = tx_crc16_step(crc, b[k]); }
                crc ^= 0xFFFFu;
                d[30] = (uint8_t)(crc >> 8); d[31] = (uint8_t)(crc & 0xFFu);
            }
            for (uint32_t it = 0; it < 4 * (S.n_words + 1); it++)
                tx_encode_word(in + 24 * (it / (S.n_words + 1)), it % (S.n_words + 1), S.n_words, P.sched.data() + S.sched_offset, m->prbs.data(),
                               cw + 72 * (it / (S.n_words + 1)));
            memcpy(o, cw, sizeof(cw));
            for (size_t gi = 0; gi < P.gaps.size() / 2; gi++)
                for (uint32_t q = 0; q < 4; q++) memset(o + 1152 + (size_t)q * 6912 + (size_t)P.gaps[2 * gi] * 8, 0, (size_t)P.gaps[2 * gi + 1] * 8);
        }
        for (int s = 0; s < m->n_sub; s++) {
            const dabgpu_tx_sub_plan& S = P.subs[(size_t)s];
            const uint32_t nblk = S.ring_row_dwords, cw_dwords = 16 * nblk, nw1 = S.n_words + 1;
            std::vector<uint32_t> lds((size_t)4 * cw_dwords, 0);
            uint32_t* ring_e = m->ring.data() + S.ring_offset;
            for (uint32_t it = 0; it < 4 * nw1; it++) {
                const uint32_t q = it / nw1;
                const uint32_t* src = reinterpret_cast<const uint32_t*>(payload + ((size_t)f * 4 + q) * P.cif_in_bytes + S.in_offset);
                tx_encode_word(src, it % nw1, S.n_words, P.sched.data() + S.sched_offset, m->prbs.data(), lds.data() + q * cw_dwords);
            }
            for (uint32_t it = 0; it < 4 * nblk; it++) {
                const uint32_t q = it / nblk, k = it % nblk;
                uint32_t a[16];
                tx_emit_block(ring_e + (size_t)((slot0 + q) & 15u) * P.ring_slot_dwords + k, nblk, lds.data(), cw_dwords, q, k, a);
                const uint32_t nd = std::min(16u, 2u * S.length - 16u * k);
                memcpy(o + 1152 + (size_t)q * 6912 + (size_t)S.start_address * 8 + (size_t)k * 64, a, (size_t)nd * 4);
            }
            for (uint32_t it = 0; it < 4 * nblk; it++) tx_file_block(ring_e, P.ring_slot_dwords, nblk, slot0, lds.data(), cw_dwords, it / nblk, it % nblk);
        }
    }
    m->count += F;
}

}  // extern "C"
