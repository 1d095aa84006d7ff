// dab_encode_core.h -- the word-parallel arithmetic of the channel encoder (dab_encode.hip), host and device: 32 input bits at a time
// through energy dispersal, the K = 7 rate-1/4 code and a puncturing run, and the 16-way bit transpose between a CIF's natural bit
// order and the time interleaver's class order.  Plain C++ so that tests/test_tx_encode_core.py can run the same functions on the CPU
// against the oracle.  Bit streams are LSB first: bit k of a stream is bit k % 32 of dword k / 32, which is the frame-bit layout of
// DABGPU_TX_PAYLOAD_FRAME_BITS.
#pragma once
#include <stdint.h>

#include "dabgpu_host_logic.h"

namespace dabgpu {

// four data bytes as loaded (byte 0 lowest, each byte MSB first on the air) -> bit j = input bit j
DABGPU_HD inline uint32_t tx_info_word(uint32_t x) {
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    return ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
}

// EN 300 401 11.1.1: x0 = a_i + a_{i-2} + a_{i-3} + a_{i-5} + a_{i-6}, x1 = a_i + a_{i-1} + a_{i-2} + a_{i-3} + a_{i-6},
// x2 = a_i + a_{i-1} + a_{i-4} + a_{i-6}, x3 = x0 for the 32 input bits of `cur`; `prev` = the 32 bits before them (0 at the start)
DABGPU_HD inline void tx_generators(uint32_t prev, uint32_t cur, uint32_t g[3]) {
    const uint64_t w = ((uint64_t)cur << 32) | prev;
    const uint32_t d1 = (uint32_t)(w >> 31), d2 = (uint32_t)(w >> 30), d3 = (uint32_t)(w >> 29), d4 = (uint32_t)(w >> 28),
                   d5 = (uint32_t)(w >> 27), d6 = (uint32_t)(w >> 26);
    g[0] = cur ^ d2 ^ d3 ^ d5 ^ d6;
    g[1] = cur ^ d1 ^ d2 ^ d3 ^ d6;
    g[2] = cur ^ d1 ^ d4 ^ d6;
}

// bit j of the low byte -> bit 4 j
DABGPU_HD inline uint32_t tx_spread8(uint32_t x) {
    x &= 0xFFu;
    x = (x | (x << 12)) & 0x000F000Fu;
    x = (x | (x << 6)) & 0x03030303u;
    return (x | (x << 3)) & 0x11111111u;
}

// run p (0..3) of a word's mother code: 8 input bits x 4 outputs, bit 4 j + r = output r of input bit 8 p + j
DABGPU_HD inline uint32_t tx_mother_run(const uint32_t g[3], int p) {
    const uint32_t s0 = tx_spread8(g[0] >> (8 * p));
    return s0 | (tx_spread8(g[1] >> (8 * p)) << 1) | (tx_spread8(g[2] >> (8 * p)) << 2) | (s0 << 3);
}

// the kept bits of a run, packed from bit 0 (keep_mask keeps the first outputs of every input bit: dabgpu_tx_sched_entry)
DABGPU_HD inline uint32_t tx_puncture_run(uint32_t mother, uint32_t keep_mask) {
    const uint32_t m = mother & keep_mask;
    uint32_t out = 0, pos = 0;
#pragma unroll
    for (int g = 0; g < 8; g++) {
        out |= ((m >> (4 * g)) & 15u) << pos;
        pos += (uint32_t)__builtin_popcount((keep_mask >> (4 * g)) & 15u);
    }
    return out;
}

// a[m] = two rows of 16 bits (low and high half): both 16 x 16 bit matrices transposed in place (its own inverse)
DABGPU_HD inline void tx_transpose16(uint32_t a[16]) {
    uint32_t mask = 0x00FF00FFu;
#pragma unroll
    for (int s = 8; s; s >>= 1) {
#pragma unroll
        for (int k = 0; k < 16; k++) {
            if (k & s) continue;
            const uint32_t t = ((a[k] >> s) ^ a[k + s]) & mask;
            a[k + s] ^= t;
            a[k] ^= t << s;
        }
        mask ^= mask << (s >> 1);
    }
}

// 512 consecutive bits of a CIF in natural order (16 dwords) -> their 16 class dwords: class c = bits 16 j + c, j = 0..31
DABGPU_HD inline void tx_natural_to_classes(uint32_t a[16]) {
    uint32_t b[16];
#pragma unroll
    for (int m = 0; m < 16; m++) b[m] = ((a[m >> 1] >> (16 * (m & 1))) & 0xFFFFu) | (((a[8 + (m >> 1)] >> (16 * (m & 1))) & 0xFFFFu) << 16);
    tx_transpose16(b);
#pragma unroll
    for (int m = 0; m < 16; m++) a[m] = b[m];
}
// and back
DABGPU_HD inline void tx_classes_to_natural(uint32_t a[16]) {
    tx_transpose16(a);
    uint32_t b[16];
#pragma unroll
    for (int m = 0; m < 8; m++) {
        b[m] = (a[2 * m] & 0xFFFFu) | (a[2 * m + 1] << 16);
        b[8 + m] = (a[2 * m] >> 16) | (a[2 * m + 1] & 0xFFFF0000u);
    }
#pragma unroll
    for (int m = 0; m < 16; m++) a[m] = b[m];
}

// EN 300 401 12: bits of class c = i % 16 are sent TX_CIF_DELAY[c] CIFs late; class TX_DELAY_CLASS[d] has delay d (a 4-bit reversal)
DABGPU_HD inline uint32_t tx_cif_delay(uint32_t c) { return ((c & 1u) << 3) | ((c & 2u) << 1) | ((c & 4u) >> 1) | ((c & 8u) >> 3); }

// EN 300 401 5.2.1: CRC16 of a FIB body (x^16 + x^12 + x^5 + 1, register preset to ones, result complemented)
DABGPU_HD inline uint32_t tx_crc16_step(uint32_t crc, uint32_t byte) {
    crc ^= byte << 8;
#pragma unroll
    for (int j = 0; j < 8; j++) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x1021u) & 0xFFFFu : (crc << 1) & 0xFFFFu;
    return crc;
}

#if defined(__HIP_DEVICE_COMPILE__)
#define DABGPU_TX_OR(p, v) atomicOr((p), (v))        // threads of a workgroup deposit into one LDS code word
#else
#define DABGPU_TX_OR(p, v) (*(p) |= (v))
#endif
#define TX_PRBS_WORDS 511                                   // the energy-dispersal sequence has period 511 bits: 511 dwords hold it 32 times

// word w of a code word (w == n_words: the tail): src = its input dwords, cw = its bits in LDS (zeroed)
DABGPU_HD inline void tx_encode_word(const uint32_t* src, uint32_t w, uint32_t n_words, const dabgpu_tx_sched_entry* sch, const uint32_t* prbs,
                                      uint32_t* cw) {
    const dabgpu_tx_sched_entry e = sch[w];
    const uint32_t cur = w < n_words ? tx_info_word(src[w] ^ prbs[w % TX_PRBS_WORDS]) : 0u;
    const uint32_t prev = w > 0 ? tx_info_word(src[w - 1] ^ prbs[(w - 1) % TX_PRBS_WORDS]) : 0u;
    uint32_t g[3];
    tx_generators(prev, cur, g);
    const uint32_t per_run = (uint32_t)__builtin_popcount(e.keep_mask);
    const int runs = w < n_words ? 4 : 1;
    for (int p = 0; p < runs; p++) {
        const uint32_t bit = e.out_bit + (uint32_t)p * per_run;
        const uint64_t v = (uint64_t)tx_puncture_run(tx_mother_run(g, p), e.keep_mask) << (bit & 31u);
        DABGPU_TX_OR(&cw[bit >> 5], (uint32_t)v);
        if (v >> 32) DABGPU_TX_OR(&cw[(bit >> 5) + 1], (uint32_t)(v >> 32));
    }
}


// transmitted CIF q (0..3) of a frame, block k (512 bits) of a sub-channel: `row` = class row 0, dword k of the CIF's ring slot (rows
// row_stride dwords apart), lds = the frame's four logical frames in natural order (cw_dwords each); classes whose delay stays inside
// the frame come from lds.  a[] = the block's 16 dwords in natural order.
DABGPU_HD inline void tx_emit_block(const uint32_t* row, uint32_t row_stride, const uint32_t* lds, uint32_t cw_dwords, uint32_t q, uint32_t k,
                                    uint32_t a[16]) {
#pragma unroll
    for (int c = 0; c < 16; c++) a[c] = row[(uint32_t)c * row_stride];
    tx_classes_to_natural(a);
#pragma unroll
    for (uint32_t d = 0; d < 4; d++) {
        if (d > q) continue;
        const uint32_t m = 0x00010001u << tx_cif_delay(d);          // the class with delay d, in both halves of a dword
        const uint32_t* fresh = lds + (q - d) * cw_dwords + 16 * k;
#pragma unroll
        for (int j = 0; j < 16; j++) a[j] = (a[j] & ~m) | (fresh[j] & m);
    }
}

// logical frame q, block k: class c's dword goes to the slot of CIF q + delay(c) unless that CIF belongs to this frame (emitted already).
// ring = the sub-channel's rows in slot 0 of its ensemble, slot0 = slot of the frame's first CIF
DABGPU_HD inline void tx_file_block(uint32_t* ring, uint32_t ring_slot_dwords, uint32_t row_stride, uint32_t slot0, const uint32_t* lds,
                                    uint32_t cw_dwords, uint32_t q, uint32_t k) {
    const uint32_t* fresh = lds + q * cw_dwords + 16 * k;
    uint32_t a[16];
#pragma unroll
    for (int j = 0; j < 16; j++) a[j] = fresh[j];
    tx_natural_to_classes(a);
#pragma unroll
    for (uint32_t c = 0; c < 16; c++) {
        const uint32_t d = tx_cif_delay(c);
        if (q + d > 3u) ring[(size_t)((slot0 + q + d) & 15u) * ring_slot_dwords + c * row_stride + k] = a[c];
    }
}

}  // namespace dabgpu
