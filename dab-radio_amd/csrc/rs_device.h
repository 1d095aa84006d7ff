// rs_device.h -- what the kernels of dabplus.hip, dabplus_tx.hip and packet_fec.hip share beyond rs_core.h: the GF(2^8) tables in constant
// memory (a copy per translation unit), their copy into LDS beside the CRC-16 table, and the CRC of a byte run shared by 2^lg lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rs_core.h"

namespace dabgpu {

static __constant__ rs::GfTables GF_TABLES = rs::make_gf();

// L.crc_tab (x^16+x^12+x^5+1, MSB first) alone (dabplus.hip lends its place away), and with L.exp and L.log; the caller synchronises
template <class T> __device__ __forceinline__ void load_crc_table(T& L, int lane) {
    for (int k = lane; k < 256; k += 64) L.crc_tab[k] = rs::crc16_entry(k);
}
template <class T> __device__ __forceinline__ void load_gf_crc_tables(T& L, int lane) {
    for (int k = lane; k < 512; k += 64) L.exp[k] = GF_TABLES.exp[k];
    for (int k = lane; k < 256; k += 64) { L.log[k] = GF_TABLES.log[k]; L.crc_tab[k] = rs::crc16_entry(k); }
}

// a(x) b(x) mod x^16+x^12+x^5+1 (16-bit residues)
__device__ __forceinline__ uint32_t crc_mulmod(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        r ^= (0u - ((b >> i) & 1u)) & a;
        a = (a << 1) ^ ((0u - ((a >> 15) & 1u)) & 0x11021u);
    }
    return r;
}

// CRC (start value 0xFFFF, inverted) of the bytes byte_at(0..nb_data-1) shared by per = 1 << lg lanes, this one lane q of them; lane per - 1
// returns it.  With the start value folded into the first two bytes the register is linear in the message: the run is padded at the FRONT
// with zero bytes to per x c, lane q runs chunk q from a zero register (and x^(8c) beside it), and the chunks are joined pairwise in lg rounds
// of shuffles.  nb_data is 2 or more -- or none (<= 0): only the shuffles, over the `state` each lane brings (au_crc_lanes' short units).
template <class F> __device__ __forceinline__ uint16_t crc_lanes(F byte_at, int nb_data, const uint16_t* crc_tab, int lg, int q, uint32_t state = 0) {
    const int per = 1 << lg;
    uint32_t m = 1;
    if (nb_data > 0) {
        const int c = (nb_data + per - 1) >> lg, z = per * c - nb_data;
        for (int t = 0, k = q * c - z; t < c; t++, k++) {
            uint32_t byte = (k >= 0) ? byte_at(k) : 0u;
            if (k == 0 || k == 1) byte ^= 0xFFu;
            state = ((state << 8) ^ crc_tab[((state >> 8) ^ byte) & 0xFFu]) & 0xFFFFu;
            m = ((m << 8) ^ crc_tab[(m >> 8) & 0xFFu]) & 0xFFFFu;
        }
    }
#pragma unroll
    for (int d = 1; d < per; d <<= 1) {
        const uint32_t left = (uint32_t)__shfl_xor((int)state, d);
        if (q & d) state ^= crc_mulmod(left, m);
        m = crc_mulmod(m, m);
    }
    return (uint16_t)(state ^ 0xFFFFu);
}

}  // namespace dabgpu
