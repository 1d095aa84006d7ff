// dabplus_common.h -- what only the DAB+ outer decoder (dabplus.hip) and the super-frame encoder (dabplus_tx.hip) share: the constants of
// RS(120,110) and of the super frame, the fire code's linear map and the access-unit CRC's short units (ETSI TS 102 563 clauses 5.2, 5.3.2,
// 6).  The fire-code table is built at compile time; every translation unit that includes this header holds its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rs_device.h"

namespace dabgpu {

constexpr int RS_N = 120, RS_ROOTS = 10, RS_PAD = 135;
constexpr int RS_DATA = RS_N - RS_ROOTS;
constexpr int DP_MAX_FRAME_BYTES = 1536;                 // 5 n / 120 <= 64 codewords = one per lane
constexpr int DP_MAX_SF = 5 * DP_MAX_FRAME_BYTES;

// fire code x^16+x^14+x^13+x^12+x^11+x^5+x^3+x^2+x+1 over the 72 bits after the check word, zero start value: message bit b (0 = MSB of
// the first byte) contributes x^(16 + 71 - b) mod p(x); the check word is the XOR of the contributions of the set bits
struct FireTab { uint16_t w[72]; };
constexpr FireTab make_fire_tab() {
    FireTab t{};
    unsigned c = 0x782Fu;                                    // x^16 mod p
    for (int p = 0; p < 72; p++) {
        t.w[71 - p] = (uint16_t)c;
        c = (c & 0x8000u) ? (((c << 1) ^ 0x782Fu) & 0xFFFFu) : ((c << 1) & 0xFFFFu);
    }
    return t;
}
static __constant__ FireTab FIRE_TAB = make_fire_tab();

// fire code of the 9 bytes at x, by the whole wavefront: lane l takes message bits l and l + 64; every lane returns the check word
__device__ __forceinline__ uint16_t firecode_wave(const uint8_t* x, int lane) {
    uint32_t v = ((x[lane >> 3] >> (7 - (lane & 7))) & 1) ? FIRE_TAB.w[lane] : 0u;
    if (lane < 8 && ((x[8] >> (7 - lane)) & 1)) v ^= FIRE_TAB.w[64 + lane];
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) v ^= (uint32_t)__shfl_xor((int)v, sft);
    return (uint16_t)v;
}

// CRC of an access unit shared by 1 << lg lanes (crc_lanes).  A unit of one byte or none has no two bytes to fold the start value into: the
// group's last lane starts from the register after it, and no lane has a chunk to run.
template <class F> __device__ __forceinline__ uint16_t au_crc_lanes(F byte_at, int nb_data, const uint16_t* crc_tab, int lg, int q) {
    uint32_t state = 0;
    if (q == (1 << lg) - 1) {
        if (nb_data == 1) state = ((0xFFFFu << 8) ^ crc_tab[(0xFFu ^ byte_at(0)) & 0xFFu]) & 0xFFFFu;
        else if (nb_data < 1) state = 0xFFFFu;
    }
    return crc_lanes(byte_at, (nb_data < 2) ? 0 : nb_data, crc_tab, lg, q, state);
}

}  // namespace dabgpu
