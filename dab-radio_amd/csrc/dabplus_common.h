// dabplus_common.h -- what the DAB+ outer decoder (dabplus.hip) and the super-frame encoder (dabplus_tx.hip) share: the GF(2^8) tables of
// RS(120,110), the fire code's and the access-unit CRC's linear maps (ETSI TS 102 563 clauses 5.2, 5.3.2, 6).  Tables are built at compile
// time; every translation unit that includes this header holds its own copy in constant memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dabgpu {

constexpr int RS_N = 120, RS_ROOTS = 10, RS_PAD = 135;
constexpr int RS_DATA = RS_N - RS_ROOTS;
constexpr int DP_MAX_FRAME_BYTES = 1536;                 // 5 n / 120 <= 64 codewords = one per lane
constexpr int DP_MAX_SF = 5 * DP_MAX_FRAME_BYTES;

struct GfTables { uint8_t exp[512]; uint8_t log[256]; };
constexpr GfTables make_gf() {
    GfTables t{};
    unsigned x = 1;
    for (int i = 0; i < 255; i++) {
        t.exp[i] = (uint8_t)x; t.exp[i + 255] = (uint8_t)x; t.log[x] = (uint8_t)i;
        x <<= 1;
        if (x & 0x100u) x ^= 0x11Du;
    }
    t.exp[510] = t.exp[0]; t.exp[511] = t.exp[1];
    t.log[0] = 0;
    return t;
}
static __constant__ GfTables GF_TABLES = make_gf();

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

}  // namespace dabgpu
