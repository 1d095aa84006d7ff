// rs_core.h -- the Reed-Solomon arithmetic that the DAB+ outer code (dabplus.hip, dabplus_tx.hip: RS(120,110), ETSI TS 102 563 clause 6) and
// packet-mode FEC (packet_fec.hip: RS(204,188), EN 300 401 clause 5.3.5) share with the host tests (tests/cpp/rs_core_host.cpp): GF(2^8) with
// p(x) = x^8+x^4+x^3+x^2+1, first root alpha^0, Berlekamp-Massey / Chien / Forney as the reference's one decoder class has them
// (src/dab/algorithms/reed_solomon_decoder.cpp), the systematic encoder as a linear map, and the CRC-16 table's entries.  A code is its
// template arguments: N symbols, ROOTS parity symbols, shortened by PAD = 255 - N.  The field is "anything with .exp[512] and .log[256]",
// polynomials are "anything indexable": register arrays, LDS rows, host arrays.  Loops have fixed trip counts with guards, so that arrays
// the caller keeps in registers are only indexed by constants.  Plain C++, no HIP headers, no tables in memory.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RS_HD __host__ __device__ __forceinline__
#define RS_UNROLL _Pragma("unroll")
#else
#define RS_HD inline
#define RS_UNROLL
#endif

namespace dabgpu {
namespace rs {

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

template <class T> RS_HD uint8_t mul(const T& L, uint8_t a, uint8_t b) { return (a && b) ? L.exp[L.log[a] + L.log[b]] : (uint8_t)0; }
template <class T> RS_HD uint8_t div(const T& L, uint8_t a, uint8_t b) { return a ? L.exp[L.log[a] + 255 - L.log[b]] : (uint8_t)0; }
template <class T> RS_HD uint8_t pow(const T& L, int e) { e %= 255; if (e < 0) e += 255; return L.exp[e]; }

// entry k of the table of CRC-16 x^16+x^12+x^5+1, MSB first
constexpr uint16_t crc16_entry(int k) {
    uint16_t c = (uint16_t)(k << 8);
    for (int j = 0; j < 8; j++) c = (c & 0x8000u) ? (uint16_t)((c << 1) ^ 0x1021u) : (uint16_t)(c << 1);
    return c;
}

// ---- encoder ----
// row j = logarithms of the ROOTS coefficients of x^(N - 1 - j) mod g(x), highest power first (= parity byte order), g(x) = prod (x + alpha^r),
// r = 0..ROOTS-1; 16 bytes per row for one aligned read.  A zero coefficient has no logarithm: it is marked in `zero` (bit r).
template <int N_DATA, int ROOTS> struct ParityTab {
    static_assert(ROOTS <= 16, "a row is 16 bytes");
    alignas(16) uint8_t log_coef[N_DATA][16];
    uint16_t zero[N_DATA];
    bool all_nonzero;
};
template <int N_DATA, int ROOTS> constexpr ParityTab<N_DATA, ROOTS> make_parity_tab() {
    const GfTables gf = make_gf();
    auto m = [&](unsigned a, unsigned b) -> unsigned { return (a && b) ? gf.exp[gf.log[a] + gf.log[b]] : 0u; };
    unsigned g[ROOTS + 1] = {1};                             // ascending powers
    for (int r = 0; r < ROOTS; r++) {
        for (int k = r + 1; k > 0; k--) g[k] = g[k - 1] ^ m(g[k], gf.exp[r]);
        g[0] = m(g[0], gf.exp[r]);
    }
    ParityTab<N_DATA, ROOTS> t{};
    t.all_nonzero = true;
    unsigned rem[ROOTS] = {};                                // x^e mod g(x), ascending powers; e = ROOTS first
    for (int k = 0; k < ROOTS; k++) rem[k] = g[k];           // x^ROOTS = g(x) - x^ROOTS = the lower coefficients (characteristic 2)
    for (int j = N_DATA - 1; j >= 0; j--) {                  // e = N - 1 - j
        t.zero[j] = 0;
        for (int r = 0; r < ROOTS; r++) {
            t.log_coef[j][r] = gf.log[rem[ROOTS - 1 - r]];
            if (rem[ROOTS - 1 - r] == 0) { t.zero[j] |= (uint16_t)(1u << r); t.all_nonzero = false; }
        }
        const unsigned top = rem[ROOTS - 1];                 // times x
        for (int k = ROOTS - 1; k > 0; k--) rem[k] = rem[k - 1] ^ m(top, g[k]);
        rem[0] = m(top, g[0]);
    }
    return t;
}

// Parity and syndromes are packed four to a word: byte r in bits 8 (r % 4) .. of word r / 4.
template <int ROOTS> RS_HD uint8_t packed_byte(const uint32_t (&w)[(ROOTS + 3) / 4], int r) { return (uint8_t)(w[r >> 2] >> (8 * (r & 3))); }

// what a non-zero data symbol adds to the parity of its code word: the symbol times its row of the table (`ld` = the symbol's logarithm,
// `row` = the row's 16 bytes as four words, `zero` its mark).  A zero symbol adds nothing and has no logarithm: the caller skips it.
template <int ROOTS, class T> RS_HD void parity_add(const T& L, uint32_t ld, const uint32_t (&row)[4], uint32_t zero, uint32_t (&w)[(ROOTS + 3) / 4]) {
    RS_UNROLL
    for (int k = 0; k < (ROOTS + 3) / 4; k++) {
        uint32_t t = 0;                                      // the word's bytes, then one addition
        RS_UNROLL
        for (int b = 0; b < 4; b++)
            if (4 * k + b < ROOTS && !((zero >> (4 * k + b)) & 1u)) t |= (uint32_t)L.exp[ld + ((row[k] >> (8 * b)) & 0xFFu)] << (8 * b);
        w[k] ^= t;
    }
}

// ---- decoder ----
// what symbol j (0 = highest power) of value cj adds to the syndromes S_r = sum_j c_j alpha^(r (N - 1 - j)): one look-up per root, no chain
template <int N, int ROOTS, class T> RS_HD void syndrome_add(const T& L, uint8_t cj, int j, uint32_t (&w)[(ROOTS + 3) / 4]) {
    if (!cj) return;
    const int lc = L.log[cj], e = N - 1 - j;
    int t = 0;                                               // (r e) mod 255
    RS_UNROLL
    for (int r = 0; r < ROOTS; r++) {
        w[r >> 2] ^= (uint32_t)L.exp[lc + t] << (8 * (r & 3));
        t += e; if (t >= 255) t -= 255;
    }
}

// Berlekamp-Massey over the syndromes S[0..ROOTS-1] (reed_solomon_decoder.cpp:323-382 in polynomial form), then the evaluator
// omega = S C mod x^ROOTS (:425-434), which may overwrite what S was copied from.  C (the locator on return), B, Tm: ROOTS + 1 each.  -> degree
template <int ROOTS, class T, class Syn, class Poly, class Omega>
RS_HD int locator(const T& L, const Syn& S, Poly& C, Poly& B, Poly& Tm, Omega& omega) {
    RS_UNROLL
    for (int k = 0; k <= ROOTS; k++) { C[k] = (k == 0); B[k] = (k == 0); }
    int len = 0;
    for (int r = 1; r <= ROOTS; r++) {
        uint8_t d = 0;
        RS_UNROLL
        for (int k = 0; k < ROOTS; k++) if (k < r) d ^= mul(L, C[k], S[(r - 1 - k) < 0 ? 0 : (r - 1 - k)]);
        if (d == 0) {
            RS_UNROLL
            for (int k = ROOTS; k > 0; k--) B[k] = B[k - 1];
            B[0] = 0;
        } else {
            Tm[0] = C[0];
            RS_UNROLL
            for (int k = 0; k < ROOTS; k++) Tm[k + 1] = (uint8_t)(C[k + 1] ^ mul(L, d, B[k]));
            if (2 * len <= r - 1) {
                len = r - len;
                RS_UNROLL
                for (int k = 0; k <= ROOTS; k++) B[k] = div(L, C[k], d);
            } else {
                RS_UNROLL
                for (int k = ROOTS; k > 0; k--) B[k] = B[k - 1];
                B[0] = 0;
            }
            RS_UNROLL
            for (int k = 0; k <= ROOTS; k++) C[k] = Tm[k];
        }
    }
    int deg = 0;
    RS_UNROLL
    for (int k = 0; k <= ROOTS; k++) if (C[k]) deg = k;
    RS_UNROLL
    for (int a = 0; a < ROOTS; a++) {
        uint8_t t = 0;
        RS_UNROLL
        for (int b = 0; b < ROOTS; b++) if (b <= a) t ^= mul(L, S[a - b < 0 ? 0 : a - b], C[b]);
        omega[a] = t;
    }
    return deg;
}

// Chien search (:387-410) in ascending order: reg[k] = log C_k + k x (mod 255).  chien_start leaves reg at candidate x - 1 ...
template <int ROOTS, class T, class Poly> RS_HD void chien_start(const T& L, const Poly& C, int x, int (&reg)[ROOTS + 1]) {
    RS_UNROLL
    for (int k = 1; k <= ROOTS; k++) reg[k] = (L.log[C[k]] + k * (x - 1)) % 255;
}
// ... and chien_next moves it to the next one and returns C(alpha^x): zero at a root, which marks symbol x - 1 of the unshortened block
template <int ROOTS, class T, class Poly> RS_HD uint8_t chien_next(const T& L, const Poly& C, int deg, int (&reg)[ROOTS + 1]) {
    uint8_t v = 1;
    RS_UNROLL
    for (int k = 1; k <= ROOTS; k++) {
        if (k <= deg && C[k]) {
            reg[k] += k;
            if (reg[k] >= 255) reg[k] -= 255;
            v ^= L.exp[reg[k]];
        }
    }
    return v;
}

// Forney's error value at the root alpha^x (:440-467): e = omega(X^-1) X / C'(X^-1) with first root alpha^0; zero when omega vanishes there
template <int ROOTS, class T, class Poly, class Omega> RS_HD uint8_t forney(const T& L, const Poly& C, const Omega& omega, int deg, int x) {
    uint8_t num1 = 0, den = 0;
    RS_UNROLL
    for (int a = ROOTS - 1; a >= 0; a--) if (a < deg) num1 ^= mul(L, omega[a], pow(L, a * x));
    const uint8_t num2 = pow(L, -x);
    const int top = ((deg < ROOTS - 1) ? deg : (ROOTS - 1)) & ~1;
    RS_UNROLL
    for (int a = (ROOTS - 1) & ~1; a >= 0; a -= 2) if (a <= top) den ^= mul(L, C[a + 1], pow(L, a * x));
    return div(L, mul(L, num1, num2), den);
}

}  // namespace rs
}  // namespace dabgpu
