// dabplus_tx_layout_fuzz.cpp -- dabgpu_dabplus_superframe_layout (dab-radio_amd/csrc/dabgpu_host_logic.cpp) under ASan + UBSan
// (tests/test_dabplus_tx_layout_fuzz.py builds it): random frame sizes, descriptors and lengths, 0xFFFF among them.  The start array sits
// between guard words, a success is checked against the three conditions the header states, a refusal against the reason it gives.
//   dabplus_tx_layout_fuzz <iterations> <seed>  -> one JSON line
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "dabgpu.h"

int main(int argc, char** argv) {
    const long iters = argc > 1 ? std::atol(argv[1]) : 100000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
    long failed = 0, by_status[4] = {0, 0, 0, 0};
    for (long it = 0; it < iters; it++) {
        const int kind = (int)(rng() % 4);
        uint32_t n = (kind == 0) ? (uint32_t)(rng() % 1700) : 24u * (uint32_t)(1 + rng() % 64);
        if (rng() % 97 == 0) n = (uint32_t)rng();
        const uint8_t d = (uint8_t)rng();
        const int na_exp = ((d >> 6) & 1) ? (((d >> 5) & 1) ? 3 : 6) : (((d >> 5) & 1) ? 2 : 4);
        struct { uint16_t before[4]; uint16_t start[7]; uint16_t after[4]; } g;
        for (auto& v : g.before) v = 0xBEEF;
        for (auto& v : g.after) v = 0xBEEF;
        for (auto& v : g.start) v = 0x7777;
        uint16_t len[6];
        for (auto& v : len) v = (rng() % 5 == 0) ? 0xFFFF : (uint16_t)(rng() % 3000);
        if (kind >= 2 && n >= 24 && n <= 1536 && n % 24 == 0) {
            // lengths that fill the super frame (kind 3: cut anywhere, so that starts beyond 4095 occur)
            const uint32_t first = 3 + (12 * (na_exp - 1) + 7) / 8;
            uint32_t room = 110 * (n / 24) - first - 2 * na_exp;
            for (int a = 0; a < na_exp - 1; a++) {
                const uint32_t take = (kind == 3) ? (uint32_t)(rng() % (room + 1)) : (uint32_t)(rng() % (room / (uint32_t)(na_exp - a) + 1));
                len[a] = (uint16_t)take; room -= take;
            }
            len[na_exp - 1] = (uint16_t)room;
            if (rng() % 7 == 0) len[rng() % na_exp] += (rng() & 1) ? 1 : -1;       // one byte long / short
        }
        int na = -5; uint32_t n_rs = 12345;
        const int st = dabgpu_dabplus_superframe_layout(n, d, len, g.start, &na, &n_rs);
        bool ok = st >= 0 && st <= 3;
        for (auto v : g.before) ok = ok && v == 0xBEEF;
        for (auto v : g.after) ok = ok && v == 0xBEEF;
        const bool size_ok = n >= 24 && n <= 1536 && n % 24 == 0;
        if (ok) by_status[st]++;
        if (st == 1) ok = ok && !size_ok;
        else ok = ok && size_ok && na == na_exp && n_rs == n / 24;
        if (st != 0) for (auto v : g.start) ok = ok && v == 0x7777;                 // a refusal writes no start
        if (st == 0 || st == 2 || st == 3) {
            uint64_t s = 3 + (12 * (na_exp - 1) + 7) / 8;
            bool fits = true;
            uint64_t starts[7] = {s};
            for (int a = 0; a < na_exp; a++) { s += (uint64_t)len[a] + 2; starts[a + 1] = s; if (a + 1 < na_exp && s > 4095) fits = false; }
            const bool fills = size_ok && s == 110ull * (n / 24);
            if (st == 0) {
                ok = ok && fills && fits;
                for (int a = 0; a < 7; a++) ok = ok && g.start[a] == (a <= na_exp ? starts[a] : 0);
            }
            if (st == 2) ok = ok && !fills;
            if (st == 3) ok = ok && fills && !fits;
        }
        if (!ok) { failed++; if (failed < 5) std::fprintf(stderr, "case %ld: n=%u d=%u st=%d na=%d n_rs=%u\n", it, n, d, st, na, n_rs); }
    }
    // the optional outputs really are optional
    const uint16_t two[6] = {97, 0, 0, 0, 0, 0};
    if (dabgpu_dabplus_superframe_layout(24, 0x20, two, nullptr, nullptr, nullptr) != 2 || dabgpu_dabplus_superframe_layout(24, 0x20, nullptr, nullptr, nullptr, nullptr) != -1) failed++;
    std::printf("{\"iterations\": %ld, \"failed_checks\": %ld, \"status0\": %ld, \"status1\": %ld, \"status2\": %ld, \"status3\": %ld}\n", iters, failed,
                by_status[0], by_status[1], by_status[2], by_status[3]);
    return failed ? 1 : 0;
}
