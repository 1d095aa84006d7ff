// rs_core_host.cpp -- dab-radio_amd/csrc/rs_core.h on the host (tests/test_rs_core_host.py): the pieces the kernels deal over lanes, composed
// serially for one word -- syndromes, locator, Chien search over alpha^1..alpha^255, Forney, and the rule that the roots found must number
// the locator's degree.  CODE is 120 (RS(120,110), DAB+) or 204 (RS(204,188), packet mode).
//   rs_core_host decode CODE IN OUT       IN: words of CODE bytes; OUT per word, as i32: the count (-1: uncorrectable), 16 positions in the
//                                         order of the search (-1 beyond the count), the CODE symbols after correction
//   rs_core_host parity CODE IN OUT       IN: data parts (CODE - roots bytes each); OUT: their parity bytes through the parity map
//   rs_core_host fuzz SEED ROUNDS         both codes: code words with 0..roots symbol errors anywhere in the 255-symbol block, the shortened
//                                         region included, and random words; invariants checked here; built with
//                                         -fsanitize=address,undefined by the test and run directly
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "rs_core.h"

using namespace dabgpu;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); abort(); } } while (0)

static constexpr rs::GfTables GF = rs::make_gf();

static uint64_t rng_state = 1;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }

template <int N, int ROOTS> struct Code {
    static constexpr int PAD = 255 - N, DATA = N - ROOTS, WORDS = (ROOTS + 3) / 4;

    // the word's syndromes on top of those in w (the fuzz puts errors of the shortened region there, which no word can carry)
    static int decode(uint8_t* word, int* positions, uint32_t (&w)[WORDS]) {
        for (int j = 0; j < N; j++) rs::syndrome_add<N, ROOTS>(GF, word[j], j, w);
        uint8_t S[ROOTS], any = 0;
        for (int r = 0; r < ROOTS; r++) any |= S[r] = rs::packed_byte<ROOTS>(w, r);
        if (!any) return 0;
        uint8_t C[ROOTS + 1], B[ROOTS + 1], T[ROOTS + 1], omega[ROOTS];
        const int deg = rs::locator<ROOTS>(GF, S, C, B, T, omega);
        int reg[ROOTS + 1], root[ROOTS], found = 0;
        rs::chien_start<ROOTS>(GF, C, 1, reg);
        for (int x = 1; x <= 255; x++) {
            if (rs::chien_next<ROOTS>(GF, C, deg, reg)) continue;
            CHECK(found < deg);                              // a polynomial of degree d has at most d roots
            root[found++] = x;
        }
        if (found != deg) return -1;
        for (int k = 0; k < found; k++) {
            const int loc = root[k] - 1;
            positions[k] = loc;
            if (loc >= PAD) word[loc - PAD] ^= rs::forney<ROOTS>(GF, C, omega, deg, root[k]);
        }
        return deg;
    }

    static void parity(const uint8_t* data, uint8_t* out) {
        static constexpr rs::ParityTab<DATA, ROOTS> TAB = rs::make_parity_tab<DATA, ROOTS>();
        uint32_t w[WORDS] = {};
        for (int j = 0; j < DATA; j++) {
            if (!data[j]) continue;
            uint32_t row[4];
            memcpy(row, TAB.log_coef[j], 16);
            rs::parity_add<ROOTS>(GF, GF.log[data[j]], row, TAB.zero[j], w);
        }
        for (int r = 0; r < ROOTS; r++) out[r] = rs::packed_byte<ROOTS>(w, r);
    }

    static int run_decode(FILE* in, FILE* out) {
        std::vector<uint8_t> word(N);
        while (fread(word.data(), 1, N, in) == (size_t)N) {
            int32_t rec[1 + 16 + N];
            int pos[ROOTS];
            uint32_t w[WORDS] = {};
            rec[0] = decode(word.data(), pos, w);
            for (int k = 0; k < 16; k++) rec[1 + k] = (k < rec[0]) ? pos[k] : -1;
            for (int j = 0; j < N; j++) rec[17 + j] = word[j];
            fwrite(rec, 4, 1 + 16 + N, out);
        }
        return 0;
    }

    static int run_parity(FILE* in, FILE* out) {
        std::vector<uint8_t> data(DATA), par(ROOTS);
        while (fread(data.data(), 1, DATA, in) == (size_t)DATA) {
            parity(data.data(), par.data());
            fwrite(par.data(), 1, ROOTS, out);
        }
        return 0;
    }

    static void fuzz();
};

template <int N, int ROOTS> void Code<N, ROOTS>::fuzz() {
    // exactly the word and exactly the positions a decode may report: the sanitizer sees any index beyond them
    std::vector<uint8_t> sent(N), word;
    std::vector<int> pos(ROOTS, -1);
    for (int j = 0; j < DATA; j++) sent[j] = (rnd() % 4 == 0) ? 0 : (uint8_t)rnd();
    parity(sent.data(), sent.data() + DATA);
    {
        word = sent;
        uint32_t w[WORDS] = {};
        CHECK(decode(word.data(), pos.data(), w) == 0 && word == sent);
    }
    // e errors at distinct places of the 255-symbol block; those below PAD only exist as syndromes
    const int e = (int)(rnd() % (ROOTS + 1));
    std::vector<int> where;
    while ((int)where.size() < e) {
        const int p = (rnd() % 3 == 0) ? (int)(rnd() % PAD) : PAD + (int)(rnd() % N);
        if (std::find(where.begin(), where.end(), p) == where.end()) where.push_back(p);
    }
    std::sort(where.begin(), where.end());
    word = sent;
    uint32_t w[WORDS] = {};
    for (int p : where) {
        const uint8_t v = (uint8_t)(1 + rnd() % 255);
        if (p >= PAD) word[p - PAD] ^= v;
        else rs::syndrome_add<255, ROOTS>(GF, v, p, w);
    }
    const int count = decode(word.data(), pos.data(), w);
    if (e <= ROOTS / 2) {
        CHECK(count == e && word == sent);                   // (errors of the shortened region are reported, not applied)
        for (int k = 0; k < e; k++) CHECK(pos[k] == where[k]);
    } else {
        CHECK(count >= -1 && count <= ROOTS);
        for (int k = 0; k < count; k++) CHECK(pos[k] >= 0 && pos[k] < 255);
    }
    for (auto& v : word) v = (uint8_t)rnd();
    uint32_t w2[WORDS] = {};
    const int c2 = decode(word.data(), pos.data(), w2);
    CHECK(c2 >= -1 && c2 <= ROOTS);
}

template <class C> static int run(const char* mode, const char* in_path, const char* out_path) {
    FILE* in = fopen(in_path, "rb");
    FILE* out = fopen(out_path, "wb");
    if (!in || !out) return 2;
    const int st = !strcmp(mode, "decode") ? C::run_decode(in, out) : C::run_parity(in, out);
    fclose(in);
    fclose(out);
    return st;
}

int main(int argc, char** argv) {
    if (argc >= 5 && (!strcmp(argv[1], "decode") || !strcmp(argv[1], "parity"))) {
        if (!strcmp(argv[2], "120")) return run<Code<120, 10>>(argv[1], argv[3], argv[4]);
        if (!strcmp(argv[2], "204")) return run<Code<204, 16>>(argv[1], argv[3], argv[4]);
    }
    if (argc >= 4 && !strcmp(argv[1], "fuzz")) {
        rng_state = strtoull(argv[2], nullptr, 10) * 2 + 1;
        const long rounds = strtol(argv[3], nullptr, 10);
        for (long i = 0; i < rounds; i++) { Code<120, 10>::fuzz(); Code<204, 16>::fuzz(); }
        printf("fuzz ok: %ld rounds\n", rounds);
        return 0;
    }
    fprintf(stderr, "usage: rs_core_host decode|parity 120|204 IN OUT | fuzz SEED ROUNDS\n");
    return 2;
}
