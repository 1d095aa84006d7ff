// Driver of the symbol noise profile's planner and of the symbol-weighted combiner's (dabgpu_sym_profile_plan,
// dabgpu_diversity_plan_symbols, dab-radio_amd/csrc/dabgpu_host_logic.cpp) for tests/test_sym_profile_plan.py: a program of its own,
// built plain and under -fsanitize=address,undefined.  The planners dereference no device address they are handed, so the addresses here
// are made up.
//   plan <mode> <dqpsk> <n_frames> <sync> <symbol_weight> <symbol_noise> <ref_noise> <valid> [null_out]       one call, as JSON
//   dplan <n_branches> <n_frames> <bits> <stride> <layout> <spb> <dq> <scale> <weight> <sync> <band> <sym> <tables>
//                               one call of the combiner's planner: every branch has the same addresses; tables: 0 both arrays null,
//                               1 the band array only, 2 the symbol array only, 3 both
//   fuzz <n> <seed>             random arguments of both planners against the rules restated below
//   frames                      dabgpu_sym_profile_rows_host on a few frames (under the sanitizers too)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "dabgpu.h"

static std::string esc(const char* s) { std::string o; for (; *s; s++) { if (*s == '"' || *s == '\\') o += '\\'; o += *s; } return o; }

// p: sync, symbol_weight, symbol_noise, ref_noise, valid
struct Args { int mode; uintptr_t dq; size_t nf; uintptr_t p[5]; };

static int call(const Args& a, dabgpu_noise_geometry* g) {
    return dabgpu_sym_profile_plan(a.mode, (const float*)a.dq, a.nf, (const dabgpu_sync_state*)a.p[0], (const float*)a.p[1], (const float*)a.p[2],
                                   (const float*)a.p[3], (const uint32_t*)a.p[4], g);
}

// the rules, restated: 0 = accepted, else a word of the reason the message must contain
static const char* expect(const Args& a) {
    if (a.mode != 1) return "mode";
    if (a.nf == 0 || a.nf > (size_t)1 << 24) return "n_frames";
    if (!a.dq) return "null products";
    if (a.dq % 16) return "16-byte";
    for (int i = 0; i < 5; i++) if (a.p[i] % 4) return "4-byte";
    if (!a.p[1] && !a.p[2] && !a.p[3] && !a.p[4]) return "no output";
    return nullptr;
}

// the combiner's planner: one branch record for all branches
struct DArgs { int nb; size_t nf; uintptr_t bits; size_t stride; int layout, spb; uintptr_t dq, scale, weight, sync, band, sym; int tables; };

static int dcall(const DArgs& a, dabgpu_diversity_geometry* g) {
    dabgpu_diversity_branch br[16];
    const float* band[16];
    const float* sym[16];
    for (int b = 0; b < 16; b++) {
        br[b].d_dqpsk = (const float*)a.dq; br[b].d_scale = (const float*)a.scale; br[b].d_weight = (const float*)a.weight;
        br[b].d_sync = (const dabgpu_sync_state*)a.sync;
        band[b] = (const float*)a.band; sym[b] = (const float*)a.sym;
    }
    return dabgpu_diversity_plan_symbols(br, a.nb, a.nf, (const int8_t*)a.bits, a.stride, a.layout, a.spb, (a.tables & 1) ? band : nullptr,
                                         (a.tables & 2) ? sym : nullptr, g);
}

static const char* dexpect(const DArgs& a) {
    if (a.nb < 1 || a.nb > 8) return "n_branches";
    if (a.nf > (size_t)1 << 24) return "n_frames";
    if (a.layout != 0 && a.layout != 1) return "bits_layout";
    if (a.spb < 0 || a.spb > 75) return "symbols_per_block";
    if (a.stride != 0 && (a.stride < 230400 || a.stride % 16)) return "bits_frame_stride";
    if (!a.bits || a.bits % 16) return "d_bits";
    if (!a.dq || !a.scale) return "no products";
    if (a.dq % 16) return "d_dqpsk";
    if ((a.scale | a.weight | a.sync) % 4) return "scales, weights";
    if ((a.tables & 1) && a.band) {
        if (a.band % 4) return "band weights";
        if (a.weight) return "both a band table";
    }
    if ((a.tables & 2) && a.sym && a.sym % 4) return "symbol weights";
    return nullptr;
}

static uint64_t rng_state;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static const int N_WORDS = 6, N_DWORDS = 12;
static const char* const WORDS[N_WORDS] = {"mode", "n_frames", "null products", "16-byte", "4-byte", "no output"};
static const char* const DWORDS[N_DWORDS] = {"n_branches", "n_frames", "bits_layout", "symbols_per_block", "bits_frame_stride", "d_bits", "no products",
                                             "d_dqpsk", "scales, weights", "band weights", "both a band table", "symbol weights"};

int main(int argc, char** argv) {
    if (argc >= 10 && !strcmp(argv[1], "plan")) {
        Args a;
        a.mode = atoi(argv[2]);
        a.dq = (uintptr_t)strtoull(argv[3], nullptr, 0);
        a.nf = (size_t)strtoull(argv[4], nullptr, 0);
        for (int i = 0; i < 5; i++) a.p[i] = (uintptr_t)strtoull(argv[5 + i], nullptr, 0);
        dabgpu_noise_geometry g;
        memset(&g, 0xEE, sizeof(g));
        const bool null_out = argc >= 11 && atoi(argv[10]);
        const int st = call(a, null_out ? nullptr : &g);
        printf("{\"status\": %d, \"error\": \"%s\", \"grid\": %u, \"threads\": %u, \"lds_bytes\": %u}\n", st, st ? esc(dabgpu_last_error()).c_str() : "", g.grid,
               g.threads, g.lds_bytes);
        return 0;
    }
    if (argc == 15 && !strcmp(argv[1], "dplan")) {
        DArgs a;
        a.nb = atoi(argv[2]); a.nf = (size_t)strtoull(argv[3], nullptr, 0); a.bits = (uintptr_t)strtoull(argv[4], nullptr, 0);
        a.stride = (size_t)strtoull(argv[5], nullptr, 0); a.layout = atoi(argv[6]); a.spb = atoi(argv[7]);
        a.dq = (uintptr_t)strtoull(argv[8], nullptr, 0); a.scale = (uintptr_t)strtoull(argv[9], nullptr, 0);
        a.weight = (uintptr_t)strtoull(argv[10], nullptr, 0); a.sync = (uintptr_t)strtoull(argv[11], nullptr, 0);
        a.band = (uintptr_t)strtoull(argv[12], nullptr, 0); a.sym = (uintptr_t)strtoull(argv[13], nullptr, 0); a.tables = atoi(argv[14]);
        dabgpu_diversity_geometry g;
        memset(&g, 0xEE, sizeof(g));
        const int st = dcall(a, &g);
        printf("{\"status\": %d, \"error\": \"%s\", \"grid\": %u, \"threads\": %u, \"lds_bytes\": %u, \"symbols_per_block\": %u, \"runs_per_frame\": %u}\n", st,
               st ? esc(dabgpu_last_error()).c_str() : "", g.grid, g.threads, g.lds_bytes, g.symbols_per_block, g.runs_per_frame);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "fuzz")) {
        const long n = atol(argv[2]);
        rng_state = 0x9E3779B97F4A7C15ull ^ (uint64_t)atol(argv[3]);
        long accepted = 0, refused = 0, failed = 0, reasons[N_WORDS] = {0}, daccepted = 0, drefused = 0, dreasons[N_DWORDS] = {0};
        for (long it = 0; it < n; it++) {
            // mostly valid values, each field wrong now and then
            Args a;
            a.mode = (rnd() % 24 == 0) ? (int)(rnd() % 7) - 1 : 1;
            a.dq = (rnd() % 24 == 0) ? (uintptr_t)(rnd() % 3) * 8 : 0x100000 + ((rnd() % 16 == 0) ? 4 : 16) * (uintptr_t)(rnd() % 4096);
            a.nf = (rnd() % 16 == 0) ? ((size_t)1 << 24) + (rnd() % 3) - 1 : (size_t)(rnd() % 5000);
            for (int i = 0; i < 5; i++)
                a.p[i] = (rnd() % (i < 1 ? 2 : 3) == 0) ? 0 : 0x40000000 * (uintptr_t)(i + 1) + ((rnd() % 50 == 0) ? 1 + (uintptr_t)(rnd() % 3) : 4 * (uintptr_t)(rnd() % 4096));
            dabgpu_noise_geometry g;
            memset(&g, 0xEE, sizeof(g));
            const int st = call(a, &g);
            const char* want = expect(a);
            bool ok;
            if (want) {
                ok = st == DABGPU_ERR_INVALID_ARG && strstr(dabgpu_last_error(), want) && g.grid == 0 && g.threads == 0 && g.lds_bytes == 0;
                refused++;
                for (int r = 0; r < N_WORDS; r++) if (!strcmp(want, WORDS[r])) reasons[r]++;
            } else {
                ok = st == DABGPU_OK && g.grid == (uint32_t)a.nf && g.threads == 256 && g.lds_bytes == 4512;
                accepted++;
            }
            if (!ok) {
                failed++;
                if (failed < 10) fprintf(stderr, "iteration %ld: want %s, status %d (%s), grid %u\n", it, want ? want : "ok", st, dabgpu_last_error(), g.grid);
            }
            // the combiner's planner
            DArgs d;
            d.nb = (rnd() % 16 == 0) ? (int)(rnd() % 12) - 1 : 1 + (int)(rnd() % 8);
            d.nf = (rnd() % 24 == 0) ? ((size_t)1 << 24) + (rnd() % 3) - 1 : (size_t)(rnd() % 5000);
            d.bits = (rnd() % 24 == 0) ? (uintptr_t)(rnd() % 2) * 8 : 0x700000 + ((rnd() % 24 == 0) ? 8 : 16) * (uintptr_t)(rnd() % 4096);
            d.stride = (rnd() % 3 == 0) ? 0 : 230400 + ((rnd() % 16 == 0) ? 8 : 16) * (size_t)(rnd() % 100) - ((rnd() % 24 == 0) ? 32 : 0);
            d.layout = (rnd() % 24 == 0) ? (int)(rnd() % 5) - 1 : (int)(rnd() % 2);
            d.spb = (rnd() % 24 == 0) ? (int)(rnd() % 90) - 5 : (int)(rnd() % 76);
            d.dq = (rnd() % 32 == 0) ? 0 : 0x100000 + ((rnd() % 24 == 0) ? 4 : 16) * (uintptr_t)(rnd() % 4096);
            d.scale = (rnd() % 32 == 0) ? 0 : 0x200000 + ((rnd() % 32 == 0) ? 2 : 4) * (uintptr_t)(rnd() % 4096);
            d.weight = (rnd() % 2 == 0) ? 0 : 0x300000 + ((rnd() % 32 == 0) ? 2 : 4) * (uintptr_t)(rnd() % 4096);
            d.sync = (rnd() % 2 == 0) ? 0 : 0x400000 + ((rnd() % 32 == 0) ? 2 : 4) * (uintptr_t)(rnd() % 4096);
            d.band = (rnd() % 2 == 0) ? 0 : 0x500000 + ((rnd() % 16 == 0) ? 2 : 4) * (uintptr_t)(rnd() % 4096);
            d.sym = (rnd() % 3 == 0) ? 0 : 0x600000 + ((rnd() % 8 == 0) ? 1 : 4) * (uintptr_t)(rnd() % 4096);
            d.tables = (int)(rnd() % 4);
            if ((d.tables & 1) && d.band && rnd() % 4) d.weight = 0;
            dabgpu_diversity_geometry dg;
            memset(&dg, 0xEE, sizeof(dg));
            const int dst = dcall(d, &dg);
            const char* dwant = dexpect(d);
            if (dwant) {
                ok = dst == DABGPU_ERR_INVALID_ARG && strstr(dabgpu_last_error(), dwant) && dg.grid == 0 && dg.threads == 0 && dg.lds_bytes == 0;
                drefused++;
                for (int r = 0; r < N_DWORDS; r++) if (!strcmp(dwant, DWORDS[r])) dreasons[r]++;
            } else {
                const bool tabled = ((d.tables & 1) && d.band) || ((d.tables & 2) && d.sym);
                ok = dst == DABGPU_OK && dg.threads == 256 && dg.lds_bytes == (tabled ? 6144u + 64u : 6144u) && dg.grid == (uint32_t)d.nf * dg.runs_per_frame &&
                     dg.runs_per_frame == (75u + dg.symbols_per_block - 1u) / dg.symbols_per_block && (d.spb == 0 || dg.symbols_per_block == (uint32_t)d.spb);
                daccepted++;
            }
            if (!ok) {
                failed++;
                if (failed < 10) fprintf(stderr, "iteration %ld (combiner): want %s, status %d (%s), grid %u lds %u\n", it, dwant ? dwant : "ok", dst, dabgpu_last_error(), dg.grid, dg.lds_bytes);
            }
        }
        printf("{\"checked\": %ld, \"accepted\": %ld, \"refused\": %ld, \"failed_checks\": %ld, \"reasons\": [", n, accepted, refused, failed);
        for (int r = 0; r < N_WORDS; r++) printf("%s%ld", r ? ", " : "", reasons[r]);
        printf("], \"combiner_accepted\": %ld, \"combiner_refused\": %ld, \"combiner_reasons\": [", daccepted, drefused);
        for (int r = 0; r < N_DWORDS; r++) printf("%s%ld", r ? ", " : "", dreasons[r]);
        printf("]}\n");
        return failed ? 1 : 0;
    }
    if (argc == 2 && !strcmp(argv[1], "frames")) {
        // the host form on exactly sized heap blocks: a read or write past a frame is the sanitizer's to find
        const size_t n = (size_t)75 * 1536 * 2;
        long failed = 0;
        for (int kind = 0; kind < 5; kind++) {
            std::vector<float> dq(n), v(75, -1.0f), q(75, -1.0f);
            float ref = -1.0f;
            rng_state = 0x1234567ull + (uint64_t)kind;
            for (size_t i = 0; i < n; i++) dq[i] = kind == 1 ? 0.0f : ((float)(int64_t)(rnd() % 2001) - 1000.0f) * 37.0f;
            if (kind == 2) { dq[5] = NAN; dq[9000] = INFINITY; dq[n - 1] = -INFINITY; }
            if (kind == 4) for (size_t i = 0; i < n / 2 + 3072; i++) dq[i] = NAN;            // 38 bad rows
            const int ok = dabgpu_sym_profile_rows_host(dq.data(), kind == 3 ? nullptr : v.data(), q.data(), kind == 3 ? nullptr : &ref);
            if (dabgpu_sym_profile_rows_host(nullptr, v.data(), q.data(), &ref) != -1) failed++;
            if (ok != ((kind == 1 || kind == 4) ? 0 : 1)) failed++;
            if (kind == 3) continue;
            int ones = 0;
            for (int s = 0; s < 75; s++) {
                if (!(v[s] >= 0.0f && v[s] <= 1.0f) || !(q[s] >= 0.0f)) failed++;
                if (!ok && (v[s] != 0.0f || q[s] != 0.0f)) failed++;
                ones += v[s] == 1.0f;
            }
            if (ok && (ones < 38 || !(ref > 0.0f))) failed++;
            if (!ok && ref != 0.0f) failed++;
            if (kind == 2 && (v[0] != 0.0f || v[74] != 0.0f || !isinf(q[0]))) failed++;
        }
        printf("{\"failed_checks\": %ld}\n", failed);
        return failed ? 1 : 0;
    }
    fprintf(stderr, "usage: see the head of tests/cpp/sym_profile_plan_fuzz.cpp\n");
    return 2;
}
