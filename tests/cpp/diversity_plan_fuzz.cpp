// Driver of the receive-diversity planner (dabgpu_diversity_plan, dab-radio_amd/csrc/dabgpu_host_logic.cpp) for tests/test_diversity_plan.py:
// a program of its own, built plain and under -fsanitize=address,undefined.  The planner dereferences no address it is handed, so the
// branch tables here hold made-up addresses.
//   plan <n_branches> <n_frames> <layout> <spb> <stride> <bits> <dqpsk> <scale> <weight> <sync> [null_table] [null_out]   one call, as JSON
//   cover <n_frames> <spb>      walks the grid the way the kernel does and counts how often every (frame, symbol) is visited
//   fuzz <n> <seed>             random arguments against the rules restated below
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "dabgpu.h"

static std::string esc(const char* s) { std::string o; for (; *s; s++) { if (*s == '"' || *s == '\\') o += '\\'; o += *s; } return o; }

static int call(int nb, size_t nf, int layout, int spb, size_t stride, uintptr_t bits, const dabgpu_diversity_branch* tab, dabgpu_diversity_geometry* g) {
    return dabgpu_diversity_plan(tab, nb, nf, (const int8_t*)bits, stride, layout, spb, g);
}

// the rules, restated: 0 = accepted, else a word of the reason the message must contain
static const char* expect(int nb, size_t nf, int layout, int spb, size_t stride, uintptr_t bits, const dabgpu_diversity_branch* tab) {
    if (nb < 1 || nb > 8) return "n_branches";
    if (nf > (size_t)1 << 24) return "n_frames";
    if (layout != 0 && layout != 1) return "bits_layout";
    if (spb < 0 || spb > 75) return "symbols_per_block";
    if (stride != 0 && (stride < 230400 || stride % 16)) return "bits_frame_stride";
    if (!bits || bits % 16) return "d_bits";
    for (int b = 0; b < nb; b++) {
        if (!tab[b].d_dqpsk || !tab[b].d_scale) return "no products or no scales";
        if ((uintptr_t)tab[b].d_dqpsk % 16) return "d_dqpsk";
        if ((uintptr_t)tab[b].d_scale % 4 || (uintptr_t)tab[b].d_weight % 4 || (uintptr_t)tab[b].d_sync % 4) return "4-byte";
    }
    return nullptr;
}

static uint64_t rng_state;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

int main(int argc, char** argv) {
    if (argc >= 12 && !strcmp(argv[1], "plan")) {
        const int nb = atoi(argv[2]);
        dabgpu_diversity_branch tab[8];
        for (int b = 0; b < 8; b++) {
            tab[b].d_dqpsk = (const float*)(uintptr_t)strtoull(argv[8], nullptr, 0);
            tab[b].d_scale = (const float*)(uintptr_t)strtoull(argv[9], nullptr, 0);
            tab[b].d_weight = (const float*)(uintptr_t)strtoull(argv[10], nullptr, 0);
            tab[b].d_sync = (const dabgpu_sync_state*)(uintptr_t)strtoull(argv[11], nullptr, 0);
        }
        // only the LAST branch carries what the command line says when "last" is given: the others are well-formed
        if (argc >= 15 && atoi(argv[14])) for (int b = 0; b + 1 < nb && b < 7; b++) { tab[b].d_dqpsk = (const float*)0x10000; tab[b].d_scale = (const float*)0x20000; tab[b].d_weight = nullptr; tab[b].d_sync = nullptr; }
        dabgpu_diversity_geometry g;
        memset(&g, 0xEE, sizeof(g));
        const bool null_table = argc >= 13 && atoi(argv[12]), null_out = argc >= 14 && atoi(argv[13]);
        const int st = dabgpu_diversity_plan(null_table ? nullptr : tab, nb, (size_t)strtoull(argv[3], nullptr, 0), (const int8_t*)(uintptr_t)strtoull(argv[7], nullptr, 0),
                                             (size_t)strtoull(argv[6], nullptr, 0), atoi(argv[4]), atoi(argv[5]), null_out ? nullptr : &g);
        printf("{\"status\": %d, \"error\": \"%s\", \"symbols_per_block\": %u, \"runs_per_frame\": %u, \"grid\": %u, \"threads\": %u, \"lds_bytes\": %u}\n", st,
               st ? esc(dabgpu_last_error()).c_str() : "", g.symbols_per_block, g.runs_per_frame, g.grid, g.threads, g.lds_bytes);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "cover")) {
        const size_t nf = (size_t)strtoull(argv[2], nullptr, 0);
        const int spb = atoi(argv[3]);
        dabgpu_diversity_branch tab[1] = {{(const float*)0x10000, (const float*)0x20000, nullptr, nullptr}};
        dabgpu_diversity_geometry g;
        if (call(1, nf, 0, spb, 0, 0x30000, tab, &g)) { printf("{\"status\": 2}\n"); return 0; }
        std::vector<uint8_t> seen(nf * 75, 0);
        size_t outside = 0;
        for (uint32_t blk = 0; blk < g.grid; blk++) {                 // the kernel's own index arithmetic (diversity.hip)
            const size_t frame = blk / g.runs_per_frame; const int run = (int)(blk % g.runs_per_frame);
            if (frame >= nf) continue;
            const int row0 = run * (int)g.symbols_per_block, row1 = row0 + (int)g.symbols_per_block < 75 ? row0 + (int)g.symbols_per_block : 75;
            for (int row = row0; row < row1; row++) { if (row < 0 || row >= 75) outside++; else seen[frame * 75 + row]++; }
        }
        size_t once = 0;
        for (uint8_t v : seen) once += v == 1;
        printf("{\"status\": 0, \"cells\": %zu, \"once\": %zu, \"outside\": %zu, \"symbols_per_block\": %u, \"runs_per_frame\": %u, \"grid\": %u}\n", seen.size(), once,
               outside, g.symbols_per_block, g.runs_per_frame, g.grid);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "fuzz")) {
        const long n = atol(argv[2]);
        rng_state = 0x9E3779B97F4A7C15ull ^ (uint64_t)atol(argv[3]);
        long accepted = 0, refused = 0, failed = 0, chosen = 0;
        long reasons[9] = {0};
        static const char* const WORDS[9] = {"n_branches", "n_frames", "bits_layout", "symbols_per_block", "bits_frame_stride", "d_bits", "no products or no scales",
                                             "d_dqpsk", "4-byte"};
        for (long it = 0; it < n; it++) {
            // mostly valid values, each field wrong now and then
            const int nb = (rnd() % 16 == 0) ? (int)(rnd() % 20) - 5 : 1 + (int)(rnd() % 8);
            const size_t nf = (rnd() % 24 == 0) ? ((size_t)1 << 24) + (rnd() % 3) - 1 : (size_t)(rnd() % 5000);
            const int layout = (rnd() % 16 == 0) ? (int)(rnd() % 7) - 3 : (int)(rnd() % 2);
            const int spb = (rnd() % 12 == 0) ? (int)(rnd() % 200) - 60 : (int)(rnd() % 76);
            const size_t stride = (rnd() % 3 == 0) ? 0 : (rnd() % 8 == 0) ? (size_t)(rnd() % 400000) : 230400 + 16 * (size_t)(rnd() % 5000);
            const uintptr_t bits = (rnd() % 16 == 0) ? (uintptr_t)(rnd() % 64) : 0x40000 + 16 * (uintptr_t)(rnd() % 1000);
            dabgpu_diversity_branch tab[8];
            for (int b = 0; b < 8; b++) {
                tab[b].d_dqpsk = (const float*)((rnd() % 40 == 0) ? (uintptr_t)(rnd() % 3) * 8 : 0x100000 + 16 * (uintptr_t)(rnd() % 4096));
                tab[b].d_scale = (const float*)((rnd() % 40 == 0) ? (uintptr_t)(rnd() % 4) : 0x200000 + 4 * (uintptr_t)(rnd() % 4096));
                tab[b].d_weight = (const float*)((rnd() % 2) ? 0 : (rnd() % 40 == 0) ? 0x300001 : 0x300000 + 4 * (uintptr_t)(rnd() % 4096));
                tab[b].d_sync = (const dabgpu_sync_state*)((rnd() % 2) ? 0 : (rnd() % 40 == 0) ? 0x400002 : 0x400000 + 4 * (uintptr_t)(rnd() % 4096));
            }
            dabgpu_diversity_geometry g;
            memset(&g, 0xEE, sizeof(g));
            const int st = call(nb, nf, layout, spb, stride, bits, tab, &g);
            const char* want = expect(nb, nf, layout, spb, stride, bits, tab);
            bool ok = true;
            if (want) {
                ok = st == DABGPU_ERR_INVALID_ARG && strstr(dabgpu_last_error(), want) && g.grid == 0 && g.threads == 0 && g.symbols_per_block == 0;
                refused++;
                for (int r = 0; r < 9; r++) if (!strcmp(want, WORDS[r])) reasons[r]++;
            } else {
                const uint32_t s = g.symbols_per_block, r = g.runs_per_frame;
                ok = st == DABGPU_OK && s >= 1 && s <= 75 && (spb == 0 || s == (uint32_t)spb) && r * s >= 75 && (r - 1) * s < 75 && g.grid == nf * r &&
                     g.threads == 256 && g.lds_bytes == 6144;
                // the choice: at most 25 runs a frame, and from 86 frames on three runs of 25
                if (ok && spb == 0) { chosen++; ok = r <= 25 && (nf < 86 || s == 25); }
                // the result does not depend on the stride, the layout or the optional pointers
                dabgpu_diversity_geometry g2;
                for (int b = 0; b < 8; b++) { tab[b].d_weight = nullptr; tab[b].d_sync = nullptr; }
                ok = ok && call(nb, nf, 1 - layout, spb, 0, bits, tab, &g2) == DABGPU_OK && !memcmp(&g, &g2, sizeof(g));
                accepted++;
            }
            if (!ok) { failed++; if (failed < 5) fprintf(stderr, "case %ld: status %d error '%s' expected '%s'\n", it, st, dabgpu_last_error(), want ? want : "ok"); }
        }
        printf("{\"checked\": %ld, \"accepted\": %ld, \"refused\": %ld, \"failed_checks\": %ld, \"chosen\": %ld, \"reasons\": [", n, accepted, refused, failed, chosen);
        for (int r = 0; r < 9; r++) printf("%ld%s", reasons[r], r < 8 ? ", " : "");
        printf("]}\n");
        return failed ? 1 : 0;
    }
    fprintf(stderr, "usage: see the head of tests/cpp/diversity_plan_fuzz.cpp\n");
    return 2;
}
