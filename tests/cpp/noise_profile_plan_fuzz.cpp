// Driver of the noise profile's planner and the banded combiner's (dabgpu_noise_profile_plan, dabgpu_diversity_plan_banded,
// dab-radio_amd/csrc/dabgpu_host_logic.cpp) for tests/test_noise_profile_plan.py: a program of its own, built plain and under
// -fsanitize=address,undefined.  The planners dereference no address they are handed (the tables in host memory apart), so the addresses
// here are made up.
//   plan <mode> <iq> <n_frames> <stride> <null_offset> <alpha> <states> <freq> <exclude> <profile_in> <profile_out> <band_weight> <mean> <power>
//        <valid> [null_out]                                       one call, as JSON
//   banded <n_branches> <n_frames> <bits> <stride> <layout> <spb> <dqpsk0> <scale0> <weight0> <band0> <band1> [null_bands]
//                                                                 branch 0 as given, the others well formed with band1
//   fuzz <n> <seed>             random arguments of both planners against the rules restated below
//   bands                       dabgpu_noise_profile_bands_host, _exclude_tii and _band_mean_host on a few tables (under the sanitizers too)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include "dabgpu.h"

static std::string esc(const char* s) { std::string o; for (; *s; s++) { if (*s == '"' || *s == '\\') o += '\\'; o += *s; } return o; }

// p: states, freq, exclude, profile_in, profile_out, band_weight, mean, power, valid
struct Args { int mode; uintptr_t iq; size_t nf, stride, off; float alpha; uintptr_t p[9]; };

static int call(const Args& a, dabgpu_noise_geometry* g) {
    return dabgpu_noise_profile_plan(a.mode, (const float*)a.iq, a.nf, a.stride, a.off, (const dabgpu_sync_state*)a.p[0], (const float*)a.p[1],
                                     (const uint32_t*)a.p[2], (const float*)a.p[3], a.alpha, (const float*)a.p[4], (const float*)a.p[5],
                                     (const float*)a.p[6], (const float*)a.p[7], (const uint32_t*)a.p[8], g);
}

// the rules, restated: 0 = accepted, else a word of the reason the message must contain
static const char* expect(const Args& a) {
    if (a.mode != 1) return "mode";
    if (a.nf == 0 || a.nf > (size_t)1 << 24) return "n_frames";
    if (!a.iq) return "null samples";
    if (a.iq % 8) return "8-byte";
    for (int i = 0; i < 9; i++) if (a.p[i] % 4) return "4-byte";
    const size_t lim = (size_t)1 << 40;
    if (a.off > lim || a.stride > lim || a.stride < a.off + 2656 + (a.p[0] ? 1543 : 0)) return "stream_stride_samples";
    if (!(a.alpha > 0.0f && a.alpha <= 1.0f)) return "alpha";
    if (a.p[3] && a.p[4] && a.p[3] != a.p[4]) {
        const uintptr_t bytes = (uintptr_t)a.nf * 512;
        if (a.p[3] < a.p[4] + bytes && a.p[4] < a.p[3] + bytes) return "overlap";
    }
    if (!a.p[4] && !a.p[5] && !a.p[6] && !a.p[7] && !a.p[8]) return "no output";
    return nullptr;
}

struct Banded { int n; size_t nf; uintptr_t bits; size_t stride; int layout, spb; dabgpu_diversity_branch br[9]; const float* band[9]; bool null_bands; };

static int call(const Banded& b, dabgpu_diversity_geometry* g) {
    return dabgpu_diversity_plan_banded(b.br, b.n, b.nf, (const int8_t*)b.bits, b.stride, b.layout, b.spb, b.null_bands ? nullptr : b.band, g);
}
static const char* expect(const Banded& b) {
    if (b.n < 1 || b.n > 8) return "n_branches";
    if (b.nf > (size_t)1 << 24) return "n_frames";
    if (b.layout != 0 && b.layout != 1) return "bits_layout";
    if (b.spb < 0 || b.spb > 75) return "symbols_per_block";
    if (b.stride != 0 && (b.stride < 230400 || b.stride % 16)) return "bits_frame_stride";
    if (!b.bits || b.bits % 16) return "d_bits";
    for (int i = 0; i < b.n; i++) {
        if (!b.br[i].d_dqpsk || !b.br[i].d_scale) return "no products or no scales";
        if ((uintptr_t)b.br[i].d_dqpsk % 16) return "16-byte";
        if (((uintptr_t)b.br[i].d_scale | (uintptr_t)b.br[i].d_weight | (uintptr_t)b.br[i].d_sync) % 4) return "4-byte";
    }
    if (b.null_bands) return nullptr;
    for (int i = 0; i < b.n; i++) {
        if (!b.band[i]) continue;
        if ((uintptr_t)b.band[i] % 4) return "band weights must be 4-byte";
        if (b.br[i].d_weight) return "both a band table and d_weight";
    }
    return nullptr;
}
static bool any_band(const Banded& b) { if (b.null_bands) return false; for (int i = 0; i < b.n && i < 8; i++) if (b.band[i]) return true; return false; }

static uint64_t rng_state;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static const char* const WORDS[10] = {"mode", "n_frames", "null samples", "8-byte", "4-byte", "stream_stride_samples", "alpha", "overlap", "no output", ""};
static const char* const BWORDS[11] = {"n_branches", "n_frames", "bits_layout", "symbols_per_block", "bits_frame_stride", "d_bits",
                                       "no products or no scales", "16-byte", "4-byte", "band weights must be 4-byte", "both a band table and d_weight"};

int main(int argc, char** argv) {
    if (argc >= 17 && !strcmp(argv[1], "plan")) {
        Args a;
        a.mode = atoi(argv[2]);
        a.iq = (uintptr_t)strtoull(argv[3], nullptr, 0);
        a.nf = (size_t)strtoull(argv[4], nullptr, 0); a.stride = (size_t)strtoull(argv[5], nullptr, 0); a.off = (size_t)strtoull(argv[6], nullptr, 0);
        a.alpha = strtof(argv[7], nullptr);
        for (int i = 0; i < 9; i++) a.p[i] = (uintptr_t)strtoull(argv[8 + i], nullptr, 0);
        dabgpu_noise_geometry g;
        memset(&g, 0xEE, sizeof(g));
        const bool null_out = argc >= 18 && atoi(argv[17]);
        const int st = call(a, null_out ? nullptr : &g);
        printf("{\"status\": %d, \"error\": \"%s\", \"grid\": %u, \"threads\": %u, \"lds_bytes\": %u}\n", st, st ? esc(dabgpu_last_error()).c_str() : "", g.grid,
               g.threads, g.lds_bytes);
        return 0;
    }
    if (argc >= 13 && !strcmp(argv[1], "banded")) {
        Banded b;
        memset(&b, 0, sizeof(b));
        b.n = atoi(argv[2]); b.nf = (size_t)strtoull(argv[3], nullptr, 0); b.bits = (uintptr_t)strtoull(argv[4], nullptr, 0);
        b.stride = (size_t)strtoull(argv[5], nullptr, 0); b.layout = atoi(argv[6]); b.spb = atoi(argv[7]);
        for (int i = 0; i < 9; i++) {
            b.br[i].d_dqpsk = (const float*)(uintptr_t)(0x1000000 * (i + 1)); b.br[i].d_scale = (const float*)(uintptr_t)(0x100000 + 64 * i);
            b.band[i] = (const float*)(uintptr_t)strtoull(argv[12], nullptr, 0);
        }
        b.br[0].d_dqpsk = (const float*)(uintptr_t)strtoull(argv[8], nullptr, 0); b.br[0].d_scale = (const float*)(uintptr_t)strtoull(argv[9], nullptr, 0);
        b.br[0].d_weight = (const float*)(uintptr_t)strtoull(argv[10], nullptr, 0); b.band[0] = (const float*)(uintptr_t)strtoull(argv[11], nullptr, 0);
        b.null_bands = argc >= 14 && atoi(argv[13]);
        dabgpu_diversity_geometry g;
        memset(&g, 0xEE, sizeof(g));
        const int st = call(b, &g);
        printf("{\"status\": %d, \"error\": \"%s\", \"symbols_per_block\": %u, \"runs_per_frame\": %u, \"grid\": %u, \"threads\": %u, \"lds_bytes\": %u}\n", st,
               st ? esc(dabgpu_last_error()).c_str() : "", g.symbols_per_block, g.runs_per_frame, g.grid, g.threads, g.lds_bytes);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "fuzz")) {
        const long n = atol(argv[2]);
        rng_state = 0x9E3779B97F4A7C15ull ^ (uint64_t)atol(argv[3]);
        long accepted = 0, refused = 0, failed = 0, reasons[9] = {0}, b_accepted = 0, b_refused = 0, b_reasons[11] = {0};
        const float alphas[] = {1.0f, 0.25f, 0.5f, 1.0e-6f, 0.0f, -0.25f, 1.0000001f, 2.0f, NAN, INFINITY, -INFINITY};
        for (long it = 0; it < n; it++) {
            // mostly valid values, each field wrong now and then
            Args a;
            a.mode = (rnd() % 24 == 0) ? (int)(rnd() % 7) - 1 : 1;
            a.iq = (rnd() % 24 == 0) ? (uintptr_t)(rnd() % 3) * 4 : 0x100000 + ((rnd() % 24 == 0) ? 4 : 8) * (uintptr_t)(rnd() % 4096);
            a.nf = (rnd() % 16 == 0) ? ((size_t)1 << 24) + (rnd() % 3) - 1 : (size_t)(rnd() % 5000);
            a.off = (rnd() % 32 == 0) ? ((size_t)1 << 40) + (rnd() % 3) - 1 : (size_t)(rnd() % 300000);
            a.alpha = alphas[(rnd() % 12 == 0) ? 4 + rnd() % 7 : rnd() % 4];
            for (int i = 0; i < 9; i++)
                a.p[i] = (rnd() % (i < 4 ? 2 : 3) == 0) ? 0 : 0x40000000 * (uintptr_t)(i + 1) + ((rnd() % 70 == 0) ? 1 + (uintptr_t)(rnd() % 3) : 4 * (uintptr_t)(rnd() % 4096));
            if (a.p[3] && rnd() % 4 == 0) {                                        // the state next to itself: in place, or overlapping by some floats
                const uint64_t pick = rnd() % 4;
                const uintptr_t bytes = (uintptr_t)a.nf * 512;
                a.p[4] = pick == 0 ? a.p[3] : pick == 1 ? a.p[3] + 4 * (uintptr_t)(1 + rnd() % 200) : pick == 2 ? a.p[3] + bytes : a.p[3] + bytes - 4;
            }
            const size_t need = a.off + 2656 + (a.p[0] ? 1543 : 0);
            const uint64_t pick = rnd() % 8;
            a.stride = pick == 0 ? need - 1 - (size_t)(rnd() % 3000) % need : pick == 1 ? need : pick == 2 ? ((size_t)1 << 40) + (rnd() % 3) - 1 : need + (size_t)(rnd() % 200000);
            dabgpu_noise_geometry g;
            memset(&g, 0xEE, sizeof(g));
            const int st = call(a, &g);
            const char* want = expect(a);
            bool ok;
            if (want) {
                ok = st == DABGPU_ERR_INVALID_ARG && strstr(dabgpu_last_error(), want) && g.grid == 0 && g.threads == 0 && g.lds_bytes == 0;
                refused++;
                for (int r = 0; r < 9; r++) if (!strcmp(want, WORDS[r])) reasons[r]++;
            } else {
                ok = st == DABGPU_OK && g.grid == a.nf && g.threads == 256 && g.lds_bytes == 18432 + 8192 + 8;
                accepted++;
            }
            if (!ok) { failed++; if (failed < 5) fprintf(stderr, "case %ld: status %d error '%s' expected '%s'\n", it, st, dabgpu_last_error(), want ? want : "ok"); }

            Banded b;
            memset(&b, 0, sizeof(b));
            b.n = (rnd() % 24 == 0) ? (int)(rnd() % 3) * 9 - 9 + (int)(rnd() % 2) * 9 : 1 + (int)(rnd() % 8);
            if (b.n > 9) b.n = 9;
            b.nf = (rnd() % 24 == 0) ? ((size_t)1 << 24) + (rnd() % 3) - 1 : (size_t)(rnd() % 5000);
            b.bits = (rnd() % 24 == 0) ? (uintptr_t)(rnd() % 2) * 8 : 0x8000000 + 16 * (uintptr_t)(rnd() % 4096);
            b.stride = (rnd() % 3 == 0) ? 0 : (rnd() % 16 == 0) ? 230400 - 16 + (rnd() % 3) * 8 : 230400 + 16 * (size_t)(rnd() % 100);
            b.layout = (rnd() % 24 == 0) ? (int)(rnd() % 5) - 2 : (int)(rnd() % 2);
            b.spb = (rnd() % 24 == 0) ? (int)(rnd() % 3) * 77 - 1 : (int)(rnd() % 76);
            b.null_bands = rnd() % 8 == 0;
            for (int i = 0; i < 9; i++) {
                b.br[i].d_dqpsk = (rnd() % 100 == 0) ? nullptr : (const float*)(0x10000000 * (uintptr_t)(i + 1) + ((rnd() % 100 == 0) ? 8 : 16) * (uintptr_t)(rnd() % 64));
                b.br[i].d_scale = (rnd() % 100 == 0) ? nullptr : (const float*)(0x1000000 + ((rnd() % 100 == 0) ? 2 : 4) * (uintptr_t)(1 + rnd() % 64));
                const bool banded = rnd() % 2;
                b.band[i] = banded ? (const float*)(0x2000000 * (uintptr_t)(i + 1) + ((rnd() % 50 == 0) ? 2 : 4) * (uintptr_t)(rnd() % 64)) : nullptr;
                b.br[i].d_weight = ((banded || b.null_bands) ? rnd() % 30 == 0 : rnd() % 2) ? (const float*)(0x3000000 + 4 * (uintptr_t)(rnd() % 64)) : nullptr;
                b.br[i].d_sync = (rnd() % 2) ? (const dabgpu_sync_state*)(0x4000000 + 4 * (uintptr_t)(rnd() % 64)) : nullptr;
            }
            dabgpu_diversity_geometry dg;
            memset(&dg, 0xEE, sizeof(dg));
            const int bst = call(b, &dg);
            const char* bwant = expect(b);
            if (bwant) {
                ok = bst == DABGPU_ERR_INVALID_ARG && strstr(dabgpu_last_error(), bwant) && dg.grid == 0 && dg.threads == 0 && dg.lds_bytes == 0;
                b_refused++;
                for (int r = 0; r < 11; r++) if (!strcmp(bwant, BWORDS[r])) b_reasons[r]++;
            } else {
                ok = bst == DABGPU_OK && dg.threads == 256 && dg.grid == b.nf * dg.runs_per_frame && dg.lds_bytes == (any_band(b) ? 6208u : 6144u) &&
                     dg.symbols_per_block >= 1 && dg.runs_per_frame == (75 + dg.symbols_per_block - 1) / dg.symbols_per_block;
                b_accepted++;
            }
            if (!ok) { failed++; if (failed < 5) fprintf(stderr, "banded case %ld: status %d error '%s' expected '%s'\n", it, bst, dabgpu_last_error(), bwant ? bwant : "ok"); }
        }
        printf("{\"checked\": %ld, \"accepted\": %ld, \"refused\": %ld, \"failed_checks\": %ld, \"reasons\": [", n, accepted, refused, failed);
        for (int r = 0; r < 9; r++) printf("%ld%s", reasons[r], r < 8 ? ", " : "");
        printf("], \"banded_accepted\": %ld, \"banded_refused\": %ld, \"banded_reasons\": [", b_accepted, b_refused);
        for (int r = 0; r < 11; r++) printf("%ld%s", b_reasons[r], r < 10 ? ", " : "");
        printf("]}\n");
        return failed ? 1 : 0;
    }
    if (argc == 2 && !strcmp(argv[1], "bands")) {
        float C[1536], prof[128], bw[128], mean;
        uint32_t ex[48];
        long bad = 0;
        const float vals[] = {0.0f, 1.0f, 3.0e-38f, 1.0e-45f, 3.0e38f, INFINITY, NAN, -1.0f, 5000.0f};
        rng_state = 78;
        for (float v : vals)
            for (float p : vals)
                for (int rep = 0; rep < 4; rep++) {
                    for (int i = 0; i < 1536; i++) C[i] = (rep == 0 || rnd() % 3) ? v : (float)(rnd() % 1000);
                    for (int i = 0; i < 128; i++) prof[i] = (rnd() % 3) ? p : (float)(rnd() % 10);
                    for (int i = 0; i < 48; i++) ex[i] = rep == 1 ? 0xFFFFFFFFu : rep == 2 ? (uint32_t)rnd() : 0u;
                    float keep[128];
                    memcpy(keep, prof, sizeof(keep));
                    const int ok = dabgpu_noise_profile_bands_host(C, rep ? ex : nullptr, rep == 3 ? nullptr : prof, 0.25f, prof, bw, &mean);
                    if (ok == 1) {
                        bad += !(mean >= 1.17549435e-38f && isfinite(mean));
                        for (int i = 0; i < 128; i++) bad += !(bw[i] > 0.0f);                 // (+infinity where M 2^-20 is below the normal range)
                    } else {
                        bad += ok != 0 || mean != 0.0f;
                        for (int i = 0; i < 128; i++) bad += bw[i] != 0.0f || memcmp(&prof[i], rep == 3 ? &bw[i] : &keep[i], 4) != 0;
                    }
                    bad += !(dabgpu_diversity_band_mean_host(bw) >= 0.0f);
                }
        bad += dabgpu_noise_profile_bands_host(nullptr, nullptr, nullptr, 1.0f, prof, bw, &mean) != -1;
        bad += dabgpu_noise_profile_bands_host(C, nullptr, nullptr, NAN, prof, bw, &mean) != -1;
        bad += dabgpu_noise_profile_bands_host(C, nullptr, nullptr, 1.0f, nullptr, nullptr, nullptr) < 0;
        const uint8_t mains[3] = {0, 69, 33}, subs[3] = {0, 23, 11}, wrong[1] = {70};
        bad += dabgpu_noise_profile_exclude_tii(mains, subs, 3, ex) != DABGPU_OK;
        int bits = 0;
        for (int i = 0; i < 48; i++) bits += __builtin_popcount(ex[i]);
        bad += bits != 96;
        bad += dabgpu_noise_profile_exclude_tii(wrong, subs, 1, ex) != DABGPU_ERR_INVALID_ARG;
        bad += dabgpu_noise_profile_exclude_tii(nullptr, nullptr, 0, ex) != DABGPU_OK || ex[0] != 0;
        bad += dabgpu_noise_profile_exclude_tii(mains, subs, 3, nullptr) != DABGPU_ERR_INVALID_ARG;
        bad += dabgpu_diversity_band_mean_host(nullptr) != 0.0f;
        printf("{\"failed_checks\": %ld}\n", bad);
        return bad ? 1 : 0;
    }
    fprintf(stderr, "usage: see the head of tests/cpp/noise_profile_plan_fuzz.cpp\n");
    return 2;
}
