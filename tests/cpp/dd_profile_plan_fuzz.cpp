// Driver of the decision-directed noise profile's planner (dabgpu_dd_profile_plan, dab-radio_amd/csrc/dabgpu_host_logic.cpp) for
// tests/test_dd_profile_plan.py: a program of its own, built plain and under -fsanitize=address,undefined.  The planner dereferences no
// address it is handed, so the addresses here are made up.
//   plan <mode> <dqpsk> <n_frames> <alpha> <sync> <exclude> <profile_in> <profile_out> <band_weight> <mean> <carrier_noise> <carrier_amplitude>
//        <valid> [null_out]                                       one call, as JSON
//   fuzz <n> <seed>             random arguments against the rules restated below
//   frames                      dabgpu_dd_profile_carriers_host and dabgpu_noise_profile_bands_host on a few frames (under the sanitizers too)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "dabgpu.h"

static std::string esc(const char* s) { std::string o; for (; *s; s++) { if (*s == '"' || *s == '\\') o += '\\'; o += *s; } return o; }

// p: sync, exclude, profile_in, profile_out, band_weight, mean, carrier_noise, carrier_amplitude, valid
struct Args { int mode; uintptr_t dq; size_t nf; float alpha; uintptr_t p[9]; };

static int call(const Args& a, dabgpu_noise_geometry* g) {
    return dabgpu_dd_profile_plan(a.mode, (const float*)a.dq, a.nf, (const dabgpu_sync_state*)a.p[0], (const uint32_t*)a.p[1], (const float*)a.p[2], a.alpha,
                                  (const float*)a.p[3], (const float*)a.p[4], (const float*)a.p[5], (const float*)a.p[6], (const float*)a.p[7],
                                  (const uint32_t*)a.p[8], g);
}

// the rules, restated: 0 = accepted, else a word of the reason the message must contain
static const char* expect(const Args& a) {
    if (a.mode != 1) return "mode";
    if (a.nf == 0 || a.nf > (size_t)1 << 24) return "n_frames";
    if (!a.dq) return "null products";
    if (a.dq % 16) return "16-byte";
    for (int i = 0; i < 9; i++) if (i != 6 && i != 7 && a.p[i] % 4) return "4-byte";
    if (a.p[6] % 8 || a.p[7] % 8) return "8-byte";
    if (!(a.alpha > 0.0f && a.alpha <= 1.0f)) return "alpha";
    if (a.p[2] && a.p[3] && a.p[2] != a.p[3]) {
        const uintptr_t bytes = (uintptr_t)a.nf * 512;
        if (a.p[2] < a.p[3] + bytes && a.p[3] < a.p[2] + bytes) return "overlap";
    }
    if (!a.p[3] && !a.p[4] && !a.p[5] && !a.p[6] && !a.p[7] && !a.p[8]) return "no output";
    return nullptr;
}

static uint64_t rng_state;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static const int N_WORDS = 9;
static const char* const WORDS[N_WORDS] = {"mode", "n_frames", "null products", "16-byte", "4-byte", "8-byte", "alpha", "overlap", "no output"};

int main(int argc, char** argv) {
    if (argc >= 15 && !strcmp(argv[1], "plan")) {
        Args a;
        a.mode = atoi(argv[2]);
        a.dq = (uintptr_t)strtoull(argv[3], nullptr, 0);
        a.nf = (size_t)strtoull(argv[4], nullptr, 0);
        a.alpha = strtof(argv[5], nullptr);
        for (int i = 0; i < 9; i++) a.p[i] = (uintptr_t)strtoull(argv[6 + i], nullptr, 0);
        dabgpu_noise_geometry g;
        memset(&g, 0xEE, sizeof(g));
        const bool null_out = argc >= 16 && atoi(argv[15]);
        const int st = call(a, null_out ? nullptr : &g);
        printf("{\"status\": %d, \"error\": \"%s\", \"grid\": %u, \"threads\": %u, \"lds_bytes\": %u}\n", st, st ? esc(dabgpu_last_error()).c_str() : "", g.grid,
               g.threads, g.lds_bytes);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "fuzz")) {
        const long n = atol(argv[2]);
        rng_state = 0x9E3779B97F4A7C15ull ^ (uint64_t)atol(argv[3]);
        long accepted = 0, refused = 0, failed = 0, reasons[N_WORDS] = {0};
        const float alphas[] = {1.0f, 0.25f, 0.5f, 1.0e-6f, 0.0f, -0.25f, 1.0000001f, 2.0f, NAN, INFINITY, -INFINITY};
        for (long it = 0; it < n; it++) {
            // mostly valid values, each field wrong now and then
            Args a;
            a.mode = (rnd() % 24 == 0) ? (int)(rnd() % 7) - 1 : 1;
            a.dq = (rnd() % 24 == 0) ? (uintptr_t)(rnd() % 3) * 8 : 0x100000 + ((rnd() % 16 == 0) ? 4 : 16) * (uintptr_t)(rnd() % 4096);
            a.nf = (rnd() % 16 == 0) ? ((size_t)1 << 24) + (rnd() % 3) - 1 : (size_t)(rnd() % 5000);
            a.alpha = alphas[(rnd() % 12 == 0) ? 4 + rnd() % 7 : rnd() % 4];
            for (int i = 0; i < 9; i++)
                a.p[i] = (rnd() % (i < 3 ? 2 : 3) == 0) ? 0 : 0x40000000 * (uintptr_t)(i + 1) + ((rnd() % 70 == 0) ? 1 + (uintptr_t)(rnd() % 7) : 8 * (uintptr_t)(rnd() % 4096));
            if (a.p[2] && rnd() % 4 == 0) {                                        // the state next to itself: in place, or overlapping by some floats
                const uint64_t pick = rnd() % 4;
                const uintptr_t bytes = (uintptr_t)a.nf * 512;
                a.p[3] = pick == 0 ? a.p[2] : pick == 1 ? a.p[2] + 4 * (uintptr_t)(1 + rnd() % 200) : pick == 2 ? a.p[2] + bytes : a.p[2] + bytes - 4;
            }
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
                ok = st == DABGPU_OK && g.grid == (uint32_t)a.nf && g.threads == 256 && g.lds_bytes == 6152;
                accepted++;
            }
            if (!ok) {
                failed++;
                if (failed < 10) fprintf(stderr, "iteration %ld: want %s, status %d (%s), grid %u\n", it, want ? want : "ok", st, dabgpu_last_error(), g.grid);
            }
        }
        printf("{\"checked\": %ld, \"accepted\": %ld, \"refused\": %ld, \"failed_checks\": %ld, \"reasons\": [", n, accepted, refused, failed);
        for (int r = 0; r < N_WORDS; r++) printf("%s%ld", r ? ", " : "", reasons[r]);
        printf("]}\n");
        return failed ? 1 : 0;
    }
    if (argc == 2 && !strcmp(argv[1], "frames")) {
        // the host forms on exactly sized heap blocks: a read or write past a frame is the sanitizer's to find
        const size_t n = (size_t)75 * 1536 * 2;
        long failed = 0;
        for (int kind = 0; kind < 4; kind++) {
            std::vector<float> dq(n), Q(1536, -1.0f), A(1536, -1.0f), prof(128, 0.0f), bw(128, -1.0f);
            rng_state = 0x1234567ull + (uint64_t)kind;
            for (size_t i = 0; i < n; i++) dq[i] = kind == 1 ? 0.0f : ((float)(int64_t)(rnd() % 2001) - 1000.0f) * 37.0f;
            if (kind == 2) { dq[5] = NAN; dq[9000] = INFINITY; dq[n - 1] = -INFINITY; }
            if (dabgpu_dd_profile_carriers_host(dq.data(), kind == 3 ? nullptr : Q.data(), A.data()) != 0) failed++;
            if (dabgpu_dd_profile_carriers_host(nullptr, Q.data(), A.data()) != -1) failed++;
            if (kind == 3) continue;
            float mean = -1.0f;
            uint32_t ex[48];
            for (int i = 0; i < 48; i++) ex[i] = (uint32_t)rnd();
            const int ok = dabgpu_noise_profile_bands_host(Q.data(), ex, prof.data(), 0.25f, prof.data(), bw.data(), &mean);
            if (ok != (kind == 1 ? 0 : 1)) failed++;
            for (int c = 0; c < 1536; c++) if (!(Q[c] >= 0.0f)) failed++;
            for (int b = 0; b < 128; b++) if (ok ? !(bw[b] > 0.0f) : bw[b] != 0.0f) failed++;
        }
        printf("{\"failed_checks\": %ld}\n", failed);
        return failed ? 1 : 0;
    }
    fprintf(stderr, "usage: see the head of tests/cpp/dd_profile_plan_fuzz.cpp\n");
    return 2;
}
