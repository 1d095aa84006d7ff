// Driver of the noise estimator's planner (dabgpu_noise_plan, dab-radio_amd/csrc/dabgpu_host_logic.cpp) for tests/test_noise_plan.py: a
// program of its own, built plain and under -fsanitize=address,undefined.  The planner dereferences no address it is handed, so the
// addresses here are made up.
//   plan <mode> <iq> <n_frames> <stride> <null_offset> <states> <freq> <noise> <signal> <weight> <snr> <energy> <valid> [null_out]   one call, as JSON
//   fuzz <n> <seed>             random arguments against the rules restated below
//   floor                       dabgpu_noise_floor_host on a few tables (the host form runs under the sanitizers too)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include "dabgpu.h"

static std::string esc(const char* s) { std::string o; for (; *s; s++) { if (*s == '"' || *s == '\\') o += '\\'; o += *s; } return o; }

struct Args { int mode; uintptr_t iq; size_t nf, stride, off; uintptr_t p[8]; };      // p: states, freq, noise, signal, weight, snr, energy, valid

static int call(const Args& a, dabgpu_noise_geometry* g) {
    return dabgpu_noise_plan(a.mode, (const float*)a.iq, a.nf, a.stride, a.off, (const dabgpu_sync_state*)a.p[0], (const float*)a.p[1], (const float*)a.p[2],
                             (const float*)a.p[3], (const float*)a.p[4], (const float*)a.p[5], (const float*)a.p[6], (const uint32_t*)a.p[7], g);
}

// the rules, restated: 0 = accepted, else a word of the reason the message must contain
static const char* expect(const Args& a) {
    if (a.mode != 1) return "mode";
    if (a.nf == 0 || a.nf > (size_t)1 << 24) return "n_frames";
    if (!a.iq) return "null samples";
    if (a.iq % 8) return "8-byte";
    for (int i = 0; i < 8; i++) if (a.p[i] % 4) return "4-byte";
    const size_t lim = (size_t)1 << 40;
    if (a.off > lim || a.stride > lim || a.stride < a.off + 2656 + 2552 + (a.p[0] ? 1543 : 0)) return "stream_stride_samples";
    if (!a.p[2] && !a.p[3] && !a.p[4] && !a.p[5] && !a.p[6] && !a.p[7]) return "no output";
    return nullptr;
}

static uint64_t rng_state;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

int main(int argc, char** argv) {
    if (argc >= 15 && !strcmp(argv[1], "plan")) {
        Args a;
        a.mode = atoi(argv[2]);
        a.iq = (uintptr_t)strtoull(argv[3], nullptr, 0);
        a.nf = (size_t)strtoull(argv[4], nullptr, 0); a.stride = (size_t)strtoull(argv[5], nullptr, 0); a.off = (size_t)strtoull(argv[6], nullptr, 0);
        for (int i = 0; i < 8; i++) a.p[i] = (uintptr_t)strtoull(argv[7 + i], nullptr, 0);
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
        long accepted = 0, refused = 0, failed = 0;
        long reasons[7] = {0};
        static const char* const WORDS[7] = {"mode", "n_frames", "null samples", "8-byte", "4-byte", "stream_stride_samples", "no output"};
        for (long it = 0; it < n; it++) {
            // mostly valid values, each field wrong now and then
            Args a;
            a.mode = (rnd() % 24 == 0) ? (int)(rnd() % 7) - 1 : 1;
            a.iq = (rnd() % 24 == 0) ? (uintptr_t)(rnd() % 3) * 4 : 0x100000 + ((rnd() % 24 == 0) ? 4 : 8) * (uintptr_t)(rnd() % 4096);
            a.nf = (rnd() % 16 == 0) ? ((size_t)1 << 24) + (rnd() % 3) - 1 : (size_t)(rnd() % 5000);
            a.off = (rnd() % 32 == 0) ? ((size_t)1 << 40) + (rnd() % 3) - 1 : (size_t)(rnd() % 300000);
            for (int i = 0; i < 8; i++)
                a.p[i] = (rnd() % (i < 2 ? 2 : 3) == 0) ? 0 : 0x200000 * (uintptr_t)(i + 1) + ((rnd() % 60 == 0) ? 1 + (uintptr_t)(rnd() % 3) : 4 * (uintptr_t)(rnd() % 4096));
            const size_t need = a.off + 2656 + 2552 + (a.p[0] ? 1543 : 0);
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
                for (int r = 0; r < 7; r++) if (!strcmp(want, WORDS[r])) reasons[r]++;
            } else {
                ok = st == DABGPU_OK && g.grid == a.nf && g.threads == 256 && g.lds_bytes == 27508;
                accepted++;
            }
            if (!ok) { failed++; if (failed < 5) fprintf(stderr, "case %ld: status %d error '%s' expected '%s'\n", it, st, dabgpu_last_error(), want ? want : "ok"); }
        }
        printf("{\"checked\": %ld, \"accepted\": %ld, \"refused\": %ld, \"failed_checks\": %ld, \"reasons\": [", n, accepted, refused, failed);
        for (int r = 0; r < 7; r++) printf("%ld%s", reasons[r], r < 6 ? ", " : "");
        printf("]}\n");
        return failed ? 1 : 0;
    }
    if (argc == 2 && !strcmp(argv[1], "floor")) {
        float E[192];
        dabgpu_noise_record rec;
        long bad = 0;
        const float vals[] = {0.0f, 1.0f, 3.0e-38f, 1.0e-45f, 3.0e38f, INFINITY, NAN, -1.0f};
        const float powers[] = {0.0f, 1.0e-44f, 1.0e-30f, 1.0f, 4096.0f, 3.0e38f, INFINITY, NAN, -5.0f};
        rng_state = 77;
        for (float v : vals)
            for (float P : powers)
                for (int rep = 0; rep < 4; rep++) {
                    for (int i = 0; i < 192; i++) E[i] = (rep == 0 || rnd() % 3) ? v : (float)(rnd() % 1000);
                    const int ok = dabgpu_noise_floor_host(E, P, &rec);
                    const bool zero = rec.noise_power == 0 && rec.signal_power == 0 && rec.weight == 0 && rec.snr == 0 && rec.valid == 0;
                    if (ok ? !(rec.valid == 1 && isfinite(rec.weight) && rec.weight > 0 && isfinite(rec.noise_power) && rec.signal_power == P && rec.snr >= 0)
                           : !zero) bad++;
                }
        bad += dabgpu_noise_floor_host(nullptr, 1.0f, &rec) != 0;
        bad += dabgpu_noise_floor_host(E, 1.0f, nullptr) != 0;
        printf("{\"failed_checks\": %ld, \"unbias\": %.9g}\n", bad, (double)dabgpu_noise_unbias());
        return bad ? 1 : 0;
    }
    fprintf(stderr, "usage: see the head of tests/cpp/noise_plan_fuzz.cpp\n");
    return 2;
}
