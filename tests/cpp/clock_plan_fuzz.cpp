// Driver of the sampling-clock tracker's two planners (dabgpu_clock_estimate_plan, dabgpu_clock_derotate_plan,
// dab-radio_amd/csrc/dabgpu_host_logic.cpp) for tests/test_clock_plan.py: a program of its own, built plain and under
// -fsanitize=address,undefined.  The planners dereference no device address they are handed, so the addresses here are made up.
//   eplan <mode> <dqpsk> <n_frames> <sync> <slope_in> <gain> <slope_out> <residual> <corr> <valid> [null_out]      one call, as JSON
//   dplan <mode> <in> <out> <n_frames> <sync> <slope> <spb> [null_out]                                           one call, as JSON
//   fuzz <n> <seed>             random arguments of both planners against the rules restated below
//   frames                      the host forms on a few frames (under the sanitizers too)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "dabgpu.h"

static std::string esc(const char* s) { std::string o; for (; *s; s++) { if (*s == '"' || *s == '\\') o += '\\'; o += *s; } return o; }

// p: sync, slope_in, slope_out, residual, corr, valid
struct EArgs { int mode; uintptr_t dq; size_t nf; float gain; uintptr_t p[6]; };

static int ecall(const EArgs& a, dabgpu_noise_geometry* g) {
    return dabgpu_clock_estimate_plan(a.mode, (const float*)a.dq, a.nf, (const dabgpu_sync_state*)a.p[0], (const int64_t*)a.p[1], a.gain,
                                      (const int64_t*)a.p[2], (const int64_t*)a.p[3], (const float*)a.p[4], (const uint32_t*)a.p[5], g);
}
static bool overlap(uintptr_t a, uintptr_t b, uintptr_t bytes) { return a != b && a < b + bytes && b < a + bytes; }

// the rules, restated: 0 = accepted, else a word of the reason the message must contain
static const char* eexpect(const EArgs& a) {
    if (a.mode != 1) return "mode";
    if (a.nf == 0 || a.nf > (size_t)1 << 24) return "n_frames";
    if (!a.dq) return "null products";
    if (a.dq % 16) return "16-byte";
    if (a.p[1] % 8 || a.p[2] % 8 || a.p[3] % 8) return "8-byte";
    if (a.p[0] % 4 || a.p[4] % 4 || a.p[5] % 4) return "4-byte";
    if (!(a.gain > 0.0f && a.gain <= 1.0f)) return "gain";
    if (a.p[1] && a.p[2] && overlap(a.p[1], a.p[2], a.nf * 8)) return "overlap";
    if (!a.p[2] && !a.p[3] && !a.p[4] && !a.p[5]) return "no output";
    return nullptr;
}

struct DArgs { int mode; uintptr_t in, out; size_t nf; uintptr_t sync, slope; int spb; };

static int dcall(const DArgs& a, dabgpu_diversity_geometry* g) {
    return dabgpu_clock_derotate_plan(a.mode, (const float*)a.in, (const float*)a.out, a.nf, (const dabgpu_sync_state*)a.sync, (const int64_t*)a.slope,
                                      a.spb, g);
}
static const char* dexpect(const DArgs& a) {
    if (a.mode != 1) return "mode";
    if (a.nf == 0 || a.nf > (size_t)1 << 24) return "n_frames";
    if (!a.in || !a.out) return "null products";
    if (a.in % 16 || a.out % 16) return "16-byte";
    if (overlap(a.in, a.out, a.nf * 921600)) return "overlap";
    if (!a.slope) return "null slope";
    if (a.slope % 8) return "8-byte";
    if (a.sync % 4) return "4-byte";
    if (a.spb < 0 || a.spb > 75) return "symbols_per_block";
    return nullptr;
}
// the run length of symbols_per_block = 0: the combiner's small-batch rule
static unsigned auto_spb(size_t nf) {
    if (nf >= 86) return 25;
    size_t chunks = (256 + nf - 1) / nf;
    if (chunks > 25) chunks = 25;
    return (unsigned)((75 + chunks - 1) / chunks);
}

static uint64_t rng_state;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static uintptr_t addr(unsigned align, int odd) {                      // an address aligned to `align`, wrong one time in `odd`, null now and then
    if (rnd() % 6 == 0) return 0;
    uintptr_t a = ((uintptr_t)(rnd() % (1u << 20)) + 1) * 4096;
    if (rnd() % odd == 0) a += (uintptr_t)(rnd() % align);
    return a;
}

static const int N_EWORDS = 9, N_DWORDS = 9;
static const char* const EWORDS[N_EWORDS] = {"mode", "n_frames", "null products", "16-byte", "8-byte", "4-byte", "gain", "overlap", "no output"};
static const char* const DWORDS[N_DWORDS] = {"mode", "n_frames", "null products", "16-byte", "overlap", "null slope", "8-byte", "4-byte", "symbols_per_block"};

static int frames_check() {
    long failed = 0;
    std::vector<float> d(75 * 1536 * 2), out(75 * 1536 * 2);
    rng_state = 12345;
    // unit products at 45 degrees with a ramp of 200 ppm: 200e-6 * 2552 / 2048 cycles per carrier
    const double theta = 200e-6 * 2552.0 / 2048.0;
    for (int s = 0; s < 75; s++)
        for (int c = 0; c < 1536; c++) {
            const int k = c < 768 ? c - 768 : c - 767;
            const double ph = 2.0 * M_PI * (0.125 + 0.25 * (double)(rnd() % 4) - theta * k);      // X[s] conj(X[s + 1]): the ramp runs down
            d[2 * (s * 1536 + c)] = (float)(100.0 * cos(ph)); d[2 * (s * 1536 + c) + 1] = (float)(100.0 * sin(ph));
        }
    int64_t slope = 0;
    float corr[2];
    if (dabgpu_clock_estimate_host(d.data(), 0, 1.0f, &slope, corr) != 1) failed++;
    if (fabs(dabgpu_clock_ppm(slope) - 200.0) > 0.2) failed++;
    if (llabs(dabgpu_clock_slope_q64(200.0) - slope) > dabgpu_clock_slope_q64(0.2)) failed++;
    if (dabgpu_clock_derotate_host(d.data(), out.data(), slope) != 0) failed++;
    int64_t left = 0;
    if (dabgpu_clock_estimate_host(out.data(), 0, 0.5f, &left, nullptr) != 1 || fabs(dabgpu_clock_ppm(left)) > 0.2) failed++;
    if (dabgpu_clock_derotate_host(out.data(), out.data(), -slope) != 0) failed++;                  // in place, back again
    for (size_t i = 0; i < d.size(); i++) if (fabsf(out[i] - d[i]) > 1e-3f) { failed++; break; }
    // the edges: a NaN frame, a zero frame, every slope word the clamp can meet, refusals
    std::vector<float> bad(d.size(), NAN), zero(d.size(), 0.0f);
    const int64_t words[] = {0, 1, -1, DABGPU_CLOCK_MAX_SLOPE, -DABGPU_CLOCK_MAX_SLOPE, INT64_MAX, INT64_MIN, INT64_MAX / 2, INT64_MIN / 2};
    for (int64_t w : words) {
        int64_t s = 7;
        if (dabgpu_clock_estimate_host(bad.data(), w, 1.0f, &s, corr) != 0 || s != w || corr[0] != 0.0f || corr[1] != 0.0f) failed++;
        if (dabgpu_clock_estimate_host(zero.data(), w, 0.25f, &s, nullptr) != 0 || s != w) failed++;
        if (dabgpu_clock_estimate_host(d.data(), w, 1.0f, &s, nullptr) != 1 || s > DABGPU_CLOCK_MAX_SLOPE || s < -DABGPU_CLOCK_MAX_SLOPE) failed++;
        if (dabgpu_clock_derotate_host(d.data(), out.data(), w) != 0) failed++;
    }
    if (dabgpu_clock_estimate_host(nullptr, 0, 1.0f, &slope, corr) != -1 || dabgpu_clock_estimate_host(d.data(), 0, 0.0f, &slope, corr) != -1 ||
        dabgpu_clock_estimate_host(d.data(), 0, NAN, &slope, corr) != -1 || dabgpu_clock_derotate_host(nullptr, out.data(), 0) != -1 ||
        dabgpu_clock_derotate_host(d.data(), nullptr, 0) != -1)
        failed++;
    const double ppms[] = {0.0, 1e-9, -1e-9, 1000.0, -1000.0, 1e12, -1e12, 1e300, -1e300, NAN, INFINITY, -INFINITY};
    for (double p : ppms) { const int64_t s = dabgpu_clock_slope_q64(p); (void)dabgpu_clock_ppm(s); }
    printf("{\"failed_checks\": %ld}\n", failed);
    return failed ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc >= 12 && !strcmp(argv[1], "eplan")) {
        EArgs a;
        a.mode = atoi(argv[2]);
        a.dq = (uintptr_t)strtoull(argv[3], nullptr, 0);
        a.nf = (size_t)strtoull(argv[4], nullptr, 0);
        a.p[0] = (uintptr_t)strtoull(argv[5], nullptr, 0); a.p[1] = (uintptr_t)strtoull(argv[6], nullptr, 0);
        a.gain = strtof(argv[7], nullptr);
        for (int i = 2; i < 6; i++) a.p[i] = (uintptr_t)strtoull(argv[6 + i], nullptr, 0);
        dabgpu_noise_geometry g;
        memset(&g, 0xEE, sizeof(g));
        const bool null_out = argc >= 13 && atoi(argv[12]);
        const int st = ecall(a, null_out ? nullptr : &g);
        printf("{\"status\": %d, \"error\": \"%s\", \"grid\": %u, \"threads\": %u, \"lds_bytes\": %u}\n", st, st ? esc(dabgpu_last_error()).c_str() : "", g.grid,
               g.threads, g.lds_bytes);
        return 0;
    }
    if (argc >= 9 && !strcmp(argv[1], "dplan")) {
        DArgs a;
        a.mode = atoi(argv[2]); a.in = (uintptr_t)strtoull(argv[3], nullptr, 0); a.out = (uintptr_t)strtoull(argv[4], nullptr, 0);
        a.nf = (size_t)strtoull(argv[5], nullptr, 0); a.sync = (uintptr_t)strtoull(argv[6], nullptr, 0); a.slope = (uintptr_t)strtoull(argv[7], nullptr, 0);
        a.spb = atoi(argv[8]);
        dabgpu_diversity_geometry g;
        memset(&g, 0xEE, sizeof(g));
        const bool null_out = argc >= 10 && atoi(argv[9]);
        const int st = dcall(a, null_out ? nullptr : &g);
        printf("{\"status\": %d, \"error\": \"%s\", \"grid\": %u, \"threads\": %u, \"lds_bytes\": %u, \"symbols_per_block\": %u, \"runs_per_frame\": %u}\n", st,
               st ? esc(dabgpu_last_error()).c_str() : "", g.grid, g.threads, g.lds_bytes, g.symbols_per_block, g.runs_per_frame);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "fuzz")) {
        const long n = atol(argv[2]);
        rng_state = 0x9E3779B97F4A7C15ull ^ (uint64_t)atol(argv[3]);
        long accepted = 0, refused = 0, failed = 0, reasons[N_EWORDS] = {0}, daccepted = 0, drefused = 0, dreasons[N_DWORDS] = {0};
        const float gains[] = {1.0f, 0.5f, 1e-6f, 0.0f, -0.5f, 1.0000001f, 2.0f, NAN, INFINITY, -0.0f, 1e-45f};
        for (long it = 0; it < n; it++) {
            // mostly valid values, each field wrong now and then
            EArgs a;
            a.mode = (rnd() % 24 == 0) ? (int)(rnd() % 7) - 1 : 1;
            a.nf = (rnd() % 16 == 0) ? (size_t)(rnd() % 3 == 0 ? 0 : ((size_t)1 << 24) + rnd() % 3) : 1 + (size_t)(rnd() % 5000);
            a.dq = (rnd() % 24 == 0) ? 0 : (((uintptr_t)(rnd() % (1u << 20)) + 1) * 4096 + (rnd() % 12 == 0 ? rnd() % 16 : 0));
            a.gain = (rnd() % 4 == 0) ? gains[rnd() % 11] : (float)((rnd() % 1000) + 1) * 1e-3f;
            a.p[0] = addr(4, 20);
            a.p[1] = addr(8, 20); a.p[2] = addr(8, 20); a.p[3] = addr(8, 20);
            a.p[4] = addr(4, 20); a.p[5] = addr(4, 20);
            if (a.p[1] && rnd() % 3 == 0) a.p[2] = a.p[1] + (rnd() % 2 ? 0 : 8 * (uintptr_t)(rnd() % (2 * a.nf + 1)));      // in place, or nearby
            dabgpu_noise_geometry g;
            memset(&g, 0xEE, sizeof(g));
            const int st = ecall(a, &g);
            const char* want = eexpect(a);
            if (!want) {
                accepted++;
                if (st != 0 || g.grid != a.nf || g.threads != 256 || g.lds_bytes != 48) { failed++; fprintf(stderr, "accepting call failed: %s\n", dabgpu_last_error()); }
            } else {
                refused++;
                for (int i = 0; i < N_EWORDS; i++) if (!strcmp(want, EWORDS[i])) reasons[i]++;
                if (st != DABGPU_ERR_INVALID_ARG || !strstr(dabgpu_last_error(), want) || g.grid || g.threads || g.lds_bytes) {
                    failed++; fprintf(stderr, "expected '%s', got %d '%s'\n", want, st, dabgpu_last_error());
                }
            }
            DArgs d;
            d.mode = (rnd() % 24 == 0) ? (int)(rnd() % 7) - 1 : 1;
            d.nf = (rnd() % 16 == 0) ? (size_t)(rnd() % 3 == 0 ? 0 : ((size_t)1 << 24) + rnd() % 3) : 1 + (size_t)(rnd() % 300);
            d.in = (rnd() % 24 == 0) ? 0 : (((uintptr_t)(rnd() % (1u << 20)) + 1) * 4096 + (rnd() % 16 == 0 ? rnd() % 16 : 0));
            const int how = (int)(rnd() % 8);
            d.out = how < 3 ? d.in : how == 3 ? d.in + 16 * (uintptr_t)(rnd() % (57600 * d.nf + 2)) : how == 4 ? 0
                  : (((uintptr_t)(rnd() % (1u << 20)) + (1u << 21)) * 4096 * 64 + (rnd() % 16 == 0 ? rnd() % 16 : 0));
            d.sync = addr(4, 20);
            d.slope = rnd() % 20 == 0 ? 0 : (((uintptr_t)(rnd() % (1u << 20)) + 1) * 4096 + (rnd() % 16 == 0 ? rnd() % 8 : 0));
            d.spb = rnd() % 12 == 0 ? (int)(rnd() % 200) - 60 : (int)(rnd() % 76);
            dabgpu_diversity_geometry dg;
            memset(&dg, 0xEE, sizeof(dg));
            const int dst = dcall(d, &dg);
            const char* dwant = dexpect(d);
            if (!dwant) {
                daccepted++;
                const unsigned spb = d.spb ? (unsigned)d.spb : auto_spb(d.nf), runs = (75 + spb - 1) / spb;
                if (dst != 0 || dg.symbols_per_block != spb || dg.runs_per_frame != runs || dg.grid != d.nf * runs || dg.threads != 256 || dg.lds_bytes != 12288 ||
                    (uint64_t)spb * runs < 75) {
                    failed++; fprintf(stderr, "accepting de-rotator call failed: %s\n", dabgpu_last_error());
                }
            } else {
                drefused++;
                for (int i = 0; i < N_DWORDS; i++) if (!strcmp(dwant, DWORDS[i])) dreasons[i]++;
                if (dst != DABGPU_ERR_INVALID_ARG || !strstr(dabgpu_last_error(), dwant) || dg.grid || dg.threads || dg.lds_bytes || dg.symbols_per_block ||
                    dg.runs_per_frame) {
                    failed++; fprintf(stderr, "de-rotator: expected '%s', got %d '%s'\n", dwant, dst, dabgpu_last_error());
                }
            }
        }
        printf("{\"checked\": %ld, \"accepted\": %ld, \"refused\": %ld, \"failed_checks\": %ld, \"reasons\": [", n, accepted, refused, failed);
        for (int i = 0; i < N_EWORDS; i++) printf("%s%ld", i ? ", " : "", reasons[i]);
        printf("], \"derotate_accepted\": %ld, \"derotate_refused\": %ld, \"derotate_reasons\": [", daccepted, drefused);
        for (int i = 0; i < N_DWORDS; i++) printf("%s%ld", i ? ", " : "", dreasons[i]);
        printf("]}\n");
        return failed ? 1 : 0;
    }
    if (argc == 2 && !strcmp(argv[1], "frames")) return frames_check();
    fprintf(stderr, "usage: clock_plan_fuzz eplan ... | dplan ... | fuzz <n> <seed> | frames\n");
    return 2;
}
