// Driver of the demodulation planner's soft-decision policy (dabgpu_host_plan_demod / dabgpu_host_check_soft_cfg,
// dab-radio_amd/csrc/dabgpu_host_logic.cpp), built plain and with ASan + UBSan by tests/test_softbit_plan.py.
//   softbit_plan_driver all            every combination of the facts below with every policy and level of the lists, against the rules restated
//                                      here from their description; one JSON line of counters
//   softbit_plan_driver fuzz N SEED    N random calls (any integer as mode, loader, policy; any bit pattern as level) against the same rules
//   softbit_plan_driver plan MODE SRC DESC FFT DQPSK SYNC CLASSED SPB N_FRAMES GENERIC_MODE1 POLICY LEVEL      one plan as a JSON line
//   softbit_plan_driver cfg POLICY LEVEL                                                                      dabgpu_host_check_soft_cfg as a JSON line
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dabgpu_host_logic.h"

static long failed = 0;
#define CHECK(c) do { if (!(c)) { if (failed++ < 20) { fprintf(stderr, "check failed line %d: %s  ", __LINE__, #c); describe(mode, f); } } } while (0)

static void describe(int mode, const dabgpu_demod_facts& f) {
    fprintf(stderr, "[mode %d src %d desc %d fft %d dqpsk %d sync %d stride %d classed %d spb %d n %d generic_mode1 %d policy %d level %g]\n", mode, f.src, f.desc,
            f.fft, f.dqpsk, f.sync, f.frame_stride, f.classed, f.symbols_per_block, f.n_frames, f.generic_mode1, f.soft_policy, (double)f.soft_level);
}

struct counters { long checked, refused, normalised, weighted, bad_policy, not_mode1, bank, bad_level, earlier; long variant[12]; };

static void check_one(int mode, const dabgpu_demod_facts& f, counters& n) {
    const dabgpu_demod_plan p = dabgpu_host_plan_demod(mode, f);
    n.checked++;
    // what the planner refused before there was a policy (tests/cpp/demod_plan_driver.cpp) comes first and keeps its reason
    const bool valid_mode = mode >= 1 && mode <= 4;
    const bool mode1 = mode == 1 && !f.generic_mode1;
    const bool views = f.fft || f.dqpsk;
    const bool earlier = !valid_mode || (mode1 && (f.src < 0 || f.src > 3 || (f.classed && views) || (f.desc && (f.sync || f.frame_stride))));
    if (earlier) { CHECK(p.status == DABGPU_ERR_INVALID_ARG); n.earlier++; n.refused++; return; }
    const int layout = f.classed ? 2 : views ? 1 : 0;
    if (f.soft_policy == DABGPU_SOFT_NORMALISED) {
        // the level is not looked at, the numbers are the old ones
        CHECK(p.status == DABGPU_OK);
        if (mode1) { CHECK(p.variant == (f.src * 2 + (f.desc ? 1 : 0)) * 3 + layout); CHECK(p.variant < 24); }
        n.normalised++;
        return;
    }
    // the weighted policy: it exists, on the mode I kernel, without descriptors, with a level in [1, 127] (a NaN is outside) -- in this order
    const bool bad_policy = f.soft_policy != DABGPU_SOFT_CSI;
    const bool not_mode1 = !bad_policy && !mode1;
    const bool bank = !bad_policy && !not_mode1 && f.desc;
    const bool bad_level = !bad_policy && !not_mode1 && !bank && !(f.soft_level >= 1.0f && f.soft_level <= 127.0f);
    const bool refused = bad_policy || not_mode1 || bank || bad_level;
    CHECK((p.status == DABGPU_ERR_INVALID_ARG) == refused && (p.status == DABGPU_OK) == !refused);
    if (refused) {
        const char* e = dabgpu_last_error();
        CHECK(strstr(e, bad_policy ? "policy" : not_mode1 ? "mode I" : bank ? "bank" : "level") != nullptr);
        n.refused++; n.bad_policy += bad_policy; n.not_mode1 += not_mode1; n.bank += bank; n.bad_level += bad_level;
        return;
    }
    CHECK(p.family == DABGPU_DEMOD_MODE1);
    CHECK(p.variant == 24 + f.src * 3 + layout);
    CHECK(p.variant >= DABGPU_DEMOD_MODE1_NORMALISED_VARIANTS && p.variant < DABGPU_DEMOD_MODE1_VARIANTS);
    n.variant[p.variant - 24]++;
    n.weighted++;
    // everything else is the normalised call's: run length, grid, tail
    dabgpu_demod_facts g = f;
    g.soft_policy = DABGPU_SOFT_NORMALISED;
    const dabgpu_demod_plan q = dabgpu_host_plan_demod(mode, g);
    CHECK(q.status == DABGPU_OK && q.symbols_per_block == p.symbols_per_block && q.chunks == p.chunks && q.grid == p.grid && q.threads == p.threads &&
          q.lds_bytes == p.lds_bytes && q.tail == p.tail && q.fine_stride == p.fine_stride && q.family == p.family);
}

static void print_counters(const counters& n) {
    printf("{\"checked\": %ld, \"failed_checks\": %ld, \"refused\": %ld, \"earlier\": %ld, \"normalised\": %ld, \"weighted\": %ld, \"bad_policy\": %ld, "
           "\"not_mode1\": %ld, \"bank\": %ld, \"bad_level\": %ld, \"variants\": [", n.checked, failed, n.refused, n.earlier, n.normalised, n.weighted, n.bad_policy,
           n.not_mode1, n.bank, n.bad_level);
    for (int k = 0; k < 12; k++) printf("%ld%s", n.variant[k], k < 11 ? ", " : "]}\n");
}

static int run_all() {
    static const int POLICY[] = {0, 1, 2, -1};
    static const float LEVEL[] = {64.0f, 1.0f, 127.0f, 0.99f, 127.5f, 0.0f, -64.0f, NAN, INFINITY};
    static const int SPB[] = {0, 25, 75};
    counters n = {};
    for (int mode = 0; mode <= 5; mode++)
        for (int src = -1; src <= 4; src++)
            for (int bits = 0; bits < (1 << 9); bits++)
                for (int policy : POLICY)
                    for (float level : LEVEL)
                        for (int spb : SPB) {
                            dabgpu_demod_facts f;
                            f.src = src;
                            f.desc = bits & 1; f.fft = bits & 2; f.dqpsk = bits & 4; f.sync = bits & 8; f.frame_stride = bits & 16;
                            f.total_phase = bits & 32; f.fine_freq = bits & 64; f.classed = bits & 128; f.generic_mode1 = bits & 256;
                            f.symbols_per_block = spb; f.n_frames = 3;
                            f.soft_policy = policy; f.soft_level = level;
                            check_one(mode, f, n);
                        }
    print_counters(n);
    return failed ? 1 : 0;
}

static uint64_t rng_state;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 32); }

static int run_fuzz(long count, uint64_t seed) {
    rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
    counters n = {};
    for (long i = 0; i < count; i++) {
        dabgpu_demod_facts f;
        const uint32_t r = rnd();
        const int mode = (r & 7) == 7 ? (int)rnd() : (int)(r & 7) % 6;
        f.src = (rnd() & 15) == 0 ? (int)rnd() : (int)(rnd() % 6) - 1;
        const uint32_t bits = rnd();
        f.desc = bits & 1; f.fft = bits & 2; f.dqpsk = bits & 4; f.sync = bits & 8; f.frame_stride = bits & 16;
        f.total_phase = bits & 32; f.fine_freq = bits & 64; f.classed = bits & 128; f.generic_mode1 = bits & 256;
        f.switch_generic = bits & 512; f.switch_mode3_single = bits & 1024;
        f.symbols_per_block = (int)(rnd() % 200) - 20;
        f.n_frames = (int)(rnd() >> (rnd() % 32));
        f.soft_policy = (rnd() & 7) == 0 ? (int)rnd() : (int)(rnd() % 3);
        const uint32_t lb = rnd();
        if (rnd() & 1) memcpy(&f.soft_level, &lb, 4);                       // any bit pattern: NaNs, infinities, denormals
        else f.soft_level = (float)(lb % 1400) * 0.1f - 6.0f;
        check_one(mode, f, n);
        // the entry points' own check of a configuration
        dabgpu_soft_cfg cfg = {f.soft_policy, f.soft_level};
        const bool ok = (cfg.policy == DABGPU_SOFT_NORMALISED || cfg.policy == DABGPU_SOFT_CSI) && cfg.level >= 1.0f && cfg.level <= 127.0f;
        CHECK((dabgpu_host_check_soft_cfg("fuzz", &cfg) == DABGPU_OK) == ok);
    }
    print_counters(n);
    return failed ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "all")) return run_all();
    if (argc == 4 && !strcmp(argv[1], "fuzz")) return run_fuzz(atol(argv[2]), (uint64_t)atoll(argv[3]));
    if (argc == 4 && !strcmp(argv[1], "cfg")) {
        dabgpu_soft_cfg cfg = {atoi(argv[2]), (float)atof(argv[3])};
        const int null_st = dabgpu_host_check_soft_cfg("driver", nullptr);
        const int st = dabgpu_host_check_soft_cfg("driver", &cfg);
        printf("{\"status\": %d, \"error\": \"%s\", \"null\": %d}\n", st, st ? dabgpu_last_error() : "", null_st);
        return 0;
    }
    if (argc == 14 && !strcmp(argv[1], "plan")) {
        dabgpu_demod_facts f;
        const int mode = atoi(argv[2]);
        f.src = atoi(argv[3]); f.desc = atoi(argv[4]); f.fft = atoi(argv[5]); f.dqpsk = atoi(argv[6]); f.sync = atoi(argv[7]); f.classed = atoi(argv[8]);
        f.symbols_per_block = atoi(argv[9]); f.n_frames = atoi(argv[10]); f.generic_mode1 = atoi(argv[11]);
        f.soft_policy = atoi(argv[12]); f.soft_level = (float)atof(argv[13]);
        const dabgpu_demod_plan p = dabgpu_host_plan_demod(mode, f);
        if (p.status) { printf("{\"status\": %d, \"error\": \"%s\"}\n", p.status, dabgpu_last_error()); return 0; }
        printf("{\"status\": 0, \"family\": %d, \"variant\": %d, \"symbols_per_block\": %d, \"chunks\": %d, \"grid\": %u, \"tail\": %d}\n", (int)p.family, p.variant,
               p.symbols_per_block, p.chunks, p.grid, (int)p.tail);
        return 0;
    }
    fprintf(stderr, "usage: softbit_plan_driver all | fuzz N SEED | cfg POLICY LEVEL | plan <12 values>\n");
    return 2;
}
