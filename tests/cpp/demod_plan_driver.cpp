// Driver of the demodulation planner (dabgpu_host_plan_demod, dab-radio_amd/csrc/dabgpu_host_logic.cpp), built plain by tests/test_demod_plan.py
// and with ASan + UBSan by tests/test_host_sanitizers.py.
//   demod_plan_driver all    every combination of the facts of a call (modes 0..5, loaders -1..4, every boolean fact, both development
//                            switches, the run lengths and batch sizes below) against the launch rules restated here from their description,
//                            not from the planner; prints one JSON line of counters
//   demod_plan_driver plan MODE SRC DESC FFT DQPSK SYNC STRIDE TOTAL_PHASE FINE_FREQ CLASSED SPB N_FRAMES GENERIC_MODE1 SW_GENERIC SW_MODE3_SINGLE
//                            one plan as a JSON line (the hand-worked cases of the test)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dabgpu_host_logic.h"

static long failed = 0;
#define CHECK(c) do { if (!(c)) { if (failed++ < 20) { fprintf(stderr, "check failed line %d: %s  ", __LINE__, #c); describe(mode, f); } } } while (0)

static void describe(int mode, const dabgpu_demod_facts& f) {
    fprintf(stderr, "[mode %d src %d desc %d fft %d dqpsk %d sync %d stride %d phase %d fine %d classed %d spb %d n %d generic_mode1 %d switches %d %d]\n", mode, f.src,
            f.desc, f.fft, f.dqpsk, f.sync, f.frame_stride, f.total_phase, f.fine_freq, f.classed, f.symbols_per_block, f.n_frames, f.generic_mode1,
            f.switch_generic, f.switch_mode3_single);
}

// the modes' geometry, restated: symbols per frame (the null symbol apart), symbol period, FFT size
static const int N_SYM[5] = {0, 76, 76, 153, 76}, PERIOD[5] = {0, 2552, 638, 319, 1276}, N_FFT[5] = {0, 2048, 512, 256, 1024};

struct counters { long checked, refused, bad_mode, bad_loader, classed_views, bank_sync_stride, family[4], tail[3], raise_lds; };

static void check_one(int mode, const dabgpu_demod_facts& f, counters& n) {
    const dabgpu_demod_plan p = dabgpu_host_plan_demod(mode, f);
    n.checked++;
    const bool valid_mode = mode >= 1 && mode <= 4;
    const bool mode1 = mode == 1 && !f.generic_mode1;           // the mode I kernel; generic_mode1: mode I on the size-generic kernel
    const bool views = f.fft || f.dqpsk;
    // refused: no such mode; and, of the mode I kernel, no such loader, soft bits in class order with views, bank descriptors with sync
    // records or a frame stride
    const bool bad_loader = valid_mode && mode1 && (f.src < 0 || f.src > 3);
    const bool classed_views = valid_mode && mode1 && f.classed && views;
    const bool bank_sync_stride = valid_mode && mode1 && f.desc && (f.sync || f.frame_stride);
    const bool refused = !valid_mode || bad_loader || classed_views || bank_sync_stride;
    CHECK((p.status == DABGPU_ERR_INVALID_ARG) == refused && (p.status == DABGPU_OK) == !refused);
    if (refused) {
        CHECK(dabgpu_last_error()[0] != 0);
        n.refused++; n.bad_mode += !valid_mode; n.bad_loader += bad_loader; n.classed_views += classed_views; n.bank_sync_stride += bank_sync_stride;
        return;
    }
    // family
    dabgpu_demod_family family;
    if (mode1) family = DABGPU_DEMOD_MODE1;
    else if (mode == 1 || f.fft || f.switch_generic) family = DABGPU_DEMOD_GENERIC;
    else if (mode == 3 && !f.switch_mode3_single) family = DABGPU_DEMOD_WAVE3;
    else family = DABGPU_DEMOD_WAVE;
    CHECK(p.family == family);
    n.family[family]++;
    // variant
    if (mode1) {
        const int layout = f.classed ? 2 : views ? 1 : 0;       // (classed implies no views)
        CHECK(p.variant == (f.src * 2 + (f.desc ? 1 : 0)) * 3 + layout);
        CHECK(p.variant >= 0 && p.variant < DABGPU_DEMOD_MODE1_VARIANTS);
    } else {
        // without descriptors only loader 0 exists; with them loaders 0, 1, 2 and whatever else is given as 3 (the ladders' last else)
        CHECK(p.variant == (!f.desc ? 0 : f.src == 0 ? 1 : f.src == 1 ? 2 : f.src == 2 ? 3 : 4));
        CHECK(p.variant >= 0 && p.variant < DABGPU_DEMOD_LOADER_VARIANTS);
    }
    // run length, runs per frame
    const int n_out = N_SYM[mode] - 1;
    const int spb = (f.symbols_per_block <= 0 || f.symbols_per_block > n_out) ? (mode1 ? 25 : 19) : f.symbols_per_block;
    const int chunks = (n_out + spb - 1) / spb;
    CHECK(p.symbols_per_block == spb && p.chunks == chunks);
    CHECK((long)p.chunks * p.symbols_per_block >= n_out && (long)(p.chunks - 1) * p.symbols_per_block < n_out);
    // grid, in 64 bits: nothing wraps
    const uint64_t units = (uint64_t)f.n_frames * (uint64_t)chunks;
    const bool wave = family == DABGPU_DEMOD_WAVE || family == DABGPU_DEMOD_WAVE3;
    CHECK((uint64_t)p.grid == (wave ? (units + 3) / 4 : units));
    if (wave) CHECK((uint64_t)p.grid * 4 >= units && (uint64_t)p.grid * 4 < units + 4);
    CHECK(p.threads == ((family == DABGPU_DEMOD_GENERIC && (mode == 2 || mode == 3)) ? 128u : 256u));
    // dynamic LDS and the 48 KB attribute
    const uint64_t lds = family == DABGPU_DEMOD_GENERIC ? ((uint64_t)PERIOD[mode] + 3 * (uint64_t)N_FFT[mode]) * 8 + 2048 : 0;
    CHECK((uint64_t)p.lds_bytes == lds && p.raise_lds_limit == (lds > 48 * 1024));
    CHECK(p.raise_lds_limit == (family == DABGPU_DEMOD_GENERIC && mode == 1));
    n.raise_lds += p.raise_lds_limit;
    // phase tail (the mode I kernel's): with sync records the fine-frequency word is the record's, so they ask for the tail too
    const bool want = mode1 && (f.total_phase || f.fine_freq || f.sync);
    const bool fused = want && chunks == 1 && !f.desc && !views;
    const bool launch = want && !fused && !f.desc;
    CHECK(p.tail == (fused ? DABGPU_DEMOD_TAIL_FUSED : launch ? DABGPU_DEMOD_TAIL_LAUNCH : DABGPU_DEMOD_TAIL_NONE));
    n.tail[p.tail]++;
    if (mode1) CHECK(p.fine_stride == (f.sync ? (int)(sizeof(dabgpu_sync_state) / 4) : 1));
}

static int run_all() {
    static const int SPB[] = {-1, 0, 1, 19, 25, 38, 74, 75, 76, 152, 153};
    static const int FRAMES[] = {1, 3, 1024, 1 << 24};
    counters n = {};
    for (int mode = 0; mode <= 5; mode++)
        for (int src = -1; src <= 4; src++)
            for (int bits = 0; bits < (1 << 11); bits++)
                for (int spb : SPB)
                    for (int frames : FRAMES) {
                        dabgpu_demod_facts f;
                        f.src = src;
                        f.desc = bits & 1; f.fft = bits & 2; f.dqpsk = bits & 4; f.sync = bits & 8; f.frame_stride = bits & 16;
                        f.total_phase = bits & 32; f.fine_freq = bits & 64; f.classed = bits & 128;
                        f.switch_generic = bits & 256; f.switch_mode3_single = bits & 512; f.generic_mode1 = bits & 1024;
                        f.symbols_per_block = spb; f.n_frames = frames;
                        check_one(mode, f, n);
                    }
    printf("{\"checked\": %ld, \"failed_checks\": %ld, \"refused\": %ld, \"bad_mode\": %ld, \"bad_loader\": %ld, \"classed_views\": %ld, \"bank_sync_stride\": %ld, "
           "\"mode1\": %ld, \"generic\": %ld, \"wave\": %ld, \"wave3\": %ld, \"tail_none\": %ld, \"tail_fused\": %ld, \"tail_launch\": %ld, \"raise_lds\": %ld}\n",
           n.checked, failed, n.refused, n.bad_mode, n.bad_loader, n.classed_views, n.bank_sync_stride, n.family[0], n.family[1], n.family[2], n.family[3],
           n.tail[0], n.tail[1], n.tail[2], n.raise_lds);
    return failed ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "all")) return run_all();
    if (argc == 17 && !strcmp(argv[1], "plan")) {
        int v[15];
        for (int k = 0; k < 15; k++) v[k] = atoi(argv[2 + k]);
        dabgpu_demod_facts f;
        f.src = v[1]; f.desc = v[2]; f.fft = v[3]; f.dqpsk = v[4]; f.sync = v[5]; f.frame_stride = v[6]; f.total_phase = v[7]; f.fine_freq = v[8];
        f.classed = v[9]; f.symbols_per_block = v[10]; f.n_frames = v[11]; f.generic_mode1 = v[12]; f.switch_generic = v[13]; f.switch_mode3_single = v[14];
        const dabgpu_demod_plan p = dabgpu_host_plan_demod(v[0], f);
        if (p.status) { printf("{\"status\": %d, \"error\": \"%s\"}\n", p.status, dabgpu_last_error()); return 0; }
        printf("{\"status\": 0, \"family\": %d, \"variant\": %d, \"symbols_per_block\": %d, \"chunks\": %d, \"grid\": %u, \"threads\": %u, \"lds_bytes\": %u, "
               "\"raise_lds_limit\": %d, \"tail\": %d, \"fine_stride\": %d}\n", (int)p.family, p.variant, p.symbols_per_block, p.chunks, p.grid, p.threads,
               p.lds_bytes, (int)p.raise_lds_limit, (int)p.tail, p.fine_stride);
        return 0;
    }
    fprintf(stderr, "usage: demod_plan_driver all | plan <15 integers>\n");
    return 2;
}
