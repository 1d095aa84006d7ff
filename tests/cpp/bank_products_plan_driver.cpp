// Driver of the demodulation planner's bank_products fact (dabgpu_host_plan_demod, dab-radio_amd/csrc/dabgpu_host_logic.cpp): the stream bank's
// statement that its weighted round also stores every frame's DQPSK products by bits slot (dabgpu_stream_bank_set_products).  Built plain and
// with ASan + UBSan by tests/test_bank_products_plan.py.
//   bank_products_plan_driver all            every combination of the facts below.  Without bank_products the plan -- status, every field, and the
//                                            text of every refusal -- is the one the planner gave before the fact existed, restated here in full
//                                            (before_plan, bank_soft included); with it, the rules of the fact restated from their description.
//                                            One JSON line of counters
//   bank_products_plan_driver fuzz N SEED    N random calls (any integer as mode, loader, policy, run length, batch; any bit pattern as level)
//   bank_products_plan_driver plan MODE SRC DESC FFT DQPSK SYNC STRIDE CLASSED SPB N_FRAMES GENERIC_MODE1 POLICY LEVEL BANK_SOFT BANK_PRODUCTS
//                                            one plan as a JSON line
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "dabgpu_host_logic.h"

static long failed = 0;
#define CHECK(c) do { if (!(c)) { if (failed++ < 20) { fprintf(stderr, "check failed line %d: %s  ", __LINE__, #c); describe(mode, f); } } } while (0)

static void describe(int mode, const dabgpu_demod_facts& f) {
    fprintf(stderr, "[mode %d src %d desc %d fft %d dqpsk %d sync %d stride %d phase %d fine %d classed %d spb %d n %d generic_mode1 %d switches %d %d policy %d "
            "level %g bank_soft %d bank_products %d] %s\n", mode, f.src, f.desc, f.fft, f.dqpsk, f.sync, f.frame_stride, f.total_phase, f.fine_freq, f.classed,
            f.symbols_per_block, f.n_frames, f.generic_mode1, f.switch_generic, f.switch_mode3_single, f.soft_policy, (double)f.soft_level, f.bank_soft,
            f.bank_products, dabgpu_last_error());
}

// the modes' geometry, restated: symbols per frame (the null symbol apart), symbol period, FFT size
static const int N_SYM[5] = {0, 76, 76, 153, 76}, PERIOD[5] = {0, 2552, 638, 319, 1276}, N_FFT[5] = {0, 2048, 512, 256, 1024};

struct expected { dabgpu_demod_plan p; std::string error; };

static bool level_ok(float level) { return level >= 1.0f && level <= 127.0f; }

// the planner before bank_products existed: what it answered for these facts (bank_products is not looked at)
static expected before_plan(int mode, const dabgpu_demod_facts& f) {
    expected e;
    e.p = dabgpu_demod_plan{};
    e.p.status = DABGPU_ERR_INVALID_ARG;
    char msg[256];
    if (mode < 1 || mode > 4) { snprintf(msg, sizeof msg, "ofdm_demod: invalid transmission mode %d", mode); e.error = msg; return e; }
    const bool mode1 = mode == 1 && !f.generic_mode1;
    const bool views = f.fft || f.dqpsk;
    const int layout = f.classed ? 2 : views ? 1 : 0;
    if (mode1) {
        if (f.src < 0 || f.src > 3) { snprintf(msg, sizeof msg, "ofdm_demod: no loader %d", f.src); e.error = msg; return e; }
        if (f.classed && views) { e.error = "ofdm_demod: soft bits in class order come without the display views"; return e; }
        if (f.desc && (f.sync || f.frame_stride)) { e.error = "ofdm_demod: a bank round takes neither sync records nor a frame stride"; return e; }
        e.p.family = DABGPU_DEMOD_MODE1;
        e.p.variant = (f.src * 2 + (f.desc ? 1 : 0)) * 3 + layout;
    }
    if (f.bank_soft && !f.desc) { e.error = "ofdm_demod: bank_soft is a bank round's fact: it needs frame descriptors"; return e; }
    if (f.bank_soft && f.soft_policy == DABGPU_SOFT_NORMALISED) { e.error = "ofdm_demod: bank_soft asks for DABGPU_SOFT_CSI, the policy is the normalised one"; return e; }
    if (f.soft_policy != DABGPU_SOFT_NORMALISED) {
        if (f.soft_policy != DABGPU_SOFT_CSI) { snprintf(msg, sizeof msg, "ofdm_demod: no soft-decision policy %d", f.soft_policy); e.error = msg; return e; }
        if (!mode1) {
            snprintf(msg, sizeof msg, "ofdm_demod: the weighted soft bits exist for the transmission mode I kernel only (mode %d)", mode); e.error = msg; return e;
        }
        if (f.desc && !f.bank_soft) { e.error = "ofdm_demod: the weighted soft bits have no stream-bank loader (frame descriptors)"; return e; }
        if (f.bank_soft && views) { e.error = "ofdm_demod: a bank round has no display views under the weighted policy"; return e; }
        if (!level_ok(f.soft_level)) { snprintf(msg, sizeof msg, "ofdm_demod: soft level %g outside [1, 127]", (double)f.soft_level); e.error = msg; return e; }
        e.p.variant = f.bank_soft ? 36 + f.src * 2 + (f.classed ? 1 : 0) : 24 + f.src * 3 + layout;
    }
    if (!mode1) {
        e.p.family = (mode == 1 || f.fft || f.switch_generic) ? DABGPU_DEMOD_GENERIC : (mode == 3 && !f.switch_mode3_single) ? DABGPU_DEMOD_WAVE3 : DABGPU_DEMOD_WAVE;
        e.p.variant = !f.desc ? 0 : f.src == 0 ? 1 : f.src == 1 ? 2 : f.src == 2 ? 3 : 4;
    }
    const int n_out = N_SYM[mode] - 1;
    e.p.symbols_per_block = (f.symbols_per_block <= 0 || f.symbols_per_block > n_out) ? (mode1 ? 25 : 19) : f.symbols_per_block;
    e.p.chunks = (n_out + e.p.symbols_per_block - 1) / e.p.symbols_per_block;
    const uint64_t units = (uint64_t)(f.n_frames > 0 ? f.n_frames : 0) * (uint64_t)e.p.chunks;
    const bool wave = e.p.family == DABGPU_DEMOD_WAVE || e.p.family == DABGPU_DEMOD_WAVE3;
    e.p.grid = (uint32_t)(wave ? (units + 3) / 4 : units);
    e.p.threads = (e.p.family == DABGPU_DEMOD_GENERIC && (mode == 2 || mode == 3)) ? 128 : 256;
    e.p.lds_bytes = e.p.family == DABGPU_DEMOD_GENERIC ? (uint32_t)((PERIOD[mode] + 3 * N_FFT[mode]) * 8 + 2048) : 0;
    e.p.raise_lds_limit = e.p.lds_bytes > 48u * 1024u;
    e.p.fine_stride = f.sync ? (int)(sizeof(dabgpu_sync_state) / sizeof(float)) : 1;
    const bool want_tail = mode1 && !f.desc && (f.total_phase || f.fine_freq || f.sync);
    e.p.tail = !want_tail ? DABGPU_DEMOD_TAIL_NONE : (e.p.chunks == 1 && !views) ? DABGPU_DEMOD_TAIL_FUSED : DABGPU_DEMOD_TAIL_LAUNCH;
    e.p.status = DABGPU_OK;
    return e;
}

static bool same_launch(const dabgpu_demod_plan& a, const dabgpu_demod_plan& b) {        // everything but status and variant
    return a.family == b.family && a.symbols_per_block == b.symbols_per_block && a.chunks == b.chunks && a.grid == b.grid && a.threads == b.threads &&
           a.lds_bytes == b.lds_bytes && a.raise_lds_limit == b.raise_lds_limit && a.tail == b.tail && a.fine_stride == b.fine_stride;
}

struct counters {
    long checked, as_before, as_before_refused, as_before_views, as_before_weighted_bank, no_bank_soft, classed, fft, dqpsk, bad_policy, not_mode1, bad_level,
         products;
    long variant[4];
};

static void check_one(int mode, const dabgpu_demod_facts& f, counters& n) {
    const dabgpu_demod_plan p = dabgpu_host_plan_demod(mode, f);
    const std::string err = p.status ? dabgpu_last_error() : "";
    n.checked++;
    const expected b = before_plan(mode, f);
    const bool valid_mode = mode >= 1 && mode <= 4;
    const bool mode1 = mode == 1 && !f.generic_mode1;
    const bool views = f.fft || f.dqpsk;
    // refusals that come first whatever the new fact says: the mode, the mode I kernel's own, bank_soft's two
    const bool earlier = !valid_mode || (mode1 && (f.src < 0 || f.src > 3 || (f.classed && views) || (f.desc && (f.sync || f.frame_stride)))) ||
                         (f.bank_soft && (!f.desc || f.soft_policy == DABGPU_SOFT_NORMALISED));
    if (!f.bank_products || earlier) {
        // byte for byte the planner's earlier answer: the status, every field of an accepted plan, the text of a refusal
        CHECK(p.status == b.p.status);
        if (p.status) CHECK(err == b.error);
        else CHECK(p.variant == b.p.variant && same_launch(p, b.p) && p.variant < 44);
        n.as_before++; n.as_before_refused += p.status != 0;
        n.as_before_views += p.status != 0 && err == "ofdm_demod: a bank round has no display views under the weighted policy";
        n.as_before_weighted_bank += p.status == 0 && p.family == DABGPU_DEMOD_MODE1 && p.variant >= 36;
        return;
    }
    // bank_products: it needs bank_soft; no class order, no FFT view, no product view by frame (each refusal names the field); then the
    // weighted policy's own order -- it exists, the mode I kernel, a level in [1, 127]
    const bool no_bank_soft = !f.bank_soft;
    const bool classed = !no_bank_soft && f.classed;
    const bool fft = !no_bank_soft && !classed && f.fft;
    const bool dqpsk = !no_bank_soft && !classed && !fft && f.dqpsk;
    const bool ahead = no_bank_soft || classed || fft || dqpsk;
    const bool bad_policy = !ahead && f.soft_policy != DABGPU_SOFT_CSI;
    const bool not_mode1 = !ahead && !bad_policy && !mode1;
    const bool bad_level = !ahead && !bad_policy && !not_mode1 && !level_ok(f.soft_level);
    const bool refused = ahead || bad_policy || not_mode1 || bad_level;
    CHECK((p.status == DABGPU_ERR_INVALID_ARG) == refused && (p.status == DABGPU_OK) == !refused);
    if (refused) {
        const char* text = no_bank_soft ? "bank_soft" : classed ? "classed" : fft ? "fft" : dqpsk ? "dqpsk" : bad_policy ? "policy" : not_mode1 ? "mode I" : "level";
        CHECK(strstr(err.c_str(), text) != nullptr);
        if (ahead) CHECK(strstr(err.c_str(), "bank_products") != nullptr);
        n.no_bank_soft += no_bank_soft; n.classed += classed; n.fft += fft; n.dqpsk += dqpsk; n.bad_policy += bad_policy; n.not_mode1 += not_mode1;
        n.bad_level += bad_level;
        return;
    }
    CHECK(p.family == DABGPU_DEMOD_MODE1);
    CHECK(p.variant == 44 + f.src);
    CHECK(DABGPU_DEMOD_MODE1_BANK_PRODUCTS_FIRST == 44 && DABGPU_DEMOD_MODE1_KERNELS == 48 && DABGPU_DEMOD_MODE1_VARIANTS == 44 && DABGPU_DEMOD_MODE1_BANK_SOFT_FIRST == 36 &&
          DABGPU_DEMOD_MODE1_NORMALISED_VARIANTS == 24);
    if (p.variant >= 44 && p.variant < 48) n.variant[p.variant - 44]++;
    n.products++;
    // run length, chunks, grid, threads and tail: the weighted bank round's with the same facts, itself the normalised bank round's
    dabgpu_demod_facts g = f;
    g.bank_products = false;
    const dabgpu_demod_plan q = dabgpu_host_plan_demod(mode, g);
    CHECK(q.status == DABGPU_OK && same_launch(p, q) && q.variant == 36 + f.src * 2 && p.tail == DABGPU_DEMOD_TAIL_NONE);
}

static void print_counters(const counters& n) {
    printf("{\"checked\": %ld, \"failed_checks\": %ld, \"as_before\": %ld, \"as_before_refused\": %ld, \"as_before_views\": %ld, \"as_before_weighted_bank\": %ld, "
           "\"no_bank_soft\": %ld, \"classed\": %ld, \"fft\": %ld, \"dqpsk\": %ld, \"bad_policy\": %ld, \"not_mode1\": %ld, \"bad_level\": %ld, \"products\": %ld, "
           "\"variants\": [%ld, %ld, %ld, %ld]}\n", n.checked, failed, n.as_before, n.as_before_refused, n.as_before_views, n.as_before_weighted_bank,
           n.no_bank_soft, n.classed, n.fft, n.dqpsk, n.bad_policy, n.not_mode1, n.bad_level, n.products, n.variant[0], n.variant[1], n.variant[2], n.variant[3]);
}

static void set_bits(dabgpu_demod_facts& f, uint32_t bits) {
    f.desc = bits & 1; f.fft = bits & 2; f.dqpsk = bits & 4; f.sync = bits & 8; f.frame_stride = bits & 16; f.total_phase = bits & 32; f.fine_freq = bits & 64;
    f.classed = bits & 128; f.generic_mode1 = bits & 256; f.switch_generic = bits & 512; f.switch_mode3_single = bits & 1024; f.bank_soft = bits & 2048;
    f.bank_products = bits & 4096;
}

static int run_all() {
    static const int POLICY[] = {0, 1, 2, -1};
    static const float LEVEL[] = {64.0f, 1.0f, 127.5f, NAN};
    static const int SPB[] = {0, 19};
    static const int FRAMES[] = {1, 1024};
    counters n = {};
    for (int mode = 0; mode <= 5; mode++)
        for (int src = -1; src <= 4; src++)
            for (uint32_t bits = 0; bits < (1u << 13); bits++)
                for (int policy : POLICY)
                    for (float level : LEVEL)
                        for (int spb : SPB)
                            for (int frames : FRAMES) {
                                dabgpu_demod_facts f;
                                f.src = src;
                                set_bits(f, bits);
                                f.symbols_per_block = spb; f.n_frames = frames; f.soft_policy = policy; f.soft_level = level;
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
        const int mode = (r & 15) == 15 ? (int)rnd() : (r & 1) ? 1 : (int)((r >> 1) & 7) % 6;
        f.src = (rnd() & 15) == 0 ? (int)rnd() : (int)(rnd() % 6) - 1;
        uint32_t bits = rnd();
        if (rnd() & 1) bits = (bits & ~(8u | 16u | 256u)) | 1u | 2048u;          // half of the calls: a bank round that states bank_soft
        set_bits(f, bits);
        f.symbols_per_block = (int)(rnd() % 200) - 20;
        f.n_frames = (int)(rnd() >> (rnd() % 32));
        f.soft_policy = (rnd() & 7) == 0 ? (int)rnd() : (int)(rnd() % 3);
        const uint32_t lb = rnd();
        if (rnd() & 1) memcpy(&f.soft_level, &lb, 4);                            // any bit pattern: NaNs, infinities, denormals
        else f.soft_level = (float)(lb % 1400) * 0.1f - 6.0f;
        check_one(mode, f, n);
    }
    print_counters(n);
    return failed ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "all")) return run_all();
    if (argc == 4 && !strcmp(argv[1], "fuzz")) return run_fuzz(atol(argv[2]), (uint64_t)atoll(argv[3]));
    if (argc == 17 && !strcmp(argv[1], "plan")) {
        dabgpu_demod_facts f;
        const int mode = atoi(argv[2]);
        f.src = atoi(argv[3]); f.desc = atoi(argv[4]); f.fft = atoi(argv[5]); f.dqpsk = atoi(argv[6]); f.sync = atoi(argv[7]); f.frame_stride = atoi(argv[8]);
        f.classed = atoi(argv[9]); f.symbols_per_block = atoi(argv[10]); f.n_frames = atoi(argv[11]); f.generic_mode1 = atoi(argv[12]);
        f.soft_policy = atoi(argv[13]); f.soft_level = (float)atof(argv[14]); f.bank_soft = atoi(argv[15]); f.bank_products = atoi(argv[16]);
        const dabgpu_demod_plan p = dabgpu_host_plan_demod(mode, f);
        if (p.status) { printf("{\"status\": %d, \"error\": \"%s\"}\n", p.status, dabgpu_last_error()); return 0; }
        printf("{\"status\": 0, \"family\": %d, \"variant\": %d, \"symbols_per_block\": %d, \"chunks\": %d, \"grid\": %u, \"threads\": %u, \"tail\": %d, "
               "\"fine_stride\": %d}\n", (int)p.family, p.variant, p.symbols_per_block, p.chunks, p.grid, p.threads, (int)p.tail, p.fine_stride);
        return 0;
    }
    fprintf(stderr, "usage: bank_products_plan_driver all | fuzz N SEED | plan <15 values>\n");
    return 2;
}
