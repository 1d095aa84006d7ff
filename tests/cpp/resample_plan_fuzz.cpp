// resample_plan_fuzz.cpp -- dabgpu_resample_plan, the step conversions and dabgpu_resample_input_needed (dab-radio_amd/csrc/
// dabgpu_host_logic.cpp) under ASan + UBSan (tests/test_resample_plan.py builds it): random parameter lists with at most one defect each,
// allocated exactly so that a read past the list is caught; an acceptance is checked against the geometry the header states, a refusal
// against the defect planted; the input span against the time of every output, taken with the compiler's 128-bit integers (host only).
//   resample_plan_fuzz <iterations> <seed>  -> one JSON line with how often each side of every decision was reached
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "dabgpu.h"
#include "dabgpu_host_logic.h"
#include "resample_core.h"

typedef __int128 i128;

static i128 time_of(const dabgpu_resample_stream& P, uint64_t m) {
    return (i128)P.offset_samples * ((i128)1 << 62) + (i128)P.offset_frac_q62 + (i128)m * (i128)P.step_q62;
}
static i128 floor62(i128 t) { return t >> 62; }                  // (arithmetic shift: floor)

int main(int argc, char** argv) {
    const long iters = argc > 1 ? std::atol(argv[1]) : 100000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
    enum { OK, N_STREAMS, STEP, ABOVE_DESIGN, GAIN, OFFSET, FRAC, NULL_PARAMS, NULL_DESIGN, N_KINDS };
    long failed = 0, reached[N_KINDS][2] = {}, narrow[2] = {}, fits[2] = {}, spans = 0, round_trips = 0, times = 0;
    const float bad_values[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
    const uint64_t ONE = (uint64_t)1 << 62;
    dabgpu_resample_filter* design = new dabgpu_resample_filter;             // (only max_step is read by the planner)
    std::memset(design, 0, sizeof(*design));
    for (long it = 0; it < iters; it++) {
        const int kind = (int)(rng() % N_KINDS), side = (int)(rng() & 1);
        const size_t n = 1 + rng() % 6;
        const bool near_one = rng() % 3 == 0;
        design->max_step = near_one ? 1.0 + (double)(1 + rng() % 300) * 1e-6 : 0.5 + (double)(rng() % 1501) / 1000.0;
        const uint64_t max_q = dabgpu_host_resample_max_step_q62(design->max_step);
        std::vector<dabgpu_resample_stream> v(n);
        uint64_t top = 0;
        uint32_t rows = 0;
        for (auto& P : v) {
            std::memset(&P, 0, sizeof(P));
            P.step_q62 = (ONE >> 1) + rng() % (max_q - (ONE >> 1) + 1);
            if (near_one) P.step_q62 = ONE - (ONE >> 12) + rng() % (max_q - ONE + (ONE >> 12) + 1);
            if (rng() % 9 == 0) P.step_q62 = (rng() & 1) ? max_q : (ONE >> 1);              // (the edges are accepted)
            if (rng() % 9 == 0 && max_q >= ONE) P.step_q62 = ONE;
            P.offset_samples = (int64_t)rng() >> 1;
            if (rng() % 7 == 0) P.offset_samples = (rng() & 1) ? DABGPU_CHANNEL_MAX_POSITION : -DABGPU_CHANNEL_MAX_POSITION;
            P.offset_frac_q62 = (rng() % 4 == 0) ? 0 : rng() & (ONE - 1);
            if (rng() % 11 == 0) P.offset_frac_q62 = ONE - 1;
            P.gain = (float)(rng() % 2000) / 100.0f - 10.0f;
            P.reserved = (int32_t)rng();
            top = std::max(top, P.step_q62);
            if (!dabgpu::rs_identity(P)) rows = std::max(rows, dabgpu::rs_rows_needed(P));
        }
        dabgpu_resample_stream& B = v[rng() % n];
        size_t n_arg = n;
        const dabgpu_resample_stream* list = v.data();
        const dabgpu_resample_filter* d_arg = design;
        int k2 = kind;
        switch (kind) {
        case N_STREAMS: n_arg = side ? ((size_t)1 << 20) + 1 + rng() % 5 : 0; break;
        case STEP: B.step_q62 = side ? (ONE << 1) + 1 + rng() % 1000 : (ONE >> 1) - 1 - rng() % 1000; break;
        case ABOVE_DESIGN: if (max_q < (ONE << 1)) B.step_q62 = max_q + 1 + (side ? rng() % ((ONE << 1) - max_q) : 0); else k2 = OK; break;
        case GAIN: B.gain = bad_values[rng() % 3]; break;
        case OFFSET: B.offset_samples = side ? DABGPU_CHANNEL_MAX_POSITION + 1 + (int64_t)(rng() % 1000) : -DABGPU_CHANNEL_MAX_POSITION - 1 - (int64_t)(rng() % 1000); break;
        case FRAC: B.offset_frac_q62 = side ? ~(uint64_t)0 - rng() % 1000 : ONE + rng() % 1000; break;
        case NULL_PARAMS: list = nullptr; break;
        case NULL_DESIGN: d_arg = nullptr; break;
        default: break;
        }
        if (k2 == OK && kind == ABOVE_DESIGN) { top = std::max(top, B.step_q62); }
        dabgpu_resample_geometry g;
        std::memset(&g, 0x5A, sizeof(g));
        const bool want_g = rng() % 9 != 0;
        const int st = dabgpu_resample_plan(list, n_arg, d_arg, want_g ? &g : nullptr);
        bool ok = (k2 == OK) ? st == DABGPU_OK : st == DABGPU_ERR_INVALID_ARG;
        if (ok && k2 == OK && want_g) {
            const uint32_t window_exact = (uint32_t)((top >> 52) + ((top & (((uint64_t)1 << 52) - 1)) ? 1 : 0)) + DABGPU_RESAMPLE_TAPS + 2;   // ceil(1024 step) + taps + 2
            ok = g.block_samples == DABGPU_RESAMPLE_BLOCK && g.window_samples == window_exact && g.table_rows == rows && rows <= DABGPU_RESAMPLE_PHASES + 1 &&
                 g.lds_bytes == ((window_exact + 1) & ~1u) * 8 + rows * (DABGPU_RESAMPLE_TAPS + 1) * 4 && g.lds_bytes <= 160u * 1024u;
            if (ok) narrow[rows < DABGPU_RESAMPLE_PHASES + 1]++;
        }
        if (ok) reached[k2][side]++;
        else { failed++; if (failed < 5) std::fprintf(stderr, "case %ld: kind %d status %d (%s)\n", it, kind, st, dabgpu_last_error()); }
        // set_params against the geometry of a bank's creation
        {
            const dabgpu_resample_geometry created = {DABGPU_RESAMPLE_BLOCK, (uint32_t)(562 + rng() % 1537), (uint32_t)(rng() % 258), 0};
            const dabgpu_resample_geometry wanted = {DABGPU_RESAMPLE_BLOCK, (rng() % 3 == 0) ? created.window_samples : (uint32_t)(562 + rng() % 1537),
                                                     (rng() % 3 == 0) ? created.table_rows : (uint32_t)(rng() % 258), 0};
            const bool fit = wanted.window_samples <= created.window_samples && wanted.table_rows <= created.table_rows;
            if ((dabgpu_host_resample_fits(created, wanted) == DABGPU_OK) != fit) failed++; else fits[fit]++;
        }
        // the time of an output and the input span of a call, against 128-bit integers
        if (kind == OK || kind == GAIN) {
            const dabgpu_resample_stream& P = v[0];
            const uint64_t pos = (rng() % 5 == 0) ? (uint64_t)DABGPU_CHANNEL_MAX_POSITION - rng() % 5000 : rng() >> (2 + rng() % 60);
            const size_t n_out = (rng() % 6 == 0) ? 0 : 1 + rng() % 5000;
            for (int q = 0; q < 4; q++) {
                const uint64_t m = pos + (n_out ? rng() % n_out : 0);
                const i128 t = time_of(P, m);
                const dabgpu::RsTime got = dabgpu::rs_time(P, m);
                const i128 fl = floor62(t);
                if (got.n != (uint64_t)fl || got.neg != (fl < 0) || got.frac != (uint64_t)(t & (i128)(ONE - 1))) failed++; else times++;
                for (int64_t n_in : {(int64_t)1, (int64_t)37, (int64_t)1 << 40}) {
                    i128 r = fl % n_in; if (r < 0) r += n_in;
                    if (dabgpu::rs_mod(dabgpu::rs_index(got), n_in) != (int64_t)r) failed++;
                }
            }
            int64_t first = 7; uint64_t count = 7;
            dabgpu_resample_stream Q = P;
            if (kind == GAIN) Q.gain = 1.0f;
            const int st3 = dabgpu_resample_input_needed(&Q, pos, n_out, &first, &count);
            const bool ident = dabgpu::rs_identity(Q);
            const i128 a = floor62(time_of(Q, pos)) - (ident ? 0 : DABGPU_RESAMPLE_TAPS / 2 - 1);
            const i128 b = n_out ? floor62(time_of(Q, pos + n_out - 1)) + (ident ? 0 : DABGPU_RESAMPLE_TAPS / 2) : a - 1;
            if (n_out && b >= ((i128)1 << 63)) { if (st3 != DABGPU_ERR_INVALID_ARG) failed++; }
            else if (st3 != DABGPU_OK || (n_out ? ((i128)first != a || (i128)count != b - a + 1) : count != 0)) failed++;
            else spans++;
        }
        // step words: the inverse of the conversion is exact for every word whose low 11 bits are clear (a double's 53 bits)
        const uint64_t w = ((ONE >> 1) + rng() % (3 * (ONE >> 1))) & ~(uint64_t)0x7FF;
        const double stp = dabgpu_resample_step(w);
        if (!(stp >= 0.5 && stp <= 2.0) || dabgpu_resample_step_q62(stp, 1.0, 0.0) != w) failed++;
        else round_trips++;
    }
    if (dabgpu_resample_step_q62(std::nan(""), 1.0, 0.0) != 0 || dabgpu_resample_step_q62(1.0, 0.0, 0.0) != 0 || dabgpu_resample_step_q62(-1.0, 1.0, 0.0) != 0 ||
        dabgpu_resample_step_q62(4.0, 1.0, 0.0) != 0 || dabgpu_resample_step_q62(1.0, 1.0, std::numeric_limits<double>::infinity()) != 0) failed++;
    delete design;
    std::printf("{\"iterations\": %ld, \"failed_checks\": %ld, \"accepted\": %ld, \"whole_table\": %ld, \"narrow\": %ld, \"round_trips\": %ld, \"spans\": %ld, \"times\": %ld",
                iters, failed, reached[OK][0] + reached[OK][1], narrow[0], narrow[1], round_trips, spans, times);
    const char* names[N_KINDS] = {"", "n_streams", "step", "above_design", "gain", "offset", "frac", "null_params", "null_design"};
    for (int k = 1; k < N_KINDS; k++) std::printf(", \"%s_low\": %ld, \"%s_high\": %ld", names[k], reached[k][0], names[k], reached[k][1]);
    std::printf(", \"fits_no\": %ld, \"fits_yes\": %ld}\n", fits[0], fits[1]);
    return failed ? 1 : 0;
}
