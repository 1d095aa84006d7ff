// interferer_plan_fuzz.cpp -- dabgpu_interferer_plan, dabgpu_interferer_design and the argument rules of an apply call
// (dab-radio_amd/csrc/dabgpu_host_logic.cpp), run plain and under ASan + UBSan (tests/test_interferer_plan.py builds it): random parameter
// lists with at most one defect each, allocated exactly so that a read past a list is caught; an acceptance is checked against the
// geometry the header states, a refusal against the defect planted.
//   interferer_plan_fuzz <iterations> <seed>  -> one JSON line with how often each side of every decision was reached
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

int main(int argc, char** argv) {
    const long iters = argc > 1 ? std::atol(argv[1]) : 100000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
    enum { OK, N_STREAMS, N_SHAPES, NULL_LISTS, INTERP, TAP_VALUE, N_SOURCES, KIND, AMP_NOT_FINITE, AMP_NEGATIVE, GATE_ON, GATE_OFFSET, SHAPE_INDEX, N_KINDS };
    enum { A_OK, A_FORMAT, A_N_OUT, A_NULL_OUT, A_IN_STRIDE, A_OUT_STRIDE, A_ALIGN, A_IN_PLACE, A_SCALE, A_GRID, A_KINDS };
    long failed = 0, reached[N_KINDS][2] = {}, apply_reached[A_KINDS][2] = {}, banded[2] = {}, fits[2] = {}, designs[2] = {}, no_input = 0, in_place_ok = 0;
    const float bad_values[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
    // four real shapes, L = 1, 2, 16, 64
    std::vector<dabgpu_interferer_shape> real(4);
    const double widths[4] = {0.6, 0.3, 0.046875, 0.0078125};
    for (int i = 0; i < 4; i++) if (dabgpu_interferer_design(widths[i], &real[i]) != DABGPU_OK) failed++;
    if (real[0].interp != 1 || real[1].interp != 2 || real[2].interp != 16 || real[3].interp != 64) failed++;
    for (long it = 0; it < iters; it++) {
        const int kind = (int)(rng() % N_KINDS), side = (int)(rng() & 1);
        const size_t n = 1 + rng() % 5;
        const int n_shapes = (int)(rng() % 5);
        std::vector<dabgpu_interferer_shape> shapes(real.begin(), real.begin() + n_shapes);
        std::vector<dabgpu_interferer_stream> v(n);
        uint32_t slots = 0, slot_bytes = 0;
        for (int i = 0; i < n_shapes; i++) {
            const uint32_t L = (uint32_t)shapes[i].interp;
            slot_bytes = std::max(slot_bytes, 64u * L + 8u * (1024u / L + 18u));
        }
        for (auto& P : v) {
            std::memset(&P, 0, sizeof(P));
            P.seed = rng(); P.n_sources = (int)(rng() % 5);
            uint32_t shaped = 0;
            for (int k = 0; k < 4; k++) {
                dabgpu_interferer_source& S = P.source[k];
                if (k >= P.n_sources) { std::memset(&S, 0xFF, sizeof(S)); continue; }       // (entries past n_sources may hold anything)
                S.kind = (int)(rng() % 3);
                S.shape = (S.kind == DABGPU_INTERFERER_BAND) ? (int)(rng() % (unsigned)(n_shapes + 1)) - 1 : (int)rng();
                S.amp = (rng() % 4 == 0) ? 0.0f : (float)(rng() % 1000) / 100.0f;
                S.freq_q64 = rng(); S.phase0_q64 = rng();
                S.gate_period = (rng() % 3 == 0) ? 0 : (rng() % 3 == 0 ? rng() : 1 + rng() % 5000);
                S.gate_on = S.gate_period ? ((rng() % 5 == 0) ? S.gate_period : rng() % (S.gate_period + 1)) : 0;      // (the edge is accepted)
                S.gate_offset = (int64_t)rng() >> 2;                                        // |offset| < 2^61
                if (rng() % 7 == 0) S.gate_offset = (rng() & 1) ? DABGPU_INTERFERER_MAX_POSITION - 1 : -DABGPU_INTERFERER_MAX_POSITION + 1;
                if (S.kind == DABGPU_INTERFERER_OFF) { S.amp = bad_values[rng() % 3]; S.gate_on = 1; S.gate_period = 0; }  // (an OFF source is not read)
                if (S.kind == DABGPU_INTERFERER_BAND && S.shape >= 0 && S.amp != 0.0f) shaped++;
            }
            slots = std::max(slots, shaped);
        }
        // the defect goes to a source that is read
        dabgpu_interferer_stream& B = v[rng() % n];
        size_t n_arg = n;
        int n_shapes_arg = n_shapes;
        const dabgpu_interferer_stream* list = v.data();
        const dabgpu_interferer_shape* shape_list = n_shapes ? shapes.data() : nullptr;
        bool planted = true;
        auto live_source = [&]() -> dabgpu_interferer_source* {
            if (B.n_sources == 0) { B.n_sources = 1; std::memset(&B.source[0], 0, sizeof(B.source[0])); }
            dabgpu_interferer_source& S = B.source[rng() % (unsigned)B.n_sources];
            if (S.kind == DABGPU_INTERFERER_OFF) { S.kind = DABGPU_INTERFERER_TONE; S.amp = 1.0f; S.gate_period = 0; S.gate_on = 0; S.gate_offset = 0; }
            return &S;
        };
        switch (kind) {
        case N_STREAMS: n_arg = side ? ((size_t)1 << 20) + 1 + rng() % 5 : 0; break;
        case N_SHAPES: n_shapes_arg = side ? 5 + (int)(rng() % 100) : -1 - (int)(rng() % 100); break;
        case NULL_LISTS: if (side && n_shapes > 0) shape_list = nullptr; else list = nullptr; break;
        case INTERP: if (n_shapes == 0) { planted = false; break; } shapes[rng() % n_shapes].interp = side ? 65 + (int)(rng() % 100) : (rng() & 1 ? 0 : 3 + 2 * (int)(rng() % 20)); break;
        case TAP_VALUE: if (n_shapes == 0) { planted = false; break; } { auto& H = shapes[rng() % n_shapes]; H.taps[rng() % (16u * (unsigned)H.interp)] = bad_values[rng() % 3]; } break;
        case N_SOURCES: B.n_sources = side ? 5 + (int)(rng() % 100) : -1 - (int)(rng() % 100); break;
        case KIND: live_source()->kind = side ? 3 + (int)(rng() % 100) : -1 - (int)(rng() % 100); break;
        case AMP_NOT_FINITE: live_source()->amp = bad_values[rng() % 3 == 2 ? 0 : rng() % 2]; break;
        case AMP_NEGATIVE: live_source()->amp = (rng() & 1) ? -1e-30f : -(float)(1 + rng() % 100); break;
        case GATE_ON: { auto* S = live_source(); S->gate_period = side ? rng() >> 1 : rng() % 5000; S->gate_on = S->gate_period + 1 + (side ? rng() >> 2 : 0); } break;
        case GATE_OFFSET: live_source()->gate_offset = side ? DABGPU_INTERFERER_MAX_POSITION + (int64_t)(rng() % 1000) : -DABGPU_INTERFERER_MAX_POSITION - (int64_t)(rng() % 1000); break;
        case SHAPE_INDEX: { auto* S = live_source(); S->kind = DABGPU_INTERFERER_BAND; S->shape = side ? n_shapes + (int)(rng() % 100) : -2 - (int)(rng() % 100); } break;
        default: break;
        }
        if (kind == AMP_NOT_FINITE) { auto* S = live_source(); if (std::isfinite(S->amp)) S->amp = bad_values[0]; }
        dabgpu_interferer_geometry g;
        std::memset(&g, 0x5A, sizeof(g));
        const bool want_g = rng() % 9 != 0;
        const int st = dabgpu_interferer_plan(list, n_arg, shape_list, n_shapes_arg, want_g ? &g : nullptr);
        const bool expect_ok = kind == OK || !planted;
        bool ok = expect_ok ? st == DABGPU_OK : st == DABGPU_ERR_INVALID_ARG;
        if (ok && expect_ok && want_g)
            ok = g.block_samples == DABGPU_INTERFERER_BLOCK && g.band_slots == slots && g.slot_bytes == (slots ? slot_bytes : 0u) && g.lds_bytes == slots * slot_bytes &&
                 g.lds_bytes <= 4u * 8400u;
        if (ok) { if (planted) reached[kind][side]++; if (expect_ok) banded[slots != 0]++; }
        else { failed++; if (failed < 5) std::fprintf(stderr, "case %ld: kind %d side %d status %d (%s)\n", it, kind, side, st, dabgpu_last_error()); }
        // set_params against the geometry of a bank's creation
        {
            const dabgpu_interferer_geometry created = {1024, (uint32_t)(rng() % 5), 8400, 0}, wanted = {1024, (uint32_t)(rng() % 5), 8400, 0};
            const bool fit = wanted.band_slots <= created.band_slots;
            if ((dabgpu_host_interferer_fits(created, wanted) == DABGPU_OK) != fit) failed++; else fits[fit]++;
        }
        // the design: every width in range gives a power of two and a table of finite taps scaled to a mean per-phase energy of 1/2
        {
            const bool good = rng() & 1;
            const double w = good ? DABGPU_INTERFERER_MIN_WIDTH + (1.0 - DABGPU_INTERFERER_MIN_WIDTH) * (double)(rng() % 100001) / 100000.0
                                  : ((rng() & 1) ? 1.0 + 1e-9 * (double)(1 + rng() % 1000) : DABGPU_INTERFERER_MIN_WIDTH * (1.0 - 1e-9 * (double)(1 + rng() % 1000)));
            if (it % 100 == 0) {                                                              // (a design costs a spectrum: not every iteration)
                dabgpu_interferer_shape H;
                const int sd = dabgpu_interferer_design(w, &H);
                bool okd = good ? sd == DABGPU_OK : sd == DABGPU_ERR_INVALID_ARG;
                if (okd && good) {
                    double e = 0.0;
                    for (int j = 0; j < 16 * H.interp; j++) e += (double)H.taps[j] * (double)H.taps[j];
                    okd = H.interp >= 1 && H.interp <= 64 && !(H.interp & (H.interp - 1)) && w * H.interp + DABGPU_INTERFERER_TRANSITION <= 1.0 + (H.interp == 1) &&
                          std::fabs(e / H.interp - 0.5) < 1e-6 && H.inband_share > 0.9 && H.inband_share <= 1.0 && H.phase_ripple >= 1.0;
                }
                if (okd) designs[good]++; else { failed++; if (failed < 5) std::fprintf(stderr, "design %g: status %d\n", w, sd); }
            }
        }
        // the arguments of an apply call: one defect at most, each rule on both of its sides
        {
            const int ak = (int)(rng() % A_KINDS), as = (int)(rng() & 1);
            const int fmt = (rng() & 1) ? DABGPU_IQ_RAW_F32L : DABGPU_IQ_RAW_U8;
            const size_t sb = fmt == DABGPU_IQ_RAW_F32L ? 8 : 2;
            size_t streams = 1 + rng() % 64, n_out = rng() % 300000;
            size_t in_stride = (rng() % 3 == 0) ? 0 : ((n_out + 1) & ~(size_t)1) + 2 * (rng() % 50);
            const size_t row = (n_out * sb + 15) & ~(size_t)15;
            size_t out_stride = (rng() % 3 == 0) ? 0 : row + 16 * (rng() % 50);
            uintptr_t in = (rng() % 4 == 0) ? 0 : 0x10000 + 16 * (rng() % 1000), out = 0x900000 + 16 * (rng() % 1000);
            float scale = (float)(rng() % 1000) / 10.0f;
            int f = fmt;
            if (ak == A_OK && rng() % 4 == 0 && in) {                                        // a legal in-place call
                f = DABGPU_IQ_RAW_F32L; in = out; in_stride = (((n_out * 8 + 15) & ~(size_t)15) + 16 * (rng() % 50)) / 8; out_stride = in_stride * 8; in_place_ok++;
            }
            switch (ak) {
            case A_FORMAT: f = as ? 11 + (int)(rng() % 20) : 1 + (int)(rng() % 9); break;
            case A_N_OUT: n_out = ((size_t)1 << 31) + 1 + rng() % 9; out_stride = 0; in_stride = 0; streams = 1; break;
            case A_NULL_OUT: out = 0; if (n_out == 0) n_out = 1; out_stride = 0; break;
            case A_IN_STRIDE: if (!in) in = 0x10000; if (n_out < 2) n_out = 2 + rng() % 1000; out_stride = 0; in_stride = as ? (n_out | 1) + 2 * (rng() % 9) : (n_out - 1); break;
            case A_OUT_STRIDE: if (n_out == 0) n_out = 1 + rng() % 1000; out_stride = as ? ((n_out * (f == DABGPU_IQ_RAW_F32L ? 8 : 2) + 15) & ~(size_t)15) + 8 : ((n_out * (f == DABGPU_IQ_RAW_F32L ? 8 : 2) + 15) & ~(size_t)15) - 16; if (out_stride == 0) out_stride = 8; if (in_stride && in_stride < n_out) in_stride = 0; break;
            case A_ALIGN: if (as || !in) out += 8; else in += 4 << (rng() % 2); break;
            case A_IN_PLACE: in = out; if (n_out == 0) n_out = 1 + rng() % 1000; if (as) { f = DABGPU_IQ_RAW_U8; in_stride = (n_out + 1) & ~(size_t)1; out_stride = 0; } else { f = DABGPU_IQ_RAW_F32L; streams = 2 + rng() % 9; in_stride = ((n_out + 1) & ~(size_t)1) + 2; out_stride = in_stride * 8 + 16; } break;
            case A_SCALE: f = DABGPU_IQ_RAW_U8; scale = bad_values[rng() % 3]; out_stride = 0; break;
            case A_GRID: streams = (size_t)1 << 20; n_out = (size_t)1 << 22; out_stride = 0; in_stride = 0; break;
            default: break;
            }
            size_t stride_io = out_stride;
            const size_t row2 = (n_out * (f == DABGPU_IQ_RAW_F32L ? 8 : 2) + 15) & ~(size_t)15;
            if (ak == A_OK && in && in == out) {}                                           // (strides set above)
            else if (ak == A_OK || ak == A_ALIGN || ak == A_FORMAT) { if (out_stride) out_stride = stride_io = row2 + 16 * (rng() % 50); }
            const int st2 = dabgpu_host_interferer_check_apply("fuzz", streams, (const void*)in, in_stride, n_out, (const void*)out, f, &stride_io, scale);
            bool ok2 = (ak == A_OK) ? st2 == DABGPU_OK : st2 == DABGPU_ERR_INVALID_ARG;
            if (ok2 && ak == A_OK) { ok2 = stride_io == (out_stride ? out_stride : row2); if (!in) no_input++; }
            if (ok2) apply_reached[ak][as]++;
            else { failed++; if (failed < 5) std::fprintf(stderr, "apply case %ld: kind %d side %d status %d (%s)\n", it, ak, as, st2, dabgpu_last_error()); }
        }
    }
    std::printf("{\"iterations\": %ld, \"failed_checks\": %ld, \"accepted\": %ld, \"tones_only\": %ld, \"banded\": %ld, \"fits_no\": %ld, \"fits_yes\": %ld, "
                "\"designs_ok\": %ld, \"designs_refused\": %ld, \"apply_no_input\": %ld, \"apply_in_place\": %ld",
                iters, failed, reached[OK][0] + reached[OK][1], banded[0], banded[1], fits[0], fits[1], designs[1], designs[0], no_input, in_place_ok);
    const char* names[N_KINDS] = {"", "n_streams", "n_shapes", "null_lists", "interp", "tap_value", "n_sources", "kind", "amp_not_finite", "amp_negative",
                                  "gate_on", "gate_offset", "shape_index"};
    for (int k = 1; k < N_KINDS; k++) std::printf(", \"%s_low\": %ld, \"%s_high\": %ld", names[k], reached[k][0], names[k], reached[k][1]);
    const char* anames[A_KINDS] = {"apply_ok", "apply_format", "apply_n_out", "apply_null_out", "apply_in_stride", "apply_out_stride", "apply_align",
                                   "apply_in_place", "apply_scale", "apply_grid"};
    for (int k = 0; k < A_KINDS; k++) std::printf(", \"%s_a\": %ld, \"%s_b\": %ld", anames[k], apply_reached[k][0], anames[k], apply_reached[k][1]);
    std::printf("}\n");
    return failed ? 1 : 0;
}
