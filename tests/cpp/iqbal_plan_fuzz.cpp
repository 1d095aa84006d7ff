// iqbal_plan_fuzz.cpp -- dabgpu_iqbal_plan, dabgpu_iqbal_impairment, dabgpu_iqbal_forget, dabgpu_iqbal_solve_host and the argument rules
// of an apply call (dab-radio_amd/csrc/dabgpu_host_logic.cpp), run plain and under ASan + UBSan (tests/test_iqbal_plan.py builds it):
// random parameter lists with at most one defect each, allocated exactly so that a read past a list is caught; an acceptance is checked
// against the geometry the header states, a refusal against the defect planted; the solve takes any bit pattern as its state and must
// leave finite coefficients.
//   iqbal_plan_fuzz <iterations> <seed>  -> one JSON line with how often each side of every decision was reached
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
    enum { OK, N_STREAMS, NULL_LIST, MODE, COEF, FORGET, MIN_WEIGHT, MAX_CALL, N_KINDS };
    enum { A_OK, A_FLAGS, A_N, A_NULL, A_IN_STRIDE, A_OUT_STRIDE, A_ALIGN, A_IN_PLACE, A_MEASURE_N, A_MEASURE_MAX, A_KINDS };
    static const char* names[N_KINDS] = {"accepted", "n_streams", "null_list", "mode", "coef", "forget", "min_weight", "max_call"};
    static const char* a_names[A_KINDS] = {"apply_ok", "apply_flags", "apply_n", "apply_null", "apply_in_stride", "apply_out_stride", "apply_align",
                                           "apply_in_place", "apply_measure_n", "apply_measure_max"};
    long failed = 0, reached[N_KINDS][2] = {}, apply_reached[A_KINDS][2] = {}, solved[2] = {}, impaired[2] = {};
    const float bad_values[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
    auto fail = [&](const char* what, long it) { if (failed++ < 10) std::fprintf(stderr, "iteration %ld: %s (%s)\n", it, what, dabgpu_last_error()); };
    auto unit = [&]() { return (float)((double)(rng() % 2000001) / 1e6 - 1.0); };
    for (long it = 0; it < iters; it++) {
        const int kind = (int)(rng() % N_KINDS), side = (int)(rng() & 1);
        size_t n = 1 + rng() % 5;
        size_t max_call = 1024 * (1 + rng() % 300);
        if (rng() % 6 == 0) max_call = (rng() & 1) ? 1024 : (size_t)1 << 31;                      // (the edges are accepted)
        std::vector<dabgpu_iqbal_stream> v(n);
        for (auto& P : v) {
            std::memset(&P, 0, sizeof(P));
            P.mode = (int)(rng() % 3); P.reserved = (int)rng();
            P.a_re = 1.0f + 0.1f * unit(); P.a_im = unit(); P.b_re = unit(); P.b_im = unit(); P.c_re = 100.0f * unit(); P.c_im = unit();
            P.forget = (rng() % 5 == 0) ? ((rng() & 1) ? 1.0f : std::numeric_limits<float>::denorm_min()) : 0.5f + 0.5f * std::fabs(unit());
            if (P.forget == 0.0f) P.forget = 1.0f;
            P.min_weight = (rng() % 5 == 0) ? 1024.0f : 1024.0f + (float)(rng() % 1000000);
        }
        dabgpu_iqbal_stream& B = v[rng() % n];
        const dabgpu_iqbal_stream* list = v.data();
        size_t n_arg = n;
        switch (kind) {
            case N_STREAMS: n_arg = side ? ((size_t)1 << 20) + 1 + rng() % 1000 : 0; break;        // (refused before the list is read)
            case NULL_LIST: list = nullptr; break;
            case MODE: B.mode = side ? 3 + (int)(rng() % 1000) : -1 - (int)(rng() % 1000); break;
            case COEF: (&B.a_re)[rng() % 6] = bad_values[rng() % 3]; break;
            case FORGET: B.forget = side ? std::nextafterf(1.0f, 2.0f) * (1.0f + (float)(rng() % 100)) : ((rng() & 1) ? -(float)(rng() % 100) : bad_values[0]); break;
            case MIN_WEIGHT: B.min_weight = side ? bad_values[rng() % 3] : std::nextafterf(1024.0f, 0.0f) - (float)(rng() % 5000); break;
            case MAX_CALL: max_call = side ? (((size_t)1 << 31) + 1024 * (1 + rng() % 100)) : ((rng() & 1) ? rng() % 1024 : 1024 * (1 + rng() % 300) + 1 + rng() % 1023); break;
            default: break;
        }
        dabgpu_iqbal_geometry g;
        std::memset(&g, 0xEE, sizeof(g));
        const int st = dabgpu_iqbal_plan(list, n_arg, max_call, &g);
        reached[kind][side]++;
        const bool grid_too_large = (uint64_t)(max_call / 1024) * n > 0x7FFFFFFFull;                 // (never with n <= 5)
        if (kind == OK && !grid_too_large) {
            if (st != DABGPU_OK || g.tile_samples != 1024 || g.tiles_per_call != max_call / 1024 || g.scratch_bytes != (uint64_t)(max_call / 1024) * n * 32)
                fail("an acceptance with the wrong geometry", it);
            // the solve of any state: the coefficients stay finite, identity unless valid
            dabgpu_iqbal_record R;
            std::memset(&R, 0, sizeof(R));
            uint32_t w[6];
            for (auto& x : w) x = (uint32_t)rng();
            if (rng() & 1) { R.N = 1e6f * (0.5f + std::fabs(unit())); for (int k = 0; k < 5; k++) R.S[k] = R.N * unit() * (k == 2 ? -1.0f : 1.0f); R.S[2] = std::fabs(R.S[2]) + 0.1f * R.N; }
            else { std::memcpy(&R.N, &w[0], 4); std::memcpy(R.S, &w[1], 20); }
            R.tiles_used = 77; R.tiles_skipped = 5; R.calls_refused = 3;
            const int ss = dabgpu_iqbal_solve_host(&B, &R);
            solved[R.valid != 0]++;
            if (ss != DABGPU_OK || R.tiles_used != 77 || R.tiles_skipped != 5 || R.calls_refused != 3) fail("solve_host", it);
            const float k6[6] = {R.a_re, R.a_im, R.b_re, R.b_im, R.c_re, R.c_im};
            if (R.valid > 1 || R.a_re != 1.0f || R.a_im != 0.0f) fail("solve_host: a is not 1", it);
            if (!R.valid && (R.b_re != 0.0f || R.b_im != 0.0f || R.c_re != 0.0f || R.c_im != 0.0f)) fail("solve_host: not valid, not identity", it);
            if (R.valid) {
                if (!(R.N >= B.min_weight) || !(R.P > 0.0f) || !(R.C_re * R.C_re + R.C_im * R.C_im < 1.0001f) || !(R.w_re * R.w_re + R.w_im * R.w_im < 1.0001f))
                    fail("solve_host: valid outside its conditions", it);
                for (float x : k6) if (!std::isfinite(x) && std::isfinite(R.d_re) && std::isfinite(R.d_im)) fail("solve_host: a coefficient is not finite", it);
            }
            // the impairment: inside its range a FIXED stream the planner accepts, outside refused
            const bool in_range = (rng() & 1) != 0;
            const double gdb = in_range ? 20.0 * unit() : (20.0 + 1e-9 + (double)(rng() % 100)) * ((rng() & 1) ? 1 : -1);
            const double pdeg = 45.0 * unit();
            dabgpu_iqbal_stream F;
            const int is = dabgpu_iqbal_impairment(gdb, pdeg, unit(), unit(), &F);
            impaired[in_range]++;
            if (in_range != (is == DABGPU_OK)) fail("impairment range", it);
            if (is == DABGPU_OK) {
                if (F.mode != DABGPU_IQBAL_FIXED || dabgpu_iqbal_plan(&F, 1, 1024, nullptr) != DABGPU_OK) fail("impairment: not a stream the planner accepts", it);
                if (std::fabs((F.a_re + F.b_re) - 1.0f) > 1e-6f || std::fabs(F.a_im - F.b_im) > 0.0f) fail("impairment: K1 + K2 is not 1 + j 2 Im K1", it);
            }
            const float lam = dabgpu_iqbal_forget(1024.0 + (double)(rng() % 10000000));
            if (!(lam > 0.36f && lam < 1.0f) || dabgpu_iqbal_forget(1023.0) != 0.0f || dabgpu_iqbal_forget(INFINITY) != 1.0f) fail("forget", it);
        } else if (kind != OK) {
            if (st != DABGPU_ERR_INVALID_ARG || g.tile_samples != 1024 || g.tiles_per_call != 0 || g.scratch_bytes != 0) fail("a defect accepted, or a geometry left behind", it);
            const char* e = dabgpu_last_error();
            const char* want = kind == N_STREAMS ? "streams" : kind == NULL_LIST ? "null parameters" : kind == MODE ? "mode" : kind == COEF ? "is not finite"
                             : kind == FORGET ? "forget" : kind == MIN_WEIGHT ? "min_weight" : "max_samples_per_call";
            if (!std::strstr(e, want)) fail("the refusal names another field", it);
        }

        // the argument rules of an apply call: fake addresses, never dereferenced
        const int akind = (int)(rng() % A_KINDS), aside = (int)(rng() & 1);
        dabgpu_iqbal_geometry geom = {1024, (uint32_t)(1 + rng() % 16), 0};
        size_t streams = 1 + rng() % 8;
        uint32_t flags = 1 + (uint32_t)(rng() % 3);
        const bool measure = (flags & DABGPU_IQBAL_MEASURE) != 0;
        size_t cnt = measure ? 1024 * (1 + rng() % geom.tiles_per_call) : 1 + rng() % 9000;
        int fmt = (rng() & 1) ? DABGPU_IQ_RAW_F32L : DABGPU_IQ_RAW_U8;
        const size_t sb = fmt == DABGPU_IQ_RAW_F32L ? 8 : 2;
        size_t in_stride = (rng() & 1) ? 0 : ((cnt + 1) & ~(size_t)1) + 2 * (rng() % 4);
        size_t out_stride = (rng() & 1) ? 0 : ((cnt * sb + 15) & ~(size_t)15) + 16 * (rng() % 4);
        uintptr_t in = 0x10000, out = 0x900000;
        switch (akind) {
            case A_FLAGS: flags = aside ? 4 + (uint32_t)(rng() % 1000) : 0; break;
            case A_N: cnt = aside ? ((size_t)1 << 31) + 1024 : 0; in_stride = 0; out_stride = 0; geom.tiles_per_call = 0xFFFFFFFFu; break;
            case A_NULL: if (aside) in = 0; else { out = 0; flags |= DABGPU_IQBAL_APPLY; } break;
            case A_IN_STRIDE: in_stride = aside ? ((cnt + 1) & ~(size_t)1) + 1 : cnt - 1; if (in_stride == 0) { cnt = 1024; in_stride = 1022; } break;
            case A_OUT_STRIDE: flags |= DABGPU_IQBAL_APPLY; if (cnt < 16) cnt = 1024; out_stride = aside ? ((cnt * sb + 15) & ~(size_t)15) + 8 : ((cnt * sb + 15) & ~(size_t)15) - 16; break;
            case A_ALIGN: if (aside) in += 8; else { out += 8; flags |= DABGPU_IQBAL_APPLY; } break;
            case A_IN_PLACE: flags |= DABGPU_IQBAL_APPLY; out = in;                                  // u8 in place, or rows of another stride
                if (aside) { fmt = DABGPU_IQ_RAW_U8; out_stride = 0; }
                else { fmt = DABGPU_IQ_RAW_F32L; in_stride = (cnt + 1) & ~(size_t)1; out_stride = in_stride * 8 + 16; }
                break;
            case A_MEASURE_N: flags |= DABGPU_IQBAL_MEASURE; cnt = 1024 * (rng() % geom.tiles_per_call) + 1 + rng() % 1023; in_stride = 0; out_stride = 0; break;
            case A_MEASURE_MAX: flags |= DABGPU_IQBAL_MEASURE; cnt = 1024 * ((size_t)geom.tiles_per_call + 1 + rng() % 5); in_stride = 0; out_stride = 0; break;
            default: break;
        }
        size_t out_stride_io = out_stride;
        const int as = dabgpu_host_iqbal_check_apply("fuzz", streams, geom, (const void*)in, in_stride, cnt, (const void*)out, fmt, &out_stride_io, 1.0f, flags);
        apply_reached[akind][aside]++;
        if (akind == A_OK) {
            if (as != DABGPU_OK) fail("a good apply call refused", it);
            if ((flags & DABGPU_IQBAL_APPLY) && out_stride_io != (out_stride ? out_stride : ((cnt * sb + 15) & ~(size_t)15))) fail("the default output stride", it);
        } else if (as != DABGPU_ERR_INVALID_ARG) fail(a_names[akind], it);
    }
    std::printf("{\"failed_checks\": %ld", failed);
    for (int k = 0; k < N_KINDS; k++) std::printf(", \"%s_low\": %ld, \"%s_high\": %ld", names[k], reached[k][0], names[k], reached[k][1]);
    for (int k = 0; k < A_KINDS; k++) std::printf(", \"%s_a\": %ld, \"%s_b\": %ld", a_names[k], apply_reached[k][0], a_names[k], apply_reached[k][1]);
    std::printf(", \"solved_identity\": %ld, \"solved_valid\": %ld, \"impairment_refused\": %ld, \"impairment_ok\": %ld}\n", solved[0], solved[1], impaired[0], impaired[1]);
    return failed ? 1 : 0;
}
