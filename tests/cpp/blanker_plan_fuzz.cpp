// blanker_plan_fuzz.cpp -- dabgpu_blanker_plan, dabgpu_blanker_input_needed and the argument rules of an apply call
// (dab-radio_amd/csrc/dabgpu_host_logic.cpp), run plain and under ASan + UBSan (tests/test_blanker_plan.py builds it): random parameter
// lists with at most one defect each, allocated exactly so that a read past a list is caught; an acceptance is checked against the
// geometry the header states, a refusal against the defect planted.
//   blanker_plan_fuzz <iterations> <seed>  -> one JSON line with how often each side of every decision was reached
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
    enum { OK, N_STREAMS, NULL_LIST, THRESHOLD_NOT_FINITE, THRESHOLD, WINDOW, GAP, GUARD, START, N_KINDS };
    enum { A_OK, A_N_IN, A_N_OUT, A_NULL, A_IN_STRIDE, A_OUT_STRIDE, A_ALIGN, A_IN_PLACE, A_MASK_STRIDE, A_MASK_ALIGN, A_GRID, A_KINDS };
    static const char* names[N_KINDS] = {"accepted", "n_streams", "null_list", "threshold_not_finite", "threshold", "window", "gap", "guard", "start"};
    static const char* a_names[A_KINDS] = {"apply_ok", "apply_n_in", "apply_n_out", "apply_null", "apply_in_stride", "apply_out_stride", "apply_align",
                                           "apply_in_place", "apply_mask_stride", "apply_mask_align", "apply_grid"};
    long failed = 0, reached[N_KINDS][2] = {}, apply_reached[A_KINDS][2] = {}, fits[2] = {}, needed[2] = {};
    const float bad_values[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
    auto fail = [&](const char* what, long it) { if (failed++ < 10) std::fprintf(stderr, "iteration %ld: %s (%s)\n", it, what, dabgpu_last_error()); };
    for (long it = 0; it < iters; it++) {
        const int kind = (int)(rng() % N_KINDS), side = (int)(rng() & 1);
        size_t n = 1 + rng() % 5;
        std::vector<dabgpu_blanker_stream> v(n);
        uint32_t reach = 0;
        for (auto& P : v) {
            std::memset(&P, 0, sizeof(P));
            P.start = (int64_t)rng() >> 2;
            if (rng() % 5 == 0) P.start = (rng() & 1) ? DABGPU_BLANKER_MAX_POSITION : -DABGPU_BLANKER_MAX_POSITION;   // (the edges are accepted)
            P.threshold = (rng() % 5 == 0) ? ((rng() & 1) ? 1024.0f : std::nextafterf(1.0f, 2.0f)) : 1.5f + (float)(rng() % 1000) / 10.0f;
            P.window = 1 + (int)(rng() % 32); P.gap = (int)(rng() % 33); P.guard = (int)(rng() % 5);
            P.enabled = (int)(rng() % 3) - 1; P.reserved = (int)rng();
            reach = std::max(reach, (uint32_t)(P.gap + P.window + P.guard));
        }
        dabgpu_blanker_stream& B = v[rng() % n];
        const dabgpu_blanker_stream* list = v.data();
        switch (kind) {
            case N_STREAMS: n = side ? ((size_t)1 << 20) + 1 + rng() % 1000 : 0; break;      // (refused before the list is read)
            case NULL_LIST: list = nullptr; break;
            case THRESHOLD_NOT_FINITE: B.threshold = bad_values[rng() % 3]; break;
            case THRESHOLD: B.threshold = side ? std::nextafterf(1024.0f, 2048.0f) * (1.0f + (float)(rng() % 100)) : 1.0f - (float)(rng() % 100) * 0.5f; break;
            case WINDOW: B.window = side ? 33 + (int)(rng() % 1000) : -(int)(rng() % 1000); break;
            case GAP: B.gap = side ? 33 + (int)(rng() % 1000) : -1 - (int)(rng() % 1000); break;
            case GUARD: B.guard = side ? 5 + (int)(rng() % 1000) : -1 - (int)(rng() % 1000); break;
            case START: B.start = side ? DABGPU_BLANKER_MAX_POSITION + 1 + (int64_t)(rng() % 1000) : -DABGPU_BLANKER_MAX_POSITION - 1 - (int64_t)(rng() % 1000); break;
            default: break;
        }
        dabgpu_blanker_geometry g;
        std::memset(&g, 0xEE, sizeof(g));
        const int st = dabgpu_blanker_plan(list, n, &g);
        reached[kind][side]++;
        if (kind == OK) {
            if (st != DABGPU_OK || g.reach_blocks != reach || g.block_samples != 1024 || g.lds_bytes != (32 + 2 * reach) * 4 + 40 * 4 || g.reserved != 0)
                fail("an acceptance with the wrong geometry", it);
            // _set_params: a list of its own against this geometry
            dabgpu_blanker_geometry w = g;
            w.reach_blocks = (uint32_t)(rng() % 69);
            const int fit = dabgpu_host_blanker_fits(g, w);
            fits[fit == DABGPU_OK]++;
            if ((fit == DABGPU_OK) != (w.reach_blocks <= g.reach_blocks)) fail("fits", it);
            // input_needed of one stream of the list
            const uint64_t pos = (rng() % 4 == 0) ? (uint64_t)DABGPU_BLANKER_MAX_POSITION - rng() % 5000 : rng() % 100000;
            const size_t n_out = (rng() % 8 == 0) ? 0 : rng() % 5000;
            int64_t first = 7; uint64_t count = 7;
            const int ns = dabgpu_blanker_input_needed(&B, pos, n_out, &first, &count);
            const int64_t r = B.enabled ? B.gap + B.window + B.guard : 0;
            auto index = [&](int64_t m) { const __int128 i = (__int128)m - (__int128)B.start; return i > (__int128)INT64_MAX ? INT64_MAX : (int64_t)i; };
            needed[n_out != 0]++;
            if (ns != DABGPU_OK) fail("input_needed refused", it);
            else if (n_out == 0) { if (count != 0) fail("input_needed of nothing", it); }
            else if (!B.enabled) { if (first != index((int64_t)pos) || count != n_out) fail("input_needed of a disabled stream", it); }
            else {
                const int64_t b0 = (int64_t)(pos / 32) - r, b1 = (int64_t)((pos + n_out - 1) / 32) + r;
                if (first != index(b0 * 32) || count != (uint64_t)(b1 - b0 + 1) * 32) fail("input_needed", it);
                if (first != INT64_MAX && ((__int128)first > (__int128)pos - B.start - 32 * r ||
                                           (__int128)first + count < (__int128)(pos + n_out) - B.start + 32 * r)) fail("input_needed covers too little", it);
            }
        } else {
            if (st != DABGPU_ERR_INVALID_ARG || g.reach_blocks != 0 || g.block_samples != 1024 || g.lds_bytes != 0) fail("a defect accepted, or a geometry left behind", it);
            const char* e = dabgpu_last_error();
            const char* want = kind == N_STREAMS ? "streams" : kind == NULL_LIST ? "null parameters" : kind == THRESHOLD_NOT_FINITE ? "threshold is not finite"
                             : kind == THRESHOLD ? "threshold" : kind == WINDOW ? "window" : kind == GAP ? "gap" : kind == GUARD ? "guard" : "start";
            if (!std::strstr(e, want)) fail("the refusal names another field", it);
        }

        // the argument rules of an apply call: fake addresses, never dereferenced
        const int akind = (int)(rng() % A_KINDS), aside = (int)(rng() & 1);
        size_t streams = 1 + rng() % 8, n_out = rng() % 9000, n_in = 1 + rng() % 9000;
        size_t in_stride = (rng() & 1) ? 0 : ((n_in + 1) & ~(size_t)1) + 2 * (rng() % 4);
        size_t out_stride = (rng() & 1) ? 0 : ((n_out * 8 + 15) & ~(size_t)15) + 16 * (rng() % 4);
        size_t mask_stride = (rng() & 1) ? 0 : n_out / 1024 + 2 + rng() % 3;
        uintptr_t in = 0x10000, out = 0x900000, mask = (rng() & 1) ? 0 : 0x2000004;
        switch (akind) {
            case A_N_IN: n_in = aside ? ((size_t)1 << 40) + 1 : 0; if (in_stride) in_stride = (size_t)1 << 41; break;
            case A_N_OUT: n_out = ((size_t)1 << 31) + 1 + rng() % 100; out_stride = 0; mask_stride = 0; break;
            case A_NULL: if (aside) in = 0; else { out = 0; if (n_out == 0) n_out = 1; out_stride = 0; mask_stride = 0; } break;
            case A_IN_STRIDE: in_stride = aside ? ((n_in + 1) & ~(size_t)1) + 1 : (n_in > 1 ? n_in - 1 : 1); if (!aside && n_in == 1) { n_in = 3; in_stride = 2; } break;
            case A_OUT_STRIDE: if (n_out < 3) n_out = 3; mask_stride = 0; out_stride = aside ? ((n_out * 8 + 15) & ~(size_t)15) + 8 : ((n_out * 8 + 15) & ~(size_t)15) - 16; break;
            case A_ALIGN: if (aside) in += 8; else out += 8; break;
            case A_IN_PLACE: in = out; break;
            case A_MASK_STRIDE: mask_stride = 1 + rng() % (n_out / 1024 + 1); break;
            case A_MASK_ALIGN: mask = 0x2000004 + 1 + rng() % 3; break;
            case A_GRID: streams = (size_t)1 << 20; n_out = (size_t)1 << 31; out_stride = 0; mask_stride = 0; break;
            default: break;
        }
        size_t out_stride_io = out_stride, mask_stride_io = mask_stride;
        const int as = dabgpu_host_blanker_check_apply("fuzz", streams, (const void*)in, in_stride, n_in, n_out, (const void*)out, &out_stride_io, (const void*)mask,
                                                       &mask_stride_io);
        apply_reached[akind][aside]++;
        if (akind == A_OK) {
            if (as != DABGPU_OK) fail("a good apply call refused", it);
            if (out_stride_io != (out_stride ? out_stride : ((n_out * 8 + 15) & ~(size_t)15))) fail("the default output stride", it);
            if (mask_stride_io != (mask_stride ? mask_stride : n_out / 1024 + 2) || dabgpu_blanker_mask_words(n_out) != n_out / 1024 + 2) fail("the default mask stride", it);
        } else if (as != DABGPU_ERR_INVALID_ARG) fail(a_names[akind], it);
    }
    std::printf("{\"failed_checks\": %ld", failed);
    for (int k = 0; k < N_KINDS; k++) std::printf(", \"%s_low\": %ld, \"%s_high\": %ld", names[k], reached[k][0], names[k], reached[k][1]);
    for (int k = 0; k < A_KINDS; k++) std::printf(", \"%s_a\": %ld, \"%s_b\": %ld", a_names[k], apply_reached[k][0], a_names[k], apply_reached[k][1]);
    std::printf(", \"fits_no\": %ld, \"fits_yes\": %ld, \"needed_none\": %ld, \"needed_some\": %ld}\n", fits[0], fits[1], needed[0], needed[1]);
    return failed ? 1 : 0;
}
