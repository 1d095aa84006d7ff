// channel_plan_fuzz.cpp -- dabgpu_channel_plan and the frequency conversions (dab-radio_amd/csrc/dabgpu_host_logic.cpp) under ASan + UBSan
// (tests/test_channel_plan.py builds it): random parameter lists with at most one defect each, allocated exactly so that a read past the
// list is caught; an acceptance is checked against the geometry the header states, a refusal against the defect planted.
//   channel_plan_fuzz <iterations> <seed>  -> one JSON line with how often each side of every decision was reached
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
    enum { OK, N_STREAMS, TAPS, DELAY, GAIN, SIGMA_NAN, SIGMA_NEG, TAP_VALUE, START, NULL_PARAMS, N_KINDS };
    // reached[kind][side]: side 0 = the low edge of a refusal (0 streams, < 1 tap, delay < 0, start < -2^62), 1 = the high one
    long failed = 0, reached[N_KINDS][2] = {}, staged[2] = {}, round_trips = 0;
    enum { A_OK, A_FORMAT, A_N_IN, A_N_OUT, A_NULL, A_IN_STRIDE, A_OUT_STRIDE, A_ALIGN, A_SCALE, A_GRID, A_KINDS };
    long apply_reached[A_KINDS][2] = {}, fits[2][2] = {};
    const float bad_values[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
    for (long it = 0; it < iters; it++) {
        const int kind = (int)(rng() % N_KINDS);
        const size_t n = 1 + rng() % 6;
        std::vector<dabgpu_channel_stream> v(n);
        uint32_t halo = 0, any_staged = 0;
        const bool all_direct = rng() % 4 == 0;
        for (auto& P : v) {
            std::memset(&P, 0, sizeof(P));
            P.freq_q64 = rng(); P.phase0_q64 = rng(); P.start = (int64_t)rng() >> 1; P.seed = rng();         // |start| <= 2^62
            if (rng() % 7 == 0) P.start = (rng() & 1) ? DABGPU_CHANNEL_MAX_POSITION : -DABGPU_CHANNEL_MAX_POSITION;   // (the edges are accepted)
            P.gain = (float)(rng() % 2000) / 100.0f - 10.0f;
            P.noise_sigma = (rng() % 3 == 0) ? 0.0f : (float)(rng() % 1000) / 100.0f;
            P.n_taps = all_direct ? 1 : 1 + (int)(rng() % 8);
            for (int k = 0; k < 8; k++) {                                        // (entries past n_taps may hold anything)
                P.tap_delay[k] = (k < P.n_taps) ? (all_direct ? 0 : (int)(rng() % 2048)) : (int)rng();
                if (k < P.n_taps && rng() % 5 == 0) P.tap_delay[k] = (rng() & 1) ? 0 : 2047;
                P.tap_re[k] = (k < P.n_taps) ? (float)(rng() % 200) / 100.0f - 1.0f : bad_values[rng() % 3];
                P.tap_im[k] = (k < P.n_taps) ? (float)(rng() % 200) / 100.0f - 1.0f : bad_values[rng() % 3];
                if (k < P.n_taps) halo = std::max(halo, ((uint32_t)P.tap_delay[k] + 1u) & ~1u);
            }
            if (!(P.n_taps == 1 && P.tap_delay[0] == 0)) any_staged = 1;
        }
        dabgpu_channel_stream& B = v[rng() % n];
        const int k = (int)(rng() % (unsigned)B.n_taps);
        size_t n_arg = n;
        const int side = (int)(rng() & 1);
        const dabgpu_channel_stream* list = v.data();
        switch (kind) {
        case N_STREAMS: n_arg = side ? ((size_t)1 << 20) + 1 + rng() % 5 : 0; break;
        case TAPS: B.n_taps = side ? 9 + (int)(rng() % 100) : (rng() & 1 ? 0 : -(int)(rng() % 100)); break;
        case DELAY: B.tap_delay[k] = side ? 2048 + (int)(rng() % 100000) : -1 - (int)(rng() % 100); break;
        case START: B.start = side ? DABGPU_CHANNEL_MAX_POSITION + 1 + (int64_t)(rng() % 1000) : -DABGPU_CHANNEL_MAX_POSITION - 1 - (int64_t)(rng() % 1000); break;
        case NULL_PARAMS: list = nullptr; break;
        case GAIN: B.gain = bad_values[rng() % 3]; break;
        case SIGMA_NAN: B.noise_sigma = bad_values[rng() % 2]; break;
        case SIGMA_NEG: B.noise_sigma = (rng() & 1) ? -1e-30f : -(float)(1 + rng() % 100); break;
        case TAP_VALUE: ((rng() & 1) ? B.tap_re : B.tap_im)[k] = bad_values[rng() % 3]; break;
        default: break;
        }
        dabgpu_channel_geometry g;
        std::memset(&g, 0x5A, sizeof(g));
        // (a list of 2^20 + streams is refused before it is read: the pointer holds n)
        const int st = dabgpu_channel_plan(list, n_arg, (rng() % 9 == 0) ? nullptr : &g);
        bool ok = (kind == OK) ? st == DABGPU_OK : st == DABGPU_ERR_INVALID_ARG;
        if (ok && kind == OK && g.halo != 0x5A5A5A5Au)
            ok = g.halo == halo && g.staged == any_staged && g.block_samples == DABGPU_CHANNEL_BLOCK &&
                 g.lds_bytes == (any_staged ? (DABGPU_CHANNEL_BLOCK + halo + 2) * 8 : 0) && halo <= 2048;
        if (ok) { reached[kind][side]++; if (kind == OK) staged[any_staged]++; }
        else { failed++; if (failed < 5) std::fprintf(stderr, "case %ld: kind %d status %d (%s)\n", it, kind, st, dabgpu_last_error()); }
        // set_params against the geometry of a bank's creation
        {
            const dabgpu_channel_geometry created = {(uint32_t)(2 * (rng() % 1025)), DABGPU_CHANNEL_BLOCK, 0, (uint32_t)(rng() & 1)};
            const dabgpu_channel_geometry wanted = {(rng() % 3 == 0) ? created.halo : (uint32_t)(2 * (rng() % 1025)), DABGPU_CHANNEL_BLOCK, 0, (uint32_t)(rng() & 1)};
            const bool fit = !(wanted.staged && !created.staged) && wanted.halo <= created.halo;
            if ((dabgpu_host_channel_fits(created, wanted) == DABGPU_OK) != fit) failed++;
            else fits[fit][wanted.halo == created.halo]++;
        }
        // the arguments of an apply call: one defect at most, each rule on both of its sides
        {
            const int ak = (int)(rng() % A_KINDS), as = (int)(rng() & 1);
            const int fmt = (rng() & 1) ? DABGPU_IQ_RAW_F32L : DABGPU_IQ_RAW_U8;
            const size_t sb = fmt == DABGPU_IQ_RAW_F32L ? 8 : 2;
            size_t streams = 1 + rng() % 64, n_in = 1 + rng() % 300000, n_out = rng() % 300000;
            size_t in_stride = (rng() % 3 == 0) ? 0 : ((n_in + 1) & ~(size_t)1) + 2 * (rng() % 50);
            const size_t row = (n_out * sb + 15) & ~(size_t)15;
            size_t out_stride = (rng() % 3 == 0) ? 0 : row + 16 * (rng() % 50);
            uintptr_t in = 0x10000 + 16 * (rng() % 1000), out = 0x900000 + 16 * (rng() % 1000);
            float scale = (float)(rng() % 1000) / 10.0f;
            int f = fmt;
            switch (ak) {
            case A_FORMAT: f = as ? 11 + (int)(rng() % 20) : 1 + (int)(rng() % 9); break;
            case A_N_IN: n_in = as ? ((size_t)1 << 40) + 1 + rng() % 9 : 0; in_stride = 0; break;
            case A_N_OUT: n_out = ((size_t)1 << 31) + 1 + rng() % 9; out_stride = 0; streams = 1; break;
            case A_NULL: if (as) { out = 0; if (n_out == 0) n_out = 1; } else in = 0; break;
            case A_IN_STRIDE: in_stride = as ? (n_in | 1) + 2 * (rng() % 9) : (n_in > 1 ? (n_in - 1) & ~(size_t)1 : 1); if (!as && in_stride == 0) in_stride = 1; break;
            case A_OUT_STRIDE: if (n_out == 0) n_out = 1 + rng() % 1000; out_stride = as ? ((n_out * sb + 15) & ~(size_t)15) + 8 : ((n_out * sb + 15) & ~(size_t)15) - 16; if (out_stride == 0) out_stride = 8; break;
            case A_ALIGN: if (as) out += 8; else in += 4 << (rng() % 2); break;
            case A_SCALE: f = DABGPU_IQ_RAW_U8; scale = bad_values[rng() % 3]; out_stride = 0; break;
            case A_GRID: streams = (size_t)1 << 20; n_out = (size_t)1 << 22; out_stride = 0; break;
            default: break;
            }
            size_t stride_io = out_stride;
            const int st2 = dabgpu_host_channel_check_apply("fuzz", streams, (const void*)in, in_stride, n_in, n_out, (const void*)out, f, &stride_io, scale);
            bool ok2 = (ak == A_OK) ? st2 == DABGPU_OK : st2 == DABGPU_ERR_INVALID_ARG;
            if (ok2 && ak == A_OK) ok2 = stride_io == (out_stride ? out_stride : row);
            if (ok2) apply_reached[ak][as]++;
            else { failed++; if (failed < 5) std::fprintf(stderr, "apply case %ld: kind %d side %d status %d (%s)\n", it, ak, as, st2, dabgpu_last_error()); }
        }
        // frequency words: the inverse of the conversion is exact for every word whose low 11 bits are clear (a double's 53 bits)
        const uint64_t w = rng() & ~(uint64_t)0x7FF;
        const double cyc = dabgpu_channel_freq_cycles(w);
        if (!(cyc >= -0.5 && cyc < 0.5) || dabgpu_channel_freq_q64(cyc) != w) failed++; else round_trips++;
    }
    if (dabgpu_channel_freq_q64(std::nan("")) != 0 || dabgpu_channel_freq_q64(0.5000001) != 0 || dabgpu_channel_freq_q64(-0.5000001) != 0) failed++;
    std::printf("{\"iterations\": %ld, \"failed_checks\": %ld, \"accepted\": %ld, \"direct\": %ld, \"staged\": %ld, \"round_trips\": %ld",
                iters, failed, reached[OK][0] + reached[OK][1], staged[0], staged[1], round_trips);
    const char* names[N_KINDS] = {"", "n_streams", "taps", "delay", "gain", "sigma_not_finite", "sigma_negative", "tap_value", "start", "null_params"};
    for (int k = 1; k < N_KINDS; k++) std::printf(", \"%s_low\": %ld, \"%s_high\": %ld", names[k], reached[k][0], names[k], reached[k][1]);
    const char* anames[A_KINDS] = {"apply_ok", "apply_format", "apply_n_in", "apply_n_out", "apply_null", "apply_in_stride", "apply_out_stride", "apply_align",
                                   "apply_scale", "apply_grid"};
    for (int k = 0; k < A_KINDS; k++) std::printf(", \"%s_a\": %ld, \"%s_b\": %ld", anames[k], apply_reached[k][0], anames[k], apply_reached[k][1]);
    std::printf(", \"fits_no\": %ld, \"fits_yes_smaller\": %ld, \"fits_yes_equal\": %ld}\n", fits[0][0] + fits[0][1], fits[1][0], fits[1][1]);
    return failed ? 1 : 0;
}
