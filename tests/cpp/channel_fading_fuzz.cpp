// channel_fading_fuzz.cpp -- dabgpu_channel_fading_plan, dabgpu_channel_fading_gain_host and the fading-table check
// (dab-radio_amd/csrc/dabgpu_host_logic.cpp) under ASan + UBSan (tests/test_channel_fading_plan.py builds it): random parameter and spec
// lists with at most one defect each, allocated exactly so that a read or write past a list is caught; an acceptance is checked against the
// rules the header states, a refusal against the defect planted.
//   channel_fading_fuzz <iterations> <seed>  -> one JSON line with how often each side of every decision was reached
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
#include "channel_core.h"

int main(int argc, char** argv) {
    const long iters = argc > 1 ? std::atol(argv[1]) : 20000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
    enum { OK, NULL_PTR, DOPPLER, KIND, RICE, LOS, PARAMS, N_KINDS };
    long failed = 0, reached[N_KINDS][2] = {}, edges = 0, gains_ok = 0, check_ok[2] = {};
    const float bad_values[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
    const double top = DABGPU_FADING_MAX_DOPPLER_CYCLES;
    for (long it = 0; it < iters; it++) {
        const int kind = (int)(rng() % N_KINDS), side = (int)(rng() & 1);
        const size_t n = 1 + rng() % 4;
        std::vector<dabgpu_channel_stream> v(n);
        std::vector<dabgpu_channel_fading_spec> sp(n);
        std::vector<dabgpu_channel_fading_stream> out(n);
        std::memset(out.data(), 0x5A, n * sizeof(out[0]));
        bool any_fading = false;
        for (size_t s = 0; s < n; s++) {
            dabgpu_channel_stream& P = v[s];
            std::memset(&P, 0, sizeof(P));
            P.gain = 1.0f; P.seed = rng(); P.freq_q64 = rng();
            P.n_taps = 1 + (int)(rng() % 8);
            dabgpu_channel_fading_spec& S = sp[s];
            S.seed = rng();
            const int e = (int)(rng() % 6);
            S.doppler_cycles = e == 0 ? 0.0 : e == 1 ? top : top * (double)(rng() % 100001) / 100000.0;
            for (int k = 0; k < 8; k++) {                                        // (entries past n_taps may hold anything)
                const bool on = k < P.n_taps;
                P.tap_delay[k] = on ? (int)(rng() % 2048) : (int)rng();
                P.tap_re[k] = on ? 0.5f : bad_values[rng() % 3];
                P.tap_im[k] = on ? -0.25f : bad_values[rng() % 3];
                S.kind[k] = on ? (int)(rng() & 1) : (int)rng();
                const int r = (int)(rng() % 5);
                S.rice_k[k] = !on ? bad_values[rng() % 3] : r == 0 ? 0.0f : (float)(rng() % 2000) / 100.0f;
                S.los_cos[k] = !on ? bad_values[rng() % 3] : r == 1 ? 1.0f : r == 2 ? -1.0f : (float)(rng() % 2001) / 1000.0f - 1.0f;
                if (on && S.kind[k] == DABGPU_TAP_STATIC && (rng() & 1)) { S.rice_k[k] = bad_values[rng() % 3]; S.los_cos[k] = 7.0f; }   // not read
                if (on && S.kind[k] == DABGPU_TAP_FADING) any_fading = true;
            }
        }
        const size_t bs = rng() % n;
        dabgpu_channel_stream& B = v[bs];
        dabgpu_channel_fading_spec& SB = sp[bs];
        int k = (int)(rng() % (unsigned)B.n_taps);
        const dabgpu_channel_stream* a0 = v.data();
        const dabgpu_channel_fading_spec* a1 = sp.data();
        dabgpu_channel_fading_stream* a2 = out.data();
        switch (kind) {
        case NULL_PTR: { const int w = (int)(rng() % 3); if (w == 0) a0 = nullptr; else if (w == 1) a1 = nullptr; else a2 = nullptr; break; }
        case DOPPLER: SB.doppler_cycles = side ? std::nextafter(top, 1.0) * (1.0 + (double)(rng() % 3)) : -std::ldexp(1.0, -(int)(rng() % 1070)); if (rng() % 9 == 0) SB.doppler_cycles = std::nan(""); break;
        case KIND: SB.kind[k] = side ? 2 + (int)(rng() % 1000) : -1 - (int)(rng() % 1000); break;
        case RICE: SB.kind[k] = DABGPU_TAP_FADING; SB.rice_k[k] = side ? bad_values[rng() % 3] : -std::ldexp(1.0f, -(int)(rng() % 140)); break;
        case LOS: SB.kind[k] = DABGPU_TAP_FADING; SB.los_cos[k] = side ? std::nextafter(1.0f, 2.0f) + (float)(rng() % 3) : std::nextafter(-1.0f, -2.0f) - (float)(rng() % 3); if (rng() % 5 == 0) SB.los_cos[k] = bad_values[rng() % 3]; break;
        case PARAMS: if (side) B.n_taps = 9 + (int)(rng() % 9); else B.tap_delay[k] = 2048 + (int)(rng() % 99); break;
        default: break;
        }
        const int st = dabgpu_channel_fading_plan(a0, a1, n, a2);
        bool ok = (kind == OK) ? st == DABGPU_OK : st == DABGPU_ERR_INVALID_ARG;
        if (ok && kind != OK && a2) {                                            // a refusal writes nothing
            const unsigned char* p = reinterpret_cast<const unsigned char*>(out.data());
            for (size_t i = 0; i < n * sizeof(out[0]) && ok; i++) ok = p[i] == 0x5A;
        }
        if (ok && kind == OK) {
            for (size_t s = 0; s < n && ok; s++) {
                const double fmax = std::ldexp(sp[s].doppler_cycles, 64) + 1.0;
                for (int t = 0; t < 8 && ok; t++) {
                    const bool fades = t < v[s].n_taps && sp[s].kind[t] == DABGPU_TAP_FADING;
                    const dabgpu_channel_fading_tap& T = out[s].tap[t];
                    ok = out[s].kind[t] == (fades ? DABGPU_TAP_FADING : DABGPU_TAP_STATIC);
                    if (!fades) {
                        for (int o = 0; o < DABGPU_FADING_OSC && ok; o++) ok = T.freq_q64[o] == 0 && T.phase_q64[o] == 0;
                        ok = ok && T.amp_diffuse == 0.0f && T.amp_los == 0.0f;
                        continue;
                    }
                    for (int o = 0; o < DABGPU_FADING_OSC && ok; o++) {
                        uint32_t w[4];
                        dabgpu::ch_philox4x32_10((uint32_t)sp[s].seed, (uint32_t)(sp[s].seed >> 32), (uint32_t)o, (uint32_t)t, (uint32_t)s, 1u, w);
                        ok = T.phase_q64[o] == (((uint64_t)w[2] << 32) | w[3]) && std::fabs((double)(int64_t)T.freq_q64[o]) <= fmax;
                    }
                    const double unit = 16.0 * (double)T.amp_diffuse * (double)T.amp_diffuse + (double)T.amp_los * (double)T.amp_los;
                    ok = ok && std::fabs(unit - 1.0) <= 4.0 * 0x1p-24 && (sp[s].rice_k[t] != 0.0f || T.amp_los == 0.0f);
                    if (sp[s].doppler_cycles == 0.0 || sp[s].doppler_cycles == top) edges++;
                }
            }
            // the tables the planner made pass the bank's check and give finite gains of at most 16 amp_diffuse + amp_los; a planted kind fails it
            if (ok) {
                ok = dabgpu_host_channel_fading_check("fuzz", v.data(), out.data(), n) == DABGPU_OK;
                const int t = (int)(rng() % 8);
                const uint64_t m0 = (rng() & 1) ? rng() >> 2 : rng() % 5000;
                const size_t count = rng() % 200;
                std::vector<float> g(2 * count);
                ok = ok && dabgpu_channel_fading_gain_host(&out[bs], t, m0, count, g.data()) == DABGPU_OK;
                const float A = 16.0f * out[bs].tap[t].amp_diffuse + out[bs].tap[t].amp_los;
                for (size_t i = 0; i < count && ok; i++)
                    ok = out[bs].kind[t] == DABGPU_TAP_FADING ? (std::fabs(g[2 * i]) <= 1.0001f * A && std::fabs(g[2 * i + 1]) <= 1.0001f * A)
                                                              : (g[2 * i] == 1.0f && g[2 * i + 1] == 0.0f);
                if (ok) gains_ok++;
                ok = ok && dabgpu_channel_fading_gain_host(&out[bs], (rng() & 1) ? 8 + (int)(rng() % 9) : -1 - (int)(rng() % 9), m0, count, g.data()) == DABGPU_ERR_INVALID_ARG;
                ok = ok && dabgpu_channel_fading_gain_host(nullptr, 0, m0, count, g.data()) == DABGPU_ERR_INVALID_ARG;
                if (ok) check_ok[0]++;
                const int which = (int)(rng() & 1);
                if (which) out[bs].kind[k] = 2 + (int)(rng() % 5);
                else { out[bs].kind[k] = DABGPU_TAP_FADING; out[bs].tap[k].amp_los = bad_values[rng() % 3]; }
                if (dabgpu_host_channel_fading_check("fuzz", v.data(), out.data(), n) == DABGPU_ERR_INVALID_ARG) check_ok[1]++; else ok = false;
            }
        }
        (void)any_fading;
        if (ok) reached[kind][side]++;
        else { failed++; if (failed < 5) std::fprintf(stderr, "case %ld: kind %d side %d status %d (%s)\n", it, kind, side, st, dabgpu_last_error()); }
    }
    std::printf("{\"iterations\": %ld, \"failed_checks\": %ld, \"accepted\": %ld, \"edge_dopplers\": %ld, \"gains\": %ld, \"tables_pass\": %ld, \"tables_fail\": %ld",
                iters, failed, reached[OK][0] + reached[OK][1], edges, gains_ok, check_ok[0], check_ok[1]);
    const char* names[N_KINDS] = {"", "null", "doppler", "kind", "rice", "los", "params"};
    for (int k = 1; k < N_KINDS; k++) std::printf(", \"%s_low\": %ld, \"%s_high\": %ld", names[k], reached[k][0], names[k], reached[k][1]);
    std::printf("}\n");
    return failed ? 1 : 0;
}
