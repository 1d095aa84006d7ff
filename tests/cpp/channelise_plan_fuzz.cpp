// channelise_plan_fuzz.cpp -- dabgpu_channeliser_plan, _design, _freq_q64, _input_needed and _decim_for (dab-radio_amd/csrc/
// dabgpu_host_logic.cpp) under ASan + UBSan (tests/test_channelise_plan.py builds it): random channel lists with at most one defect each,
// allocated exactly so that a read past the list is caught; an acceptance is checked against the geometry the header states, a refusal
// against the defect planted; the input span against every output's taps; designs against the properties the header states.
//   channelise_plan_fuzz <iterations> <seed>  -> one JSON line with how often each side of every decision was reached
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
#include "channelise_core.h"

int main(int argc, char** argv) {
    const long iters = argc > 1 ? std::atol(argv[1]) : 100000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
    enum { OK, N_STREAMS, N_CHANNELS, STREAM_RANGE, UNSORTED, NINE, GAIN, START, DECIM, NULL_LIST, NULL_DESIGN, N_KINDS };
    long failed = 0, reached[N_KINDS][2] = {}, spans = 0, designs = 0, design_refusals = 0, freqs = 0, firsts = 0;
    const float bad_values[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
    const double nan = std::nan("");
    dabgpu_channeliser_filter* design = new dabgpu_channeliser_filter;       // (only decim is read by the planner)
    std::memset(design, 0, sizeof(*design));
    for (long it = 0; it < iters; it++) {
        const int kind = (int)(rng() % N_KINDS), side = (int)(rng() & 1);
        const int D = 1 + (int)(rng() % 8);
        design->decim = D;
        const size_t n_streams = 1 + rng() % 5;
        std::vector<dabgpu_channeliser_channel> v;
        for (size_t s = 0; s < n_streams; s++) {
            const size_t k = (rng() % 4 == 0) ? 8 : rng() % 9;              // (streams without a channel are accepted)
            for (size_t i = 0; i < k; i++) {
                dabgpu_channeliser_channel C;
                C.freq_q64 = rng(); C.phase0_q64 = (rng() % 3 == 0) ? 0 : rng();
                if (rng() % 5 == 0) C.freq_q64 = C.phase0_q64 = 0;
                C.gain = (float)(rng() % 2000) / 100.0f - 10.0f;
                C.stream = (uint32_t)s;
                v.push_back(C);
            }
        }
        if (v.empty()) { dabgpu_channeliser_channel C = {0, 0, 1.0f, (uint32_t)(n_streams - 1)}; v.push_back(C); }
        int64_t start = (int64_t)(rng() >> 3) - ((int64_t)1 << 60);
        if (rng() % 7 == 0) start = (rng() & 1) ? DABGPU_CHANNELISER_MAX_START : -DABGPU_CHANNELISER_MAX_START;
        size_t n_arg = v.size(), s_arg = n_streams;
        const dabgpu_channeliser_filter* d_arg = design;
        bool null_list = false;
        int k2 = kind;
        const size_t b = rng() % v.size();
        switch (kind) {
        case N_STREAMS: s_arg = side ? ((size_t)1 << 20) + 1 + rng() % 5 : 0; break;
        case N_CHANNELS: if (side) { s_arg = 1; n_arg = 9 + rng() % 5; v.resize(n_arg, v[0]); for (auto& C : v) C.stream = 0; } else n_arg = 0; break;
        case STREAM_RANGE: v[b].stream = (uint32_t)n_streams + (side ? (uint32_t)(rng() % 1000) : 0u); break;
        case UNSORTED:                                                       // a channel of an earlier stream behind one of a later stream
            if (b > 0 && v[b - 1].stream > 0) v[b].stream = v[b - 1].stream - 1 - (side ? (uint32_t)(rng() % v[b - 1].stream) : 0u);
            else k2 = OK;
            break;
        case NINE:                                                           // 9 .. 11 channels on the first or the last of at least two streams
            s_arg = std::max(n_streams, (size_t)2);
            v.assign(9 + rng() % 3, v[0]);
            for (auto& C : v) C.stream = (uint32_t)(side ? s_arg - 1 : 0);
            n_arg = v.size();
            break;
        case GAIN: v[b].gain = bad_values[rng() % 3]; break;
        case START: start = side ? DABGPU_CHANNELISER_MAX_START + 1 + (int64_t)(rng() % 1000) : -DABGPU_CHANNELISER_MAX_START - 1 - (int64_t)(rng() % 1000); break;
        case DECIM: design->decim = side ? 9 + (int)(rng() % 100) : 0 - (int)(rng() % 100); break;
        case NULL_LIST: null_list = true; break;
        case NULL_DESIGN: d_arg = nullptr; break;
        default: break;
        }
        // an exact copy: a read past the list is a heap overflow
        std::vector<dabgpu_channeliser_channel> list(v.begin(), v.begin() + (long)std::min(n_arg, v.size()));
        dabgpu_channeliser_geometry g;
        std::memset(&g, 0x5A, sizeof(g));
        const bool want_g = rng() % 9 != 0;
        const int st = dabgpu_channeliser_plan(null_list ? nullptr : list.data(), n_arg, s_arg, start, d_arg, want_g ? &g : nullptr);
        bool ok = (k2 == OK) ? st == DABGPU_OK : st == DABGPU_ERR_INVALID_ARG;
        if (ok && k2 == OK && want_g) {
            const uint32_t d = (uint32_t)D, nt = d == 1 ? 1u : 72u;
            ok = g.decim == d && g.taps == nt * d && g.split_tile == 512 && g.combine_tile == 128 * d && g.combine_window == 128 + nt - 1 &&
                 g.combine_lds_bytes == ((128 + nt) & ~1u) * 8 && g.split_window == (d == 1 ? 0u : 584u * d) &&
                 g.split_lds_bytes == (d == 1 ? 0u : 2u * 4u * d * 147u * 8u) && g.split_lds_bytes <= 160u * 1024u;
        }
        if (ok && k2 == OK) {
            // the per-stream ranges of the internal planner: every channel of stream s, and only those
            std::vector<uint32_t> first(s_arg + 1, 0xFFFFFFFFu);
            if (dabgpu_host_channeliser_plan("fuzz", list.data(), n_arg, s_arg, start, D, nullptr, first.data()) != DABGPU_OK) ok = false;
            for (size_t s = 0; ok && s < s_arg; s++) {
                if (first[s] > first[s + 1] || first[s + 1] > n_arg || first[s + 1] - first[s] > 8) ok = false;
                for (uint32_t c = first[s]; ok && c < first[s + 1]; c++) if (list[c].stream != s) ok = false;
            }
            if (ok && (first[0] != 0 || first[s_arg] != n_arg)) ok = false;
            if (ok) firsts++;
        }
        if (ok) reached[k2][side]++;
        else { failed++; if (failed < 5) std::fprintf(stderr, "case %ld: kind %d status %d (%s)\n", it, kind, st, dabgpu_last_error()); }
        design->decim = D;

        // the input span of a split against its outputs' first and last taps
        {
            const uint64_t pos = (rng() % 5 == 0) ? (uint64_t)DABGPU_CHANNELISER_MAX_POSITION - rng() % 5000 : rng() >> (6 + rng() % 56);
            const size_t n_out = (rng() % 6 == 0) ? 0 : 1 + rng() % 5000;
            const int64_t st0 = (kind == START) ? 0 : start;
            int64_t first = 7; uint64_t count = 7;
            const int st3 = dabgpu_channeliser_input_needed(D, pos, st0, n_out, &first, &count);
            const int K = D == 1 ? 1 : 72 * D, P = D == 1 ? 0 : K / 2 - 1;
            const __int128 a = (__int128)pos * D + st0 - P, z = (__int128)(pos + (n_out ? n_out - 1 : 0)) * D + st0 - P + K - 1;
            if (st3 != DABGPU_OK || (n_out ? ((__int128)first != a || (__int128)count != z - a + 1) : count != 0)) failed++; else spans++;
            if (n_out && dabgpu::cs_split_first(D, pos + n_out - 1, st0) + K - 1 != (int64_t)z) failed++;
            if (dabgpu_channeliser_input_needed(side ? 9 : 0, pos, st0, n_out, &first, &count) != DABGPU_ERR_INVALID_ARG) failed++;
            if (dabgpu_channeliser_input_needed(D, (uint64_t)DABGPU_CHANNELISER_MAX_POSITION + 1 + rng() % 9, st0, n_out, &first, &count) != DABGPU_ERR_INVALID_ARG) failed++;
            if (dabgpu_channeliser_input_needed(D, pos, st0, n_out, side ? nullptr : &first, side ? &count : nullptr) != DABGPU_ERR_INVALID_ARG) failed++;
        }
        // frequency words: the offset over the rate, to the nearest word; outside +- half the rate 0
        {
            const double rate = 2048000.0 * (1 + rng() % 8), off = ((double)(rng() % 2000001) / 1000000.0 - 1.0) * 0.75 * rate;
            const uint64_t w = dabgpu_channeliser_freq_q64(off, rate);
            const double cyc = off / rate;
            if (std::fabs(cyc) > 0.5) { if (w != 0) failed++; }
            else if (std::fabs(std::ldexp((double)(int64_t)w, -64) - cyc) > std::ldexp(1.0, -52) && std::fabs(cyc) < 0.5) failed++;
            else freqs++;
        }
        // designs (every 64th iteration: a design costs a few million operations)
        if (it % 64 == 0) {
            dabgpu_channeliser_filter* F = new dabgpu_channeliser_filter;
            const double pb = 0.05 + (double)(rng() % 400) / 1000.0, sb = pb + 0.02 + (double)(rng() % 300) / 1000.0;
            const int dd = 1 + (int)(rng() % 8);
            const int bad = (int)(rng() % 8);
            int st4;
            switch (bad) {
            case 0: st4 = dabgpu_channeliser_design(side ? 9 : 0, pb, sb, F); break;
            case 1: st4 = dabgpu_channeliser_design(dd, side ? nan : pb, side ? sb : nan, F); break;
            case 2: st4 = dabgpu_channeliser_design(dd, sb, side ? pb : sb, F); break;                    // no transition
            case 3: st4 = dabgpu_channeliser_design(dd, pb, 0.5 * dd + 0.001 + (side ? 1.0 : 0.0), F); break;
            case 4: st4 = dabgpu_channeliser_design(dd, side ? -pb : pb, side ? sb : -sb, F); break;
            case 5: st4 = dabgpu_channeliser_design(dd, pb, sb, nullptr); break;
            default: st4 = dabgpu_channeliser_design(dd, pb, std::min(sb, 0.5 * dd), F); break;
            }
            if (bad <= 5) { if (st4 != DABGPU_ERR_INVALID_ARG) failed++; else design_refusals++; }
            else if (st4 != DABGPU_OK) { if (!(pb < std::min(sb, 0.5 * dd))) design_refusals++; else failed++; }
            else {
                double sum = 0.0;
                int arg = 0;
                for (int j = 0; j < F->taps; j++) { sum += F->table[j]; if (F->table[j] > F->table[arg]) arg = j; }
                bool good = F->decim == dd && F->taps == (dd == 1 ? 1 : 72 * dd) && std::fabs(sum - 1.0) < 1e-4 && arg == (dd == 1 ? 0 : F->taps / 2 - 1) &&
                            F->error == F->passband_error + F->stopband_level && F->passband_error >= 0.0 && F->stopband_level >= 0.0 && std::isfinite(F->error);
                for (int j = F->taps; j < 72 * 8; j++) if (F->table[j] != 0.0f) good = false;
                if (!good) failed++; else designs++;
            }
            delete F;
        }
    }
    const int rates_ok = dabgpu_channeliser_decim_for(8192000.0) == 4 && dabgpu_channeliser_decim_for(10240000.0) == 5 && dabgpu_channeliser_decim_for(10000000.0) == 4 &&
                         dabgpu_channeliser_decim_for(16384000.0) == 8 && dabgpu_channeliser_decim_for(1e9) == 8 && dabgpu_channeliser_decim_for(2048000.0) == 1 &&
                         dabgpu_channeliser_decim_for(2047999.0) == 0 && dabgpu_channeliser_decim_for(nan) == 0 && dabgpu_channeliser_decim_for(4095999.0) == 1;
    if (!rates_ok) failed++;
    if (dabgpu_channeliser_freq_q64(nan, 1.0) != 0 || dabgpu_channeliser_freq_q64(1.0, nan) != 0 || dabgpu_channeliser_freq_q64(1.0, 0.0) != 0 ||
        dabgpu_channeliser_freq_q64(1.0, -4.0) != 0 || dabgpu_channeliser_freq_q64(0.5, 1.0) != ((uint64_t)1 << 63) ||
        dabgpu_channeliser_freq_q64(-0.5, 1.0) != ((uint64_t)1 << 63) || dabgpu_channeliser_freq_q64(0.5000001, 1.0) != 0) failed++;
    delete design;
    std::printf("{\"iterations\": %ld, \"failed_checks\": %ld, \"accepted\": %ld, \"spans\": %ld, \"designs\": %ld, \"design_refusals\": %ld, \"freqs\": %ld, \"firsts\": %ld",
                iters, failed, reached[OK][0] + reached[OK][1], spans, designs, design_refusals, freqs, firsts);
    const char* names[N_KINDS] = {"", "n_streams", "n_channels", "stream_range", "unsorted", "nine", "gain", "start", "decim", "null_list", "null_design"};
    for (int k = 1; k < N_KINDS; k++) std::printf(", \"%s_low\": %ld, \"%s_high\": %ld", names[k], reached[k][0], names[k], reached[k][1]);
    std::printf("}\n");
    return failed ? 1 : 0;
}
