// Fuzzer of the channel encoder's planner (dabgpu_host_tx_plan / dabgpu_tx_encode_plan, dab-radio_amd/csrc/dabgpu_host_logic.cpp), built
// with ASan + UBSan by tests/test_tx_encode_plan.py: random and hostile sub-channel lists.  Every accepted plan is checked for what the
// kernel relies on: code words inside their capacity units, schedules inside the table and monotonic, input records back to back,
// disjoint ring rows, gaps + sub-channels = 864 CU.  Usage: tx_plan_fuzz ITERATIONS SEED; prints one JSON line.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "dabgpu_host_logic.h"

static long failed = 0;
#define CHECK(c) do { if (!(c)) { failed++; fprintf(stderr, "check failed line %d: %s\n", __LINE__, #c); } } while (0)

int main(int argc, char** argv) {
    const long iters = argc > 1 ? atol(argv[1]) : 1000;
    std::mt19937_64 rng(argc > 2 ? (uint64_t)atoll(argv[2]) : 1);
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    static const int HOSTILE[] = {0, -1, 1, 863, 864, 865, 2147483647, -2147483647 - 1, 64, 63, 4, -4, 1 << 30};
    long accepted = 0;
    for (long it = 0; it < iters; it++) {
        const int mode = pick(0, 3);                       // 0: tidy multiplex, 1: random fields, 2: hostile fields, 3: tidy with one field spoilt
        int n = (mode == 0 || mode == 3) ? pick(0, 20) : pick(-2, 70);
        std::vector<dabgpu_subchannel> subs((size_t)(n > 0 ? n : 0));
        int at = 0;
        for (auto& s : subs) {
            if (mode == 0 || mode == 3) {
                s.is_uep = pick(0, 3) == 0;
                s.uep_prot_index = pick(0, 63); s.eep_prot_level = pick(0, 3); s.eep_type = pick(0, 1);
                static const int unit[2][4] = {{12, 8, 6, 4}, {27, 21, 18, 15}};
                s.length = s.is_uep ? pick(16, 120) : unit[s.eep_type][s.eep_prot_level] * pick(1, 6);
                at += pick(0, 3);
                s.start_address = at; at += s.length;
            } else if (mode == 1) {
                s = {pick(-5, 900), pick(-5, 900), pick(-1, 2), pick(-3, 70), pick(-2, 6), pick(-1, 3)};
            } else {
                int* f = &s.start_address;
                for (int k = 0; k < 6; k++) f[k] = HOSTILE[rng() % (sizeof(HOSTILE) / sizeof(HOSTILE[0]))];
            }
        }
        if (mode == 3 && !subs.empty()) (&subs[rng() % subs.size()].start_address)[rng() % 6] = HOSTILE[rng() % (sizeof(HOSTILE) / sizeof(HOSTILE[0]))];
        dabgpu_tx_plan P;
        const int st = dabgpu_host_tx_plan(n > 0 ? subs.data() : nullptr, n, &P);
        CHECK(st == DABGPU_OK || st == DABGPU_ERR_INVALID_ARG);
        // the C entry point agrees and never writes more than it was given room for
        std::vector<dabgpu_tx_sub_plan> plans((size_t)(n > 0 ? n : 0) + 1);
        std::vector<dabgpu_tx_sched_entry> sched(P.sched.size());
        size_t ns = 0; uint32_t cif_in = 0, ring = 0;
        CHECK(dabgpu_tx_encode_plan(n > 0 ? subs.data() : nullptr, n, plans.data(), &cif_in, sched.data(), sched.size(), &ns, &ring) == st);
        if (st != DABGPU_OK) { CHECK(dabgpu_last_error()[0] != 0); continue; }
        accepted++;
        CHECK(n >= 0 && n <= 64 && P.subs.size() == (size_t)n + 1 && ns == P.sched.size() && cif_in == P.cif_in_bytes && ring == P.ring_slot_dwords);
        unsigned char used[864] = {0};
        uint32_t in_at = 0, ring_at = 0;
        for (int s = 0; s <= n; s++) {
            const dabgpu_tx_sub_plan& D = P.subs[(size_t)s];
            CHECK(memcmp(&D, &plans[(size_t)s], sizeof(D)) == 0);
            CHECK(D.kept_bits <= D.length * 64u && D.n_words > 0);
            CHECK((size_t)D.sched_offset + D.n_words + 1 <= P.sched.size());
            uint32_t bit = 0, words = 0;
            for (int k = 0; k < 4; k++) words += D.seg_blocks[k];
            CHECK(words == D.n_words);
            for (uint32_t w = 0; w <= D.n_words; w++) {
                const dabgpu_tx_sched_entry& e = P.sched[D.sched_offset + w];
                CHECK(e.out_bit == bit);
                bit += (w < D.n_words ? 4u : 1u) * (uint32_t)__builtin_popcount(e.keep_mask);
            }
            CHECK(bit == D.kept_bits);
            if (s == n) { CHECK(D.kept_bits == 2304 && D.in_bytes == 96 && D.n_words == 24); break; }
            CHECK(D.in_offset == in_at && D.in_bytes == 4 * D.n_words); in_at += D.in_bytes;
            CHECK(D.ring_offset == ring_at && D.ring_row_dwords * 8 >= D.length); ring_at += 16 * D.ring_row_dwords;
            CHECK(D.start_address + D.length <= 864 && D.length <= P.max_length);
            for (uint32_t cu = D.start_address; cu < D.start_address + D.length && cu < 864; cu++) { CHECK(!used[cu]); used[cu] = 1; }
        }
        CHECK(in_at == P.cif_in_bytes && ring_at == P.ring_slot_dwords && P.gaps.size() % 2 == 0);
        uint32_t prev_end = 0;
        for (size_t g = 0; g + 1 < P.gaps.size(); g += 2) {
            CHECK(P.gaps[g] >= prev_end && P.gaps[g + 1] > 0 && P.gaps[g] + P.gaps[g + 1] <= 864);
            for (uint32_t cu = P.gaps[g]; cu < P.gaps[g] + P.gaps[g + 1] && cu < 864; cu++) { CHECK(!used[cu]); used[cu] = 1; }
            prev_end = P.gaps[g] + P.gaps[g + 1];
        }
        for (int cu = 0; cu < 864; cu++) CHECK(used[cu]);
    }
    printf("{\"iterations\": %ld, \"accepted\": %ld, \"failed_checks\": %ld}\n", iters, accepted, failed);
    return failed ? 1 : 0;
}
