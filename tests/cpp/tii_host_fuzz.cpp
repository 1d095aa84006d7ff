// tii_host_fuzz.cpp -- the TII host logic (dabgpu_host_logic.cpp) under random arguments, built with -fsanitize=address,undefined by
// tests/test_tii_host.py: dabgpu_tii_carriers into an exactly sized heap buffer, dabgpu_tii_validate over exactly sized heap lists, each
// answer checked against the rule restated here.  Prints the count of every decision reached, as one JSON line.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "dabgpu.h"

int main(int argc, char** argv) {
    const long iters = argc > 1 ? atol(argv[1]) : 10000;
    std::mt19937_64 rng(argc > 2 ? (unsigned long long)atoll(argv[2]) : 1);
    std::map<std::string, long> n;
    long failed = 0;
    auto pick = [&](int lo, int hi) { return (int)(lo + (long long)(rng() % (unsigned long long)(hi - lo + 1))); };
    for (long it = 0; it < iters; it++) {
        // carriers: ids around both edges, and anywhere
        const int p = (rng() & 1) ? pick(-3, 73) : pick(-1000000, 1000000), c = (rng() & 1) ? pick(-3, 27) : pick(-1000000, 1000000);
        int* out = new int[32];
        const int st = dabgpu_tii_carriers(p, c, out);
        const bool ok = p >= 0 && p < 70 && c >= 0 && c < 24;
        if ((st == DABGPU_OK) != ok) failed++;
        if (ok) {
            n["carriers_ok"]++;
            const int pat = dabgpu_tii_pattern(p);
            if (__builtin_popcount((unsigned)pat) != 4 || dabgpu_tii_main_id((uint32_t)pat) != p) failed++;
            for (int q = 0; q < 32; q += 2) {
                const int k = out[q];
                if (out[q + 1] != k + 1 || k < -768 || k + 1 > 768 || k == 0 || k + 1 == 0) failed++;
                const int rel = k < -384 ? k + 768 : k < 0 ? k + 384 : k < 385 ? k - 1 : k - 385;      // 2 c + 48 b
                if (rel % 48 != 2 * c || !((pat >> (7 - rel / 48)) & 1)) failed++;
            }
        } else {
            n[p < 0 ? "carriers_main_low" : p >= 70 ? "carriers_main_high" : c < 0 ? "carriers_sub_low" : "carriers_sub_high"]++;
        }
        delete[] out;
        // masks
        const uint32_t mask = (rng() & 3) ? (uint32_t)(rng() & 0xFF) : (uint32_t)rng();
        const int id = dabgpu_tii_main_id(mask);
        if (mask <= 0xFF && __builtin_popcount(mask) == 4) { n["mask_pattern"]++; if (id < 0 || dabgpu_tii_pattern(id) != (int)mask) failed++; }
        else { n["mask_other"]++; if (id != -1) failed++; }
        // lists: mostly valid entries, one rule broken now and then
        const size_t frames = (size_t)pick(1, 6);
        std::vector<dabgpu_tii_tx>* lists = new std::vector<dabgpu_tii_tx>(frames * DABGPU_TII_MAX_TX);
        std::vector<uint8_t>* counts = new std::vector<uint8_t>(frames);
        std::string want;
        for (size_t f = 0; f < frames; f++) {
            int cnt = pick(0, 4);
            if (pick(0, 15) == 0) cnt = pick(5, 255);
            (*counts)[f] = (uint8_t)cnt;
            if (cnt > 4 && want.empty()) want = "lists_count";
            for (int i = 0; i < 4; i++) {
                dabgpu_tii_tx& t = (*lists)[f * 4 + i];
                t.main_id = (uint8_t)(pick(0, 19) ? pick(0, 69) : pick(70, 255));
                t.sub_id = (uint8_t)(pick(0, 19) ? pick(0, 23) : pick(24, 255));
                const int a = pick(0, 24);
                t.amp = a == 0 ? NAN : a == 1 ? INFINITY : a == 2 ? -INFINITY : (float)pick(-1000, 1000) * 0.01f;
                if (i < cnt && cnt <= 4 && want.empty()) {
                    if (t.main_id >= 70) want = "lists_main";
                    else if (t.sub_id >= 24) want = "lists_sub";
                    else if (!std::isfinite(t.amp)) want = "lists_amp";
                }
            }
            if (cnt > 4 && want == "lists_count") break;        // (later frames are not looked at; leave them zero)
        }
        const int sl = dabgpu_tii_validate(lists->data(), counts->data(), frames);
        if (want.empty()) { n["lists_ok"]++; if (sl != DABGPU_OK) failed++; }
        else {
            n[want]++;
            const char* word = want == "lists_count" ? "transmitters (at most" : want == "lists_main" ? "main id" : want == "lists_sub" ? "sub id" : "amp";
            if (sl != DABGPU_ERR_INVALID_ARG || !strstr(dabgpu_last_error(), word)) failed++;
        }
        delete lists;
        delete counts;
    }
    printf("{\"iterations\": %ld, \"failed_checks\": %ld", iters, failed);
    for (auto& kv : n) printf(", \"%s\": %ld", kv.first.c_str(), kv.second);
    printf("}\n");
    return failed ? 1 : 0;
}
