// tests/test_addressing_rules.py: what the decode planner and the generic batch's rule answer around the largest frame-history ring
// whose offsets the lane and octet gathers can hold in 32 bits.  Plain C++ over dabgpu_host_logic.cpp, no device.
// usage: addressing_rules_driver H...   -> one JSON line per H
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dabgpu.h"
#include "dabgpu_host_logic.h"

int main(int argc, char** argv) {
    const dabgpu_subchannel subs[3] = {{3, 6, 0, 0, 2, 0}, {100, 35, 1, 4, 0, 0}, {800, 64, 0, 0, 3, 0}};
    for (int a = 1; a < argc; a++) {
        unsigned long long g[4];
        if (sscanf(argv[a], "%llu:%llu:%llu:%llu", &g[0], &g[1], &g[2], &g[3]) == 4) {      // n_slots:cifs_per_frame:frame_stride:cif_stride
            printf("{\"geometry\": [%llu, %llu, %llu, %llu], \"batch_lanes\": %s}\n", g[0], g[1], g[2], g[3],
                   dabgpu_host_ring_fits_lanes(g[0], g[1], g[2], g[3]) ? "true" : "false");
            continue;
        }
        const int H = atoi(argv[a]);
        printf("{\"H\": %d, \"plans\": [", H);
        bool first = true;
        for (size_t n_ens : {(size_t)1, (size_t)4096}) {
            for (int forced = DABGPU_VIT_MAP_AUTO; forced <= DABGPU_VIT_MAP_OCTET; forced++) {
                dabgpu_decode_limits lim = {};
                lim.n_simd = 1024; lim.max_dec_rows = (size_t)1 << 20; lim.hybrid_k = -1; lim.forced_mapping = forced;
                dabgpu_decode_plan p;
                const int st = dabgpu_host_plan_decode(subs, 3, n_ens, H, true, lim, &p);
                printf("%s{\"n_ens\": %zu, \"forced\": %d, \"status\": %d, \"mapping\": %d, \"k_wave\": %d, \"n_lane\": %d}", first ? "" : ", ", n_ens, forced,
                       st, p.mapping, p.k_wave, p.n_lane);
                first = false;
            }
        }
        // the generic batch's rule on the ring-form code words of that ring
        printf("], \"batch_lanes\": %s}\n", dabgpu_host_ring_fits_lanes((uint64_t)H * 4, 4, DABGPU_NB_FRAME_BITS, DABGPU_NB_CIF_BITS) ? "true" : "false");
    }
    return 0;
}
