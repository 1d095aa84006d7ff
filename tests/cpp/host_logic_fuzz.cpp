// host_logic_fuzz.cpp -- the device-free part of libdabgpu.so (dab-radio_amd/csrc/dabgpu_host_logic.cpp) under
// -fsanitize=address,undefined with fuzzed arguments: sub-channel descriptors (start + length beyond 864 CU, length 0 / negative,
// UEP index outside 0..63, more than 64 sub-channels), wav images with lying chunk sizes and truncations, codeword descriptors, the
// mapping cost model at degenerate sizes, table generators at invalid modes, the decode planner (random and hostile multiplexes, batch sizes up
// to SIZE_MAX / 4, every forced mapping and scratch bound; a table of hand-worked plans).  Every call must come back with a status (never crash,
// never read or write outside its arguments -- the sanitizers abort the process otherwise), and what it accepts must be consistent.
//
//   host_logic_fuzz [iterations] [seed]          built and run by tests/test_host_sanitizers.py
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "dabgpu_host_logic.h"

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); g_fail++; } } while (0)

static void put32(std::vector<uint8_t>& v, uint32_t x) { for (int i = 0; i < 4; i++) v.push_back((uint8_t)(x >> (8 * i))); }
static void put16(std::vector<uint8_t>& v, uint16_t x) { v.push_back((uint8_t)x); v.push_back((uint8_t)(x >> 8)); }
static void tag(std::vector<uint8_t>& v, const char* t) { for (int i = 0; i < 4; i++) v.push_back((uint8_t)t[i]); }

// a well-formed wav image the mutations start from (app_wav_reader.h:107-255)
static std::vector<uint8_t> wav_image(std::mt19937& rng) {
    static const uint16_t codes[5] = {1, 3, 6, 7, 0xFFFE};
    const uint16_t code = codes[rng() % 5];
    const uint16_t bits = (uint16_t)((code == 1) ? (uint16_t[]){8, 16, 24, 32}[rng() % 4] : (code == 3) ? (uint16_t[]){32, 64}[rng() % 2] : (code == 0xFFFE ? 16 : 8));
    const uint32_t fmt_size = code == 0xFFFE ? 40 : (rng() % 3 == 0 ? 18 : 16);
    std::vector<uint8_t> v;
    tag(v, "RIFF"); put32(v, 0); tag(v, "WAVE");
    tag(v, "fmt "); put32(v, fmt_size);
    put16(v, code); put16(v, (uint16_t)(1 + rng() % 2)); put32(v, 2048000); put32(v, 2048000u * 2 * bits / 8); put16(v, (uint16_t)(2 * bits / 8)); put16(v, bits);
    if (fmt_size == 18) put16(v, 0);
    if (fmt_size == 40) {
        put16(v, 22); put16(v, bits); put32(v, 3); put16(v, 1);
        static const uint8_t GUID[14] = {0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71};
        v.insert(v.end(), GUID, GUID + 14);
    }
    if (code != 1 && code != 0xFFFE) { tag(v, "fact"); put32(v, 4); put32(v, 1000); }
    for (unsigned k = rng() % 3; k > 0; k--) { tag(v, "LIST"); const uint32_t n = rng() % 40; put32(v, n); v.insert(v.end(), n, (uint8_t)0x55); }
    tag(v, "data"); put32(v, 4000);
    v.insert(v.end(), 64, (uint8_t)0x80);
    return v;
}

// ---- decode planner (dabgpu_host_plan_decode / dabgpu_host_decode_slice / dabgpu_host_plan_uniform) ----
typedef unsigned __int128 u128;
static dabgpu_subchannel eep(int start, int length, int level, int type) { dabgpu_subchannel s{}; s.start_address = start; s.length = length; s.eep_prot_level = level; s.eep_type = type; return s; }
static dabgpu_subchannel uep(int start, int length, int index) { dabgpu_subchannel s{}; s.start_address = start; s.length = length; s.is_uep = 1; s.uep_prot_index = index; return s; }
static const size_t ROWS_6GIB = (size_t)6144 * 1024 * 1024 / 768, ROWS_2MIB = (size_t)2 * 1024 * 1024 / 768;      // 8388608, 2730

// what must hold of ANY plan the planner accepts; every size is recomputed here in 128 bits
static void check_plan(const dabgpu_decode_plan& p, const std::vector<dabgpu_subchannel>& subs, size_t n_ens, int hist_frames, bool want_fic,
                       const dabgpu_decode_limits& lim, std::mt19937& rng) {
    const int n_sub = (int)subs.size();
    CHECK(p.n_sub == n_sub && p.n_ens == n_ens && (int)p.subs.size() == n_sub, "plan header");
    CHECK(p.k_wave >= 0 && p.n_lane >= 0 && p.k_wave + p.n_lane == n_sub, "k_wave %d + n_lane %d != %d", p.k_wave, p.n_lane, n_sub);
    if (lim.forced_mapping == DABGPU_VIT_MAP_WAVE || (uint64_t)hist_frames * 230400u >= ((uint64_t)1 << 32)) CHECK(p.n_lane == 0, "lanes where they are ruled out");
    if (lim.forced_mapping == DABGPU_VIT_MAP_LANE || lim.forced_mapping == DABGPU_VIT_MAP_OCTET)
        CHECK((uint64_t)hist_frames * 230400u >= ((uint64_t)1 << 32) || (p.k_wave == 0 && p.octet == (lim.forced_mapping == DABGPU_VIT_MAP_OCTET)), "forced batch mapping");
    if (lim.forced_mapping != DABGPU_VIT_MAP_AUTO || lim.hybrid_k < 0 || lim.hybrid_k > n_sub) CHECK(p.k_wave == 0 || p.k_wave == n_sub, "a hybrid nobody asked for");
    else if (p.mapping != DABGPU_VIT_MAP_WAVE || (uint64_t)hist_frames * 230400u < ((uint64_t)1 << 32)) CHECK(p.k_wave == lim.hybrid_k, "hybrid_k %d gave k_wave %d", lim.hybrid_k, p.k_wave);
    // lane_mapped on exactly the n_lane shortest
    int flagged = 0; uint32_t longest_lane = 0, shortest_wave = UINT32_MAX, max_steps = 0, max_out = 0; u128 cif = 0;
    for (const auto& P : p.subs) {
        CHECK(P.lane_mapped <= 1, "lane_mapped %u", P.lane_mapped);
        if (P.lane_mapped) { flagged++; longest_lane = std::max(longest_lane, P.n_steps); } else shortest_wave = std::min(shortest_wave, P.n_steps);
        max_steps = std::max(max_steps, P.n_steps); max_out = std::max(max_out, P.n_out_bytes); cif += P.n_out_bytes;
    }
    CHECK(flagged == p.n_lane && (p.n_lane == 0 || p.k_wave == 0 || longest_lane <= shortest_wave), "lane_mapped is not on the %d shortest sub-channels", p.n_lane);
    CHECK(cif == p.cif_out_bytes, "cif_out_bytes");
    // the lane table: running sums in lane order, longest first
    CHECK(p.lane_subs.size() == (size_t)3 * p.n_lane && p.lane_subs_bytes == p.lane_subs.size() * 8 && p.plans_bytes == (size_t)n_sub * sizeof(dabgpu_msc_plan), "table sizes");
    u128 dec = 0, sym = 0; uint32_t lane_max = 0, lane_rows = 0, prev = UINT32_MAX; std::vector<char> seen((size_t)n_sub, 0);
    for (int j = 0; j < p.n_lane; j++) {
        const uint64_t sidx = p.lane_subs[(size_t)3 * j];
        CHECK(sidx < (uint64_t)n_sub && !seen[(size_t)sidx] && p.subs[(size_t)sidx].lane_mapped, "lane %d names sub-channel %llu", j, (unsigned long long)sidx);
        if (sidx >= (uint64_t)n_sub) return;
        seen[(size_t)sidx] = 1;
        const dabgpu_msc_plan& P = p.subs[(size_t)sidx];
        CHECK(p.lane_subs[(size_t)3 * j + 1] == dec && p.lane_subs[(size_t)3 * j + 2] == sym && P.n_steps <= prev, "lane %d offsets / order", j);
        prev = P.n_steps;
        const uint32_t rows = dabgpu_vit_in_rows(dabgpu_vit_in_bytes(P.seg_pi, P.seg_steps));
        dec += dabgpu_vit_alloc_steps(P.n_steps); sym += rows;
        lane_max = std::max(lane_max, P.n_steps); lane_rows = std::max(lane_rows, rows);
    }
    CHECK(dec == p.dec_rows_per_gq && sym == p.sym_rows_per_gq && lane_max == p.lane_max_steps && lane_rows == p.lane_max_in_rows, "rows per group quartet");
    if (p.n_lane) CHECK(p.sched_stride >= p.lane_max_steps + DABGPU_VIT_SCHED_PREFETCH && p.sched_stride % 64 == 0, "sched_stride %u for %u steps", p.sched_stride, p.lane_max_steps);
    // the FIC's place
    CHECK((p.fic == DABGPU_FIC_NONE) == !want_fic, "fic place %d, wanted %d", (int)p.fic, (int)want_fic);
    const u128 n_cw = (u128)n_ens * 4 * (u128)n_sub, n_fic = want_fic ? (u128)n_ens * 4 : 0;
    CHECK(p.n_cw == (n_cw > SIZE_MAX ? (u128)SIZE_MAX : n_cw) && p.n_fic_cw == n_fic, "codeword counts");
    const u128 descs = (n_cw + n_fic) * sizeof(dabgpu_codeword);
    CHECK(p.descs_bytes == (descs > SIZE_MAX ? (u128)SIZE_MAX : descs), "descs_bytes wrapped");
    if (p.fic == DABGPU_FIC_IN_LANES) CHECK(p.k_wave == 0 && p.n_lane > 0 && n_ens <= p.ens_per_slice && n_cw <= UINT32_MAX, "FIC_IN_LANES outside one all-lane slice");
    if (p.fic == DABGPU_FIC_IN_WAVE) CHECK(p.k_wave == n_sub, "FIC_IN_WAVE with lane-mapped sub-channels");
    CHECK(p.fic_dec_rows == 832 && p.fic_in_rows == 578, "FIB group rows %u / %u", p.fic_dec_rows, p.fic_in_rows);
    CHECK(p.max_steps == std::max(max_steps, p.fic == DABGPU_FIC_IN_WAVE ? DABGPU_FIC_STEPS : 0u) && p.max_out_bytes == std::max(max_out, p.fic == DABGPU_FIC_IN_WAVE ? DABGPU_FIC_OUT_BYTES : 0u), "wave launch maxima");
    CHECK((u128)p.sched_bytes == ((u128)p.n_lane * p.sched_stride + (p.fic == DABGPU_FIC_IN_LANES ? p.fic_dec_rows : 0)) * 8, "sched_bytes");
    if (!p.n_lane) return;
    // slices tile [0, n_ens): each starts at a multiple of ens_per_slice and takes min(rest, ens_per_slice); first, last and a random one
    CHECK(p.ens_per_slice >= 16 && p.ens_per_slice % 16 == 0, "ens_per_slice %zu", p.ens_per_slice);
    const size_t n_slices = n_ens / p.ens_per_slice + (n_ens % p.ens_per_slice != 0);
    const size_t picks[3] = {0, n_slices - 1, (size_t)(((uint64_t)rng() << 32 | rng()) % n_slices)};
    for (size_t k : picks) {
        const size_t e0 = k * p.ens_per_slice;
        const dabgpu_decode_slice sl = dabgpu_host_decode_slice(p, e0);
        CHECK(sl.ne >= 1 && sl.ne == std::min(n_ens - e0, p.ens_per_slice) && (k + 1 == n_slices) == (e0 + sl.ne == n_ens), "slice %zu of %zu: %zu ensembles", k, n_slices, sl.ne);
        const u128 gps = ((u128)sl.ne * 4 + 63) / 64, msc_dec = dec * gps, msc_sym = sym * gps, fg = p.fic == DABGPU_FIC_IN_LANES ? ((u128)n_ens * 4 + 63) / 64 : 0;
        CHECK(sl.gps == gps && gps <= UINT32_MAX && sl.n_groups == (u128)p.n_lane * gps && sl.n_fic_groups == fg, "slice groups");
        CHECK(sl.dec_rows == msc_dec + fg * 832 && sl.sym_rows == msc_sym + fg * 578 && (u128)sl.dec_rows * 512 <= SIZE_MAX && (u128)sl.sym_rows * 256 <= SIZE_MAX, "slice rows");
        CHECK(sl.dec_rows <= lim.max_dec_rows || gps == 1, "slice of %zu decision rows over the bound %zu", sl.dec_rows, lim.max_dec_rows);
        CHECK(sl.groups_bytes == ((u128)sl.n_groups + fg) * sizeof(dabgpu_vit_group), "groups_bytes");
        if (n_cw <= SIZE_MAX) CHECK(sl.cw0 == (u128)e0 * 4 * (u128)n_sub, "cw0");
        if (p.fic == DABGPU_FIC_IN_LANES)       // the appended groups start exactly where the MSC's end
            CHECK(n_slices == 1 && sl.fic_base.first == n_cw && sl.fic_base.sched_off == (u128)p.n_lane * p.sched_stride && sl.fic_base.sym_off == msc_sym * 64 &&
                  sl.fic_base.dec_off == msc_dec * 128 && sl.fic_base.res_delta == 0, "appended FIB groups");
    }
}

// Hand-worked plans of the shapes the project measures.  Every number below is worked out from the expressions of the decode entry points as
// they stood before the planner existed (rows: alloc = (steps + 6 + 63) & ~63, in_rows = (12 + sum steps/8 x (8 + PI) + 3) / 4 + 2; bound:
// MB x 2^20 / 768 rows; cost model: dabgpu_host_choose_msc_mapping on 1024 SIMDs), not by running it.
static void planner_table() {
    dabgpu_decode_limits lim = {1024.0, ROWS_6GIB, -1, DABGPU_VIT_MAP_AUTO};
    dabgpu_decode_plan p;
    // (1) the headline multiplex: 18 x 48 CU EEP 3-A (45 x PI_8 + 3 x PI_7: 1536 + 6 = 1542 steps, alloc 1600, 3072 soft bits -> 770 rows, 192
    // bytes), 4096 ensembles, FIC wanted.  Model: groups = 18 x 256 = 4608; t_wave ~ 13460, t_lane = 0.5 x 5 x 1542 + 1500.7 + 20 ~ 5376, t_oct =
    // 0.095 x 36 x 1542 + 1520.7 ~ 6794 -> LANE.  Rows per quartet 18 x 1600 = 28800 / 18 x 770 = 13860; 8388608 / 28800 = 291 quartets = 4656
    // ensembles a slice; with the FIB group's 832 rows 8388608 / 29632 = 283 -> 4528 >= 4096: the FIC joins.  4608 + 256 groups on 5120 slots.
    std::vector<dabgpu_subchannel> s18;
    for (int k = 0; k < 18; k++) s18.push_back(eep(48 * k, 48, 2, 0));
    CHECK(dabgpu_host_plan_decode(s18.data(), 18, 4096, 8, true, lim, &p) == DABGPU_OK, "headline plan");
    CHECK(p.mapping == DABGPU_VIT_MAP_LANE && p.k_wave == 0 && p.n_lane == 18 && p.octet == 0 && p.fic == DABGPU_FIC_IN_LANES, "headline mapping %d k %d fic %d", p.mapping, p.k_wave, (int)p.fic);
    CHECK(p.cif_out_bytes == 3456 && p.max_steps == 1542 && p.max_out_bytes == 192 && p.lane_max_steps == 1542 && p.lane_max_in_rows == 770 && p.sched_stride == 1600, "headline sizes");
    CHECK(p.dec_rows_per_gq == 28800 && p.sym_rows_per_gq == 13860 && p.ens_per_slice == 4656 && p.n_cw == 294912 && p.n_fic_cw == 16384, "headline rows");
    CHECK(p.sched_bytes == (28800 + 832) * 8 && p.descs_bytes == (294912 + 16384) * sizeof(dabgpu_codeword), "headline bytes");
    for (int j = 0; j < 18; j++) CHECK(p.lane_subs[3 * j + 1] == 1600u * j && p.lane_subs[3 * j + 2] == 770u * j, "headline lane %d", j);
    dabgpu_decode_slice sl = dabgpu_host_decode_slice(p, 0);
    CHECK(sl.ne == 4096 && sl.cw0 == 0 && sl.gps == 256 && sl.n_groups == 4608 && sl.n_fic_groups == 256 && sl.n_groups + sl.n_fic_groups <= 5120, "headline groups");
    CHECK(sl.sym_rows == 3548160 + 147968 && sl.dec_rows == 7372800 + 212992, "headline slice rows %zu / %zu", sl.sym_rows, sl.dec_rows);
    CHECK(sl.fic_base.first == 294912 && sl.fic_base.sched_off == 28800 && sl.fic_base.sym_off == 227082240ull && sl.fic_base.dec_off == 943718400ull, "headline FIB groups");
    // (2) the same without the FIC (the MSC entry points), and the FIC of 4096 frames alone: 16384 codewords = 256 groups; t_wave = 61.9 + 279.0 +
    // 185.1 ~ 526, t_lane = 387 + 41.8 + 20 ~ 449, t_oct = 0.095 x 1548 + 61.8 ~ 209 -> OCTET; 8388608 / 832 = 10082 groups a launch
    CHECK(dabgpu_host_plan_decode(s18.data(), 18, 4096, 8, false, lim, &p) == DABGPU_OK && p.fic == DABGPU_FIC_NONE && p.n_lane == 18 && p.n_fic_cw == 0, "MSC alone");
    sl = dabgpu_host_decode_slice(p, 0);
    CHECK(sl.n_groups == 4608 && sl.n_fic_groups == 0 && sl.sym_rows == 3548160 && sl.dec_rows == 7372800 && p.sched_bytes == 28800 * 8, "MSC alone: slice");
    dabgpu_uniform_plan u = dabgpu_host_plan_fic(16384, true, lim);
    CHECK(u.mapping == DABGPU_VIT_MAP_OCTET && u.dec_rows == 832 && u.in_rows == 578 && u.slice_groups == 10082, "FIC alone: %d %u %u %zu", u.mapping, u.dec_rows, u.in_rows, u.slice_groups);
    // (3) one ensemble x 18 sub-channels, FIC wanted (the frame session): t_wave = 123.4 + 4 x 0.814 ~ 127 against 771 + .. / 293 + .. -> WAVE, and the
    // FIC's 4 codewords alone: 62 against 387 + .. / 147 + .. -> WAVE too: one viterbi_kernel launch of 72 + 4 codewords
    CHECK(dabgpu_host_plan_decode(s18.data(), 18, 1, 8, true, lim, &p) == DABGPU_OK, "session plan");
    CHECK(p.mapping == DABGPU_VIT_MAP_WAVE && p.k_wave == 18 && p.n_lane == 0 && p.fic == DABGPU_FIC_IN_WAVE && p.n_cw == 72 && p.n_fic_cw == 4 && p.lane_subs.empty(), "session mapping");
    CHECK(p.max_steps == 1542 && p.max_out_bytes == 192 && p.descs_bytes == 76 * sizeof(dabgpu_codeword) && p.sched_bytes == 0, "session sizes");
    // (4) the heterogeneous multiplex (14 sub-channels), 4096 ensembles, FIC wanted.  steps / alloc / in_rows / bytes per sub-channel:
    //   3 x 48 CU 3-A 1542/1600/770/192   3 x 60 CU 3-A (57 + 3 blocks) 1926/1984/962/240   2 x 72 CU 3-A (69 + 3) 2310/2368/1154/288
    //   2 x 42 CU 2-B (45 x PI_6 + 3 x PI_5: 2688 soft bits) 1542/1600/674/192   UEP 35 (11, 22, 60, 3 x PI 16, 9, 6, 10: 6140) 3078/3136/1537/384
    //   UEP 38 (11, 19, 87, 3 x PI 5, 4, 2, 4: 5120) 3846/3904/1282/480   UEP 43 (11, 20, 110, 3 x PI 6, 4, 2, 5: 6144) 4614/4672/1538/576
    //   8 CU 2-A (5 x PI_13 + 1 x PI_12: 512) 198/256/130/24
    // sums: decision rows 30656, symbol rows 13339, bytes 3720.  Model: 3584 groups, mean 2131.7: t_lane = 0.5 x 4 x 2131.7 + 1633.6 ~ 5897 <
    // t_oct ~ 7304 < t_wave ~ 13718 -> LANE.  8388608 / 30656 = 273 -> 4368 a slice; / 31488 = 266 -> 4256 >= 4096: the FIC joins.
    std::vector<dabgpu_subchannel> mix;
    int at = 0;
    for (int len : {48, 48, 48, 60, 60, 60, 72, 72}) { mix.push_back(eep(at, len, 2, 0)); at += len; }
    for (int k = 0; k < 2; k++) { mix.push_back(eep(at, 42, 1, 1)); at += 42; }
    mix.push_back(uep(at, 96, 35)); at += 96; mix.push_back(uep(at, 80, 38)); at += 80; mix.push_back(uep(at, 96, 43)); at += 96;
    mix.push_back(eep(at, 8, 1, 0));
    CHECK(dabgpu_host_plan_decode(mix.data(), 14, 4096, 8, true, lim, &p) == DABGPU_OK, "mixed plan");
    CHECK(p.mapping == DABGPU_VIT_MAP_LANE && p.k_wave == 0 && p.n_lane == 14 && p.fic == DABGPU_FIC_IN_LANES && p.cif_out_bytes == 3720, "mixed mapping");
    CHECK(p.dec_rows_per_gq == 30656 && p.sym_rows_per_gq == 13339 && p.ens_per_slice == 4368 && p.lane_max_steps == 4614 && p.lane_max_in_rows == 1538 && p.sched_stride == 4672, "mixed rows");
    CHECK(p.lane_subs[0] == 12 && p.lane_subs[3] == 11 && p.lane_subs[4] == 4672 && p.lane_subs[5] == 1538 && p.lane_subs[6] == 10 && p.lane_subs[7] == 4672 + 3904 &&
          p.lane_subs[8] == 1538 + 1282 && p.lane_subs[3 * 13] == 13 && p.lane_subs[3 * 13 + 1] == 30656 - 256 && p.lane_subs[3 * 13 + 2] == 13339 - 130, "mixed lane table");
    sl = dabgpu_host_decode_slice(p, 0);
    CHECK(sl.n_groups == 3584 && sl.n_fic_groups == 256 && sl.dec_rows == 7847936 + 212992 && sl.sym_rows == 3414784 + 147968, "mixed slice");
    CHECK(sl.fic_base.first == 229376 && sl.fic_base.sched_off == 65408 && sl.fic_base.sym_off == 218546176ull && sl.fic_base.dec_off == 1004535808ull, "mixed FIB groups");
    // (5) the tests' slicing case: 2 MB = 2730 rows, the lane mapping forced, 100 ensembles x 18 sub-channels.  A quartet (28800 rows) is over the
    // bound: one quartet = 16 ensembles a slice all the same, 7 slices, the last of 4 ensembles; the FIC cannot join (16 < 100) and, forced into the
    // lane mapping, goes first on its own: 400 codewords = 7 groups, 2730 / 832 = 3 a launch
    lim.max_dec_rows = ROWS_2MIB; lim.forced_mapping = DABGPU_VIT_MAP_LANE;
    CHECK(ROWS_2MIB == 2730 && dabgpu_host_plan_decode(s18.data(), 18, 100, 8, true, lim, &p) == DABGPU_OK, "sliced plan");
    CHECK(p.n_lane == 18 && p.ens_per_slice == 16 && p.fic == DABGPU_FIC_OWN_LAUNCH && p.sched_bytes == 28800 * 8, "sliced mapping");
    sl = dabgpu_host_decode_slice(p, 96);
    CHECK(sl.ne == 4 && sl.cw0 == 96 * 72 && sl.gps == 1 && sl.n_groups == 18 && sl.n_fic_groups == 0 && sl.dec_rows == 28800 && sl.sym_rows == 13860, "last slice");
    u = dabgpu_host_plan_fic(400, true, lim);
    CHECK(u.mapping == DABGPU_VIT_MAP_LANE && u.slice_groups == 3, "sliced FIC");
}

int main(int argc, char** argv) {
    const int iters = argc > 1 ? std::atoi(argv[1]) : 20000;
    std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    auto wild = [&]() -> int {                     // mostly small, sometimes extreme
        switch (rng() % 8) { case 0: return INT32_MIN; case 1: return INT32_MAX; case 2: return -1; case 3: return 0; case 4: return pick(-70000, 70000); default: return pick(-5, 900); }
    };
    long accepted_plans = 0, accepted_wav = 0, accepted_cw = 0, accepted_decode = 0;

    for (int it = 0; it < iters; it++) {
        // ---- sub-channel plans ----
        {
            const int n_sub = (it % 97 == 0) ? pick(60, 80) : pick(0, 20);
            std::vector<dabgpu_subchannel> subs((size_t)(n_sub > 0 ? n_sub : 0));
            for (auto& s : subs) {
                const bool sane = rng() % 3 != 0;
                s.is_uep = (int)(rng() % 2);
                s.uep_prot_index = sane ? pick(0, 63) : wild();
                s.eep_prot_level = sane ? pick(0, 3) : wild();
                s.eep_type = sane ? pick(0, 1) : wild();
                s.start_address = sane ? pick(0, 800) : wild();
                s.length = sane ? (s.eep_type == 0 ? (int[]){12, 8, 6, 4}[s.eep_prot_level & 3] : (int[]){27, 21, 18, 15}[s.eep_prot_level & 3]) * pick(1, 8) : wild();
            }
            std::vector<dabgpu_msc_plan> plans;
            uint32_t off = 0, ms = 0, mo = 0;
            const int st = dabgpu_host_build_msc_plans(subs.empty() ? nullptr : subs.data(), n_sub, plans, &off, &ms, &mo);
            CHECK(st == DABGPU_OK || st == DABGPU_ERR_INVALID_ARG, "build_msc_plans status %d", st);
            if (st == DABGPU_OK) {
                accepted_plans++;
                CHECK((int)plans.size() == n_sub && n_sub <= 64, "plans %zu for %d sub-channels", plans.size(), n_sub);
                uint32_t run = 0;
                for (int k = 0; k < n_sub; k++) {
                    const dabgpu_msc_plan& P = plans[(size_t)k];
                    uint32_t steps = 0;
                    for (int j = 0; j < 4; j++) { steps += P.seg_steps[j]; CHECK(P.seg_steps[j] % 32 == 0 && P.seg_pi[j] <= 24, "segment %u x PI %u", P.seg_steps[j], P.seg_pi[j]); }
                    CHECK(P.n_steps == steps + 6 && P.out_offset == run && P.n_out_bytes * 8 == steps, "plan %d inconsistent", k);
                    CHECK(subs[(size_t)k].start_address >= 0 && subs[(size_t)k].start_address + subs[(size_t)k].length <= 864 && subs[(size_t)k].length > 0, "accepted a sub-channel outside the CIF");
                    CHECK(dabgpu_vit_in_bytes(P.seg_pi, P.seg_steps) <= (uint32_t)subs[(size_t)k].length * 64u, "plan %d consumes %u soft bits of %d CU", k,
                          dabgpu_vit_in_bytes(P.seg_pi, P.seg_steps), subs[(size_t)k].length);
                    run += P.n_out_bytes;
                    CHECK(P.n_steps <= ms && P.n_out_bytes <= mo, "maxima");
                }
                CHECK(run == off, "output bytes per CIF");
            }
            for (const auto& s : subs) {           // the public single-profile form on the same descriptors
                int pi[4], lx[4], nb = -7;
                const int nseg = dabgpu_subchannel_plan(&s, pi, lx, &nb);
                CHECK(nseg == -1 || nseg == 2 || nseg == 4, "subchannel_plan returned %d", nseg);
                if (nseg > 0) for (int j = 0; j < 4; j++) CHECK(lx[j] >= 0 && pi[j] >= 0 && pi[j] <= 24, "plan values");
            }
            (void)dabgpu_subchannel_plan(nullptr, nullptr, nullptr, nullptr);
        }
        // ---- decode planner ----
        {
            const bool sane = rng() % 4 != 0;
            const int n_sub = sane ? pick(1, 64) : (rng() % 8 ? pick(1, 64) : pick(60, 70));
            std::vector<dabgpu_subchannel> subs((size_t)n_sub);
            for (auto& s : subs) {
                if (rng() % 3 == 0) s = uep(pick(0, 864 - 416), 416, pick(0, 63));          // (any table row fits 416 CU)
                else { const int type = pick(0, 1), level = pick(0, 3); const int unit = type == 0 ? (int[]){12, 8, 6, 4}[level] : (int[]){27, 21, 18, 15}[level]; s = eep(pick(0, 600), unit * pick(1, 8), level, type); }
                if (!sane && rng() % 6 == 0) { s.length = wild(); s.start_address = wild(); s.uep_prot_index = wild(); }
            }
            static const size_t big[4] = {SIZE_MAX / 4 - 16, SIZE_MAX / 4 - 1000, SIZE_MAX / 8, (size_t)1 << 40};
            const size_t n_ens = rng() % 16 == 0 ? big[rng() % 4] : (rng() % 2 ? (size_t)pick(1, 300) : (size_t)1 + rng() % ((size_t)1 << 20));
            const int hist_frames = rng() % 8 == 0 ? pick(18000, 32768) : pick(5, 64);
            dabgpu_decode_limits lim;
            lim.n_simd = (double)pick(1, 2048);
            lim.max_dec_rows = rng() % 3 == 0 ? (size_t)pick(1, 5000) : (rng() % 2 ? ROWS_6GIB : (size_t)1 + (((uint64_t)rng() << 32 | rng()) % ((uint64_t)1 << 36)));
            lim.hybrid_k = rng() % 2 ? -1 : pick(-3, n_sub + 3);
            lim.forced_mapping = pick(0, 3);
            const bool want_fic = rng() % 2;
            dabgpu_decode_plan p;
            std::vector<dabgpu_msc_plan> ref;
            const int st = dabgpu_host_plan_decode(subs.data(), n_sub, n_ens, hist_frames, want_fic, lim, &p);
            CHECK((st == DABGPU_OK || st == DABGPU_ERR_INVALID_ARG) && st == dabgpu_host_build_msc_plans(subs.data(), n_sub, ref, nullptr, nullptr, nullptr), "plan_decode status %d", st);
            if (st == DABGPU_OK) { accepted_decode++; check_plan(p, subs, n_ens, hist_frames, want_fic, lim, rng); }
            const size_t n_cw = (size_t)(rng() % 4 == 0 ? 0 : rng());
            const uint32_t seg_pi[4] = {(uint32_t)pick(1, 24), (uint32_t)pick(1, 24), 0, 0}, seg_steps[4] = {8u * (uint32_t)pick(1, 300), 8u * (uint32_t)pick(0, 60), 0, 0};
            const dabgpu_uniform_plan u = dabgpu_host_plan_uniform(n_cw, seg_steps[0] + seg_steps[1] + 6, seg_pi, seg_steps, rng() % 2, lim);
            CHECK(u.mapping >= DABGPU_VIT_MAP_WAVE && u.mapping <= DABGPU_VIT_MAP_OCTET && u.slice_groups >= 1 && (u.slice_groups == 1 || (u128)u.slice_groups * u.dec_rows <= lim.max_dec_rows) &&
                  u.dec_rows >= seg_steps[0] + seg_steps[1] + 6 + DABGPU_VIT_SCHED_PREFETCH && u.in_rows * 4u >= dabgpu_vit_in_bytes(seg_pi, seg_steps) + 8, "uniform plan");
        }
        // ---- wav headers ----
        {
            std::vector<uint8_t> img = (it % 5 == 0) ? std::vector<uint8_t>((size_t)pick(0, 200)) : wav_image(rng);
            if (it % 5 == 0) for (auto& b : img) b = (uint8_t)rng();
            for (unsigned m = rng() % 4; m > 0 && !img.empty(); m--) {
                const size_t at = rng() % img.size();
                switch (rng() % 4) {
                case 0: img[at] = (uint8_t)rng(); break;
                case 1: if (at + 4 <= img.size()) { const uint32_t lie = (rng() % 2) ? 0xFFFFFFF0u + (rng() % 16) : (uint32_t)rng(); std::memcpy(&img[at], &lie, 4); } break;   // lying size field
                case 2: img.resize(at); break;                                                                                                                         // truncation
                default: img.insert(img.begin() + (std::ptrdiff_t)at, (size_t)(rng() % 9), (uint8_t)0); break;
                }
            }
            // exact-size heap copy: any read past n_bytes is an ASan report
            std::vector<uint8_t> exact(img);
            exact.shrink_to_fit();
            dabgpu_wav_header h;
            const int st = dabgpu_wav_parse_header(exact.empty() ? nullptr : exact.data(), exact.size(), &h);
            CHECK(st == DABGPU_OK || st == DABGPU_ERR_INVALID_ARG, "wav status %d", st);
            if (st == DABGPU_OK) {
                accepted_wav++;
                CHECK(h.data_chunk_offset <= exact.size(), "data offset %llu beyond the %zu-byte image", (unsigned long long)h.data_chunk_offset, exact.size());
                CHECK(h.iq_format >= DABGPU_IQ_WAV_PCM8 && h.iq_format < DABGPU_IQ_NB_FORMATS && (h.total_channels == 1 || h.total_channels == 2), "accepted header fields");
                CHECK(dabgpu_iq_format_sample_bytes(h.iq_format) == 2u * (h.bits_per_sample / 8u), "sample bytes of format %d", h.iq_format);
            }
            (void)dabgpu_wav_parse_header(exact.data(), exact.size(), nullptr);
        }
        // ---- codeword descriptors ----
        {
            dabgpu_codeword d;
            std::memset(&d, 0, sizeof(d));
            const bool sane = rng() % 2 == 0;
            uint32_t steps = 0;
            for (int k = 0; k < 4; k++) {
                d.seg_pi[k] = sane ? (uint32_t)pick(1, 24) : (uint32_t)wild();
                d.seg_steps[k] = sane ? 8u * (uint32_t)pick(0, 100) : (uint32_t)wild();
                steps += d.seg_steps[k];
            }
            d.n_steps = (rng() % 4) ? steps + 6 : (uint32_t)wild();
            d.d_src = (rng() % 8) ? 0x1000 : 0; d.d_out = (rng() % 8) ? 0x2000 : 0;
            d.n_slots = (rng() % 3) ? 0 : (uint32_t)wild();
            d.newest_slot = (uint32_t)wild(); d.cifs_per_frame = (uint32_t)pick(0, 5); d.cif_stride = (uint32_t)wild(); d.frame_stride = (uint32_t)wild();
            d.flags = (uint32_t)(rng() % 16);
            const int st = dabgpu_host_validate_codeword(d, (size_t)it);
            CHECK(st == DABGPU_OK || st == DABGPU_ERR_INVALID_ARG, "validate_codeword status %d", st);
            if (st == DABGPU_OK) {
                accepted_cw++;
                CHECK(d.d_src && d.d_out && d.n_steps >= 1, "accepted a codeword without addresses / steps");
                if (!(d.flags & DABGPU_CW_DEPUNCTURED)) CHECK(d.n_steps == steps + 6 && (steps % 8) == 0, "accepted n_steps %u for %u segment steps", d.n_steps, steps);
                if (d.n_slots) CHECK(d.n_slots >= 16 && d.cifs_per_frame > 0 && d.newest_slot < d.n_slots, "accepted ring geometry");
            }
        }
        // ---- cost model, run-length rules, tables ----
        {
            const size_t n_cw = (size_t)(rng() % 5 == 0 ? 0 : rng() % 500000), n_groups = (n_cw + 63) / 64;
            const double steps = (double)pick(1, 5000);
            const int forced = pick(0, 3);
            const int m = dabgpu_host_choose_mapping(forced, (rng() % 7 == 0) ? 0.0 : (double)pick(1, 2048), n_cw, n_groups, (double)n_cw * steps, (double)n_groups * steps, steps, rng() % 2);
            CHECK(m >= DABGPU_VIT_MAP_WAVE && m <= DABGPU_VIT_MAP_OCTET, "mapping %d", m);
            if (forced != DABGPU_VIT_MAP_AUTO) CHECK(m == forced, "a forced mapping must come back unchanged");
            const size_t nf = (size_t)(rng() % 3 ? rng() % 3000 : rng());
            const int spb = dabgpu_host_small_batch_spb(nf ? nf : 1);
            CHECK(spb >= 3 && spb <= 25, "small-batch run length %d for %zu frames", spb, nf);
            const int b = dabgpu_host_spb_bucket(nf);
            CHECK(b >= 0 && b <= 40 && (nf <= 1 || ((size_t)1 << b) >= nf || b == 40), "bucket %d of %zu", b, nf);
            const int mode = pick(-3, 8);
            int geom[9];
            const int gs = dabgpu_get_ofdm_params(mode, geom);
            CHECK((gs == DABGPU_OK) == (mode >= 1 && mode <= 4), "get_ofdm_params(%d) = %d", mode, gs);
            if (gs == DABGPU_OK) {
                std::vector<float> prs(2 * (size_t)geom[3]);
                std::vector<int> map((size_t)geom[5]);
                CHECK(dabgpu_get_prs_fft_ref(mode, prs.data()) == DABGPU_OK && dabgpu_get_carrier_mapper(mode, map.data()) == DABGPU_OK, "tables of mode %d", mode);
                std::vector<char> seen((size_t)geom[5], 0);
                for (int v : map) { CHECK(v >= 0 && v < geom[5] && !seen[(size_t)v], "mapper of mode %d is not a permutation", mode); if (v >= 0 && v < geom[5]) seen[(size_t)v] = 1; }
            } else {
                float dummy[4]; int idummy[4];
                CHECK(dabgpu_get_prs_fft_ref(mode, dummy) != DABGPU_OK && dabgpu_get_carrier_mapper(mode, idummy) != DABGPU_OK, "tables of an invalid mode");
            }
            std::string name;
            for (unsigned k = rng() % 12; k > 0; k--) name.push_back((char)(rng() % 96 + 32));
            const int f = dabgpu_iq_format_from_mode((rng() % 4) ? name.c_str() : "raw_s16l");
            CHECK(f >= -1 && f < 14, "format %d", f);
            CHECK(dabgpu_iq_format_sample_bytes(wild()) <= 16, "sample bytes");
            (void)dabgpu_iq_format_from_mode(nullptr);
            (void)dabgpu_strerror(wild());
        }
    }
    // the Viterbi constant tables against an independent statement of ETSI EN 300 401 table 13 and clause 10
    {
        dabgpu_vit_tables T;
        dabgpu_host_fill_vit_tables(&T);
        for (int pi = 1; pi <= 24; pi++) {
            int total = 0;
            for (int g = 0; g < 8; g++) { const int cnt = T.pi_tab[pi * 8 + g] & 0xFF, pre = T.pi_tab[pi * 8 + g] >> 8; CHECK(cnt >= 1 && cnt <= 4 && pre == total, "PI_%d group %d", pi, g); total += cnt; }
            CHECK(total == 8 + pi, "PI_%d keeps %d of 32", pi, total);
        }
        unsigned reg = 0x1FF;                             // x^9 + x^5 + 1, all ones
        for (int k = 0; k < 64; k++) {
            unsigned byte = 0;
            for (int i = 0; i < 8; i++) { const unsigned v = ((reg >> 8) ^ (reg >> 4)) & 1u; byte = (byte << 1) | v; reg = ((reg << 1) | v) & 0x1FF; }
            CHECK(T.prbs[k] == byte, "energy-dispersal byte %d", k);
        }
    }
    planner_table();
    std::printf("{\"iterations\": %d, \"accepted_plans\": %ld, \"accepted_wav\": %ld, \"accepted_codewords\": %ld, \"accepted_decode_plans\": %ld, \"failed_checks\": %d}\n", iters,
                accepted_plans, accepted_wav, accepted_cw, accepted_decode, g_fail);
    return g_fail ? 1 : 0;
}
