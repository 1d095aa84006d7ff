// dabgpu_decode_abi.hip -- channel-decode entry points of the C ABI (include/dabgpu.h): protection-profile
// tables, codeword descriptors, scratch sizing and launches.  Host side only; the arithmetic is in viterbi.hip.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <vector>

#include "dabgpu.h"
#include "dabgpu_internal.h"

static int device_waves(dabgpu_ctx* c) {
    if (c->n_cu <= 0) {
        hipDeviceProp_t p;
        c->n_cu = (hipGetDeviceProperties(&p, c->device) == hipSuccess) ? p.multiProcessorCount : 256;
    }
    return c->n_cu * 32;          // 8 waves per SIMD: the decoder is a serial recurrence per wave, throughput = waves in flight
}

// What the planner (dabgpu_host_logic.h) is told about this context and process, read once per entry-point call.  The symbol / decision
// scratch of a lane launch is bounded at <= 768 bytes per decision row: 6 GiB by default, DABGPU_VIT_SCRATCH_MB in the environment overrides.
static dabgpu_decode_limits decode_limits(dabgpu_ctx* c) {
    dabgpu_decode_limits lim;
    lim.n_simd = (double)device_waves(c) / 8.0;
    size_t mb = 6144;
    if (const char* e = getenv("DABGPU_VIT_SCRATCH_MB")) { const long v = atol(e); if (v > 0) mb = (size_t)v; }
    lim.max_dec_rows = std::max<size_t>(mb * 1024 * 1024 / 768, 1);
    const char* k = getenv("DABGPU_VIT_HYBRID_K");      // tests
    lim.hybrid_k = k ? atoi(k) : -1;
    lim.forced_mapping = c->vit_mapping;
    return lim;
}

// the staged gathers read aligned chunks of `a` bytes: every row (base + k * stride) must start on one
static bool rows_aligned(const void* base, size_t stride, size_t a) { return (uintptr_t)base % a == 0 && stride % a == 0; }

// kept-count vectors PI_1..PI_24 (ETSI EN 300 401 table 13: PI_n keeps 8+n of every 32 mother bits, the e-th extra bit in
// 4-bit group bitrev3(e mod 8)) as count | prefix << 8, and the energy-dispersal PRBS x^9+x^5+1 seeded with all ones
static int ensure_vit_tables(dabgpu_ctx* c) {
    if (c->d_vit_tables) return DABGPU_OK;
    dabgpu_vit_tables T;
    dabgpu_host_fill_vit_tables(&T);
    int st = dabgpu_check_hip(hipMalloc((void**)&c->d_vit_tables, sizeof(T)), "hipMalloc(vit tables)");
    if (st) return st;
    return dabgpu_check_hip(hipMemcpy(c->d_vit_tables, &T, sizeof(T), hipMemcpyHostToDevice), "hipMemcpy(vit tables)");
}

// one wavefront per codeword.  fic: the FIC entry points keep their device scratch in slots of their own (scratch_fic)
int dabgpu_run_viterbi(dabgpu_ctx* c, const dabgpu_cw_desc* d_descs, size_t n, uint32_t max_steps, uint32_t max_out_bytes, int tie_rule,
                       dabgpu_codeword_result* d_results, hipStream_t s, bool fic, size_t n_first, dabgpu_codeword_result* d_results_rest) {
    int st0 = ensure_vit_tables(c);
    if (st0) return st0;
    const int n_waves = (int)std::min<size_t>(n, (size_t)device_waves(c));
    const size_t words = ((size_t)max_steps + 63) & ~(size_t)63;
    uint64_t* d_scratch = nullptr;
    int st = dabgpu_scratch(c, scratch_fic<SCR_VIT_WAVE>(fic), (size_t)n_waves * words * sizeof(uint64_t), (void**)&d_scratch, s);
    if (st) return st;
    return dabgpu_check_hip(dabgpu_launch_viterbi(d_descs, (int)n, d_scratch, words, n_waves, (int)max_out_bytes, d_results,
                                                  tie_rule ? 1 : 0, c->d_vit_tables, s, (int)n_first, d_results_rest), "viterbi_kernel launch");
}

extern "C" int dabgpu_viterbi_set_mapping(dabgpu_ctx* c, int mapping) {
    if (!c || mapping < DABGPU_VIT_MAP_AUTO || mapping > DABGPU_VIT_MAP_OCTET) { dabgpu_set_error("viterbi_set_mapping: bad argument"); return DABGPU_ERR_INVALID_ARG; }
    c->vit_mapping = mapping;
    return DABGPU_OK;
}

// The lane-per-codeword (or octet) decoder over groups that were built: gather(s), then one trellis launch.  `more` are further groups
// right behind `first` in d_groups with a gather of their own (the FIB groups inside an MSC launch); sym_rows / dec_rows: rows of 64
// dwords (kept soft bits, 4 per lane and row) and of 128 dwords (decisions, one row per step) of all of them.
struct lane_groups { size_t n; int gather; uint32_t max_in_rows, groups_per_sub; };      // gather: dabgpu_launch_vit_prep's `kind`
static int run_viterbi_lanes(dabgpu_ctx* c, const dabgpu_cw_desc* d_descs, const dabgpu_vit_group* d_groups, lane_groups first, lane_groups more,
                             size_t sym_rows, size_t dec_rows, int tie_rule, const uint2* d_sched, int octet, dabgpu_codeword_result* d_results,
                             hipStream_t s, bool fic) {
    int st;
    uint32_t *d_sym = nullptr, *d_dec = nullptr;
    if ((st = dabgpu_scratch(c, scratch_fic<SCR_VIT_SYM>(fic), sym_rows * 64 * sizeof(uint32_t), (void**)&d_sym, s))) return st;
    if ((st = dabgpu_scratch(c, scratch_fic<SCR_VIT_DEC>(fic), dec_rows * 128 * sizeof(uint32_t), (void**)&d_dec, s))) return st;
    if ((st = dabgpu_check_hip(dabgpu_launch_vit_prep(first.gather, d_groups, first.n, first.max_in_rows, d_descs, d_sym, first.groups_per_sub, s), "vit_prep launch"))) return st;
    if (more.n && (st = dabgpu_check_hip(dabgpu_launch_vit_prep(more.gather, d_groups + first.n, more.n, more.max_in_rows, d_descs, d_sym, more.groups_per_sub, s),
                                         "vit_prep launch"))) return st;
    return dabgpu_check_hip(dabgpu_launch_vit_trellis(d_groups, first.n + more.n, d_descs, d_sym, d_dec, d_results, tie_rule ? 1 : 0, c->d_vit_tables, d_sched,
                                                      octet, device_waves(c) / 32, s), "vit_lanes_kernel launch");
}

// one puncturing schedule for a whole batch (FIC, uniform codeword batches): groups of 64 consecutive codewords, in bounded slices
static int run_lanes_uniform(dabgpu_ctx* c, const dabgpu_uniform_plan& u, const dabgpu_cw_desc* d_descs, size_t n, uint32_t n_steps,
                             const uint32_t* seg_pi, const uint32_t* seg_steps, int tie_rule, int gather, dabgpu_codeword_result* d_results,
                             hipStream_t s, bool fic) {
    int st = ensure_vit_tables(c);
    if (st) return st;
    uint2* d_sched = nullptr;
    if ((st = dabgpu_scratch(c, scratch_fic<SCR_VIT_SCHED>(fic), (size_t)u.dec_rows * sizeof(uint2), (void**)&d_sched, s))) return st;
    if ((st = dabgpu_check_hip(dabgpu_launch_vit_sched_uniform(d_sched, u.dec_rows, seg_pi, seg_steps, c->d_vit_tables, s), "vit_sched launch"))) return st;
    for (size_t cw0 = 0; cw0 < n; cw0 += u.slice_groups * 64) {
        const size_t n_cw = std::min(n - cw0, u.slice_groups * 64), n_groups = (n_cw + 63) / 64;
        dabgpu_vit_group* d_groups = nullptr;
        if ((st = dabgpu_scratch(c, scratch_fic<SCR_VIT_GROUPS>(fic), n_groups * sizeof(dabgpu_vit_group), (void**)&d_groups, s))) return st;
        if ((st = dabgpu_check_hip(dabgpu_launch_vit_groups_uniform(d_groups, n_cw, n_steps, seg_pi, seg_steps, s), "vit_groups launch"))) return st;
        if ((st = run_viterbi_lanes(c, d_descs + cw0, d_groups, {n_groups, gather, u.in_rows, 0}, {}, n_groups * u.in_rows, n_groups * u.dec_rows, tie_rule,
                                    d_sched, u.mapping == DABGPU_VIT_MAP_OCTET, d_results + cw0, s, fic))) return st;
    }
    return DABGPU_OK;
}

// is the batch one puncturing schedule the lane mapping can take?
static bool uniform_batch(const dabgpu_codeword* h_cw, size_t n) {
    for (size_t i = 0; i < n; i++) {
        if (h_cw[i].flags & DABGPU_CW_DEPUNCTURED) return false;                                       // (mother-code sources: wave mapping only)
        if (h_cw[i].n_steps != h_cw[0].n_steps || memcmp(h_cw[i].seg_pi, h_cw[0].seg_pi, sizeof(h_cw[0].seg_pi)) ||
            memcmp(h_cw[i].seg_steps, h_cw[0].seg_steps, sizeof(h_cw[0].seg_steps))) return false;
        // the lane mapping keeps ring offsets in 32 bits
        if (h_cw[i].n_slots != 0 && !dabgpu_host_ring_fits_lanes(h_cw[i].n_slots, h_cw[i].cifs_per_frame, h_cw[i].frame_stride, h_cw[i].cif_stride))
            return false;
    }
    return true;
}

extern "C" int dabgpu_viterbi_decode_batch(dabgpu_ctx* c, const dabgpu_codeword* h_cw, size_t n, int tie_rule,
                                           dabgpu_codeword_result* d_results, void* stream) {
    if (!c || (!h_cw && n) || (!d_results && n)) { dabgpu_set_error("viterbi_decode_batch: null argument"); return DABGPU_ERR_INVALID_ARG; }
    if (n == 0) return DABGPU_OK;
    uint32_t max_steps = 0;
    for (size_t i = 0; i < n; i++) {
        int st = dabgpu_host_validate_codeword(h_cw[i], i);
        if (st) return st;
        max_steps = std::max(max_steps, h_cw[i].n_steps);
    }
    DABGPU_BIND(c);
    hipStream_t s = (hipStream_t)stream;
    dabgpu_cw_desc* d_descs = nullptr;
    int st = dabgpu_scratch(c, SCR_CW_DESCS, n * sizeof(dabgpu_cw_desc), (void**)&d_descs, s);
    if (st) return st;
    if ((st = dabgpu_stage_h2d(c, d_descs, h_cw, n * sizeof(dabgpu_cw_desc), s))) return st;
    // (h_cw is consumed when this returns, the caller may reuse it: small tables go through the pinned staging ring, large ones through
    // the runtime's pageable path -- or, when the caller's array is page-locked, a copy that is waited for; dabgpu_stage_h2d)
    if (uniform_batch(h_cw, n)) {
        const dabgpu_uniform_plan u = dabgpu_host_plan_uniform(n, max_steps, h_cw[0].seg_pi, h_cw[0].seg_steps, false, decode_limits(c));
        if (u.mapping != DABGPU_VIT_MAP_WAVE) return run_lanes_uniform(c, u, d_descs, n, max_steps, h_cw[0].seg_pi, h_cw[0].seg_steps, tie_rule, 0, d_results, s, false);
    }
    return dabgpu_run_viterbi(c, d_descs, n, max_steps, max_steps > 6 ? (max_steps - 6) / 8 : 0, tie_rule, d_results, s);
}

// given: the limits of the decode call this one is part of (nullptr: an entry point of its own)
static int fic_decode_any(dabgpu_ctx* c, const dabgpu_decode_limits* given, const int8_t* d_bits, size_t n_frames, size_t frame_stride,
                          const int32_t* d_slots, uint8_t* d_fib_bytes, dabgpu_codeword_result* d_results, int tie_rule, void* stream) {
    if (!c || !d_bits || !d_fib_bytes || !d_results) { dabgpu_set_error("fic_decode_frames: null argument"); return DABGPU_ERR_INVALID_ARG; }
    if (n_frames == 0) return DABGPU_OK;
    if (frame_stride < DABGPU_NB_FIC_BITS) { dabgpu_set_error("fic_decode_frames: frame_stride %zu < 9216", frame_stride); return DABGPU_ERR_INVALID_ARG; }
    DABGPU_BIND(c);
    hipStream_t s = (hipStream_t)stream;
    const size_t n = n_frames * 4;
    dabgpu_cw_desc* d_descs = nullptr;
    int st = dabgpu_scratch(c, scratch_fic<SCR_CW_DESCS>(true), n * sizeof(dabgpu_cw_desc), (void**)&d_descs, s);
    if (st) return st;
    st = dabgpu_check_hip(dabgpu_launch_fic_build(d_descs, d_bits, n_frames, frame_stride, d_fib_bytes, d_slots, s), "fic_build_descs launch");
    if (st) return st;
    // FIB groups are contiguous runs of 2304 soft bits; with 16-byte aligned frames the staged gather applies (mode 3)
    const int gather = rows_aligned(d_bits, frame_stride, 16) ? 3 : 0;
    const dabgpu_uniform_plan u = dabgpu_host_plan_fic(n, gather != 0, given ? *given : decode_limits(c));
    if (u.mapping == DABGPU_VIT_MAP_WAVE) return dabgpu_run_viterbi(c, d_descs, n, DABGPU_FIC_STEPS, DABGPU_FIC_OUT_BYTES, tie_rule, d_results, s, true);
    const uint32_t seg_pi[4] = DABGPU_FIC_SEG_PI, seg_steps[4] = DABGPU_FIC_SEG_STEPS;          // one schedule for every FIB group
    return run_lanes_uniform(c, u, d_descs, n, DABGPU_FIC_STEPS, seg_pi, seg_steps, tie_rule, gather, d_results, s, true);
}

extern "C" int dabgpu_fic_decode_frames(dabgpu_ctx* c, const int8_t* d_bits, size_t n_frames, size_t frame_stride,
                                        uint8_t* d_fib_bytes, dabgpu_codeword_result* d_results, int tie_rule, void* stream) {
    return fic_decode_any(c, nullptr, d_bits, n_frames, frame_stride, nullptr, d_fib_bytes, d_results, tie_rule, stream);
}

extern "C" int dabgpu_fic_decode_ring(dabgpu_ctx* c, const int8_t* d_hist, size_t n_ens, size_t ens_stride, const int32_t* d_newest_slot,
                                      uint8_t* d_fib_bytes, dabgpu_codeword_result* d_results, int tie_rule, void* stream) {
    if (!d_newest_slot) { dabgpu_set_error("fic_decode_ring: null slot array"); return DABGPU_ERR_INVALID_ARG; }
    return fic_decode_any(c, nullptr, d_hist, n_ens, ens_stride, d_newest_slot, d_fib_bytes, d_results, tie_rule, stream);
}

// what a decode call was given beside the multiplex: the ring of soft bits, where the results go
struct msc_request {
    const int8_t* d_hist; size_t ens_stride; int hist_frames, newest_frame_slot; const int32_t* d_slots;
    uint8_t* d_out; size_t out_ens_stride; dabgpu_codeword_result* d_results; int tie_rule, bits_layout;
    int classed() const { return bits_layout == DABGPU_BITS_MSC_CLASSED; }
    // the newest frames' soft bits (the ring form's slots live on the device: its FIC descriptors add them)
    const int8_t* newest_bits() const { return d_slots ? d_hist : d_hist + (size_t)newest_frame_slot * DABGPU_NB_FRAME_BITS; }
};
// fic: also decode the FIC of the newest frame of every ensemble (dabgpu_decode_frames_layout)
struct fic_request { uint8_t* d_fib_bytes; dabgpu_codeword_result* d_results; };

// the lane-mapped sub-channels of a planned call: lane table and schedules once, then per slice of ensembles groups + gather + trellis
static int run_msc_lanes(dabgpu_ctx* c, const dabgpu_decode_plan& p, const msc_request& r, const fic_request* fic, const dabgpu_cw_desc* d_descs,
                         const dabgpu_msc_plan* d_plans, hipStream_t s) {
    int st = ensure_vit_tables(c);
    if (st) return st;
    uint64_t* d_lane_subs = nullptr;
    uint2* d_sched = nullptr;
    if ((st = dabgpu_scratch(c, SCR_LANE_SUBS, p.lane_subs_bytes, (void**)&d_lane_subs, s))) return st;
    if ((st = dabgpu_stage_h2d_cached(c, 1, d_lane_subs, p.lane_subs.data(), p.lane_subs_bytes, s))) return st;
    // the schedule table of every lane-mapped sub-channel, once per call
    if ((st = dabgpu_scratch(c, SCR_VIT_SCHED, p.sched_bytes, (void**)&d_sched, s))) return st;
    if ((st = dabgpu_check_hip(dabgpu_launch_vit_sched_msc(d_sched, p.sched_stride, d_plans, d_lane_subs, p.n_lane, c->d_vit_tables, s), "vit_sched launch"))) return st;
    // the staged gathers read the ring rows in aligned 16-byte chunks (natural order) / aligned 64-byte lines (class order: whole memory
    // lines are loaded -- with the history and every ensemble 64-byte aligned no line reaches past the end of a row, 230400 = 3600 x 64)
    const int ring4 = r.classed() ? (rows_aligned(r.d_hist, r.ens_stride, 64) ? 2 : 0) : (rows_aligned(r.d_hist, r.ens_stride, 16) ? 1 : 0);
    for (size_t e0 = 0; e0 < p.n_ens; e0 += p.ens_per_slice) {
        dabgpu_decode_slice sl = dabgpu_host_decode_slice(p, e0);
        dabgpu_vit_group* d_groups = nullptr;
        if ((st = dabgpu_scratch(c, SCR_VIT_GROUPS, sl.groups_bytes, (void**)&d_groups, s))) return st;
        if ((st = dabgpu_check_hip(dabgpu_launch_vit_groups_msc(d_groups, d_plans, d_lane_subs, p.n_lane, p.n_sub, sl.ne, sl.gps, p.sched_stride, s), "vit_groups launch"))) return st;
        lane_groups fib = {};
        if (sl.n_fic_groups) {      // the FIB groups of the newest frames behind the MSC's groups, results into the caller's FIC array
            const uint32_t fic_pi[4] = DABGPU_FIC_SEG_PI, fic_steps[4] = DABGPU_FIC_SEG_STEPS;
            if ((st = dabgpu_check_hip(dabgpu_launch_vit_sched_uniform(d_sched + sl.fic_base.sched_off, p.fic_dec_rows, fic_pi, fic_steps, c->d_vit_tables, s), "vit_sched launch"))) return st;
            sl.fic_base.res_delta = (int64_t)(reinterpret_cast<const char*>(fic->d_results) - reinterpret_cast<const char*>(r.d_results + p.n_cw));
            if ((st = dabgpu_check_hip(dabgpu_launch_vit_groups_uniform_at(d_groups + sl.n_groups, p.n_fic_cw, DABGPU_FIC_STEPS, fic_pi, fic_steps, sl.fic_base, s), "vit_groups launch"))) return st;
            // FIB groups are contiguous runs of 2304 soft bits; with 16-byte aligned frames the staged gather applies
            fib = {sl.n_fic_groups, rows_aligned(r.newest_bits(), r.ens_stride, 16) ? 3 : 0, p.fic_in_rows, 0};
        }
        if ((st = run_viterbi_lanes(c, d_descs + sl.cw0, d_groups, {sl.n_groups, ring4, p.lane_max_in_rows, sl.gps}, fib, sl.sym_rows, sl.dec_rows, r.tie_rule,
                                    d_sched, p.octet, r.d_results + sl.cw0, s, false))) return st;
    }
    return DABGPU_OK;
}

// check the arguments, read the limits, plan (dabgpu_host_plan_decode), launch what the plan says
static int msc_decode_any(dabgpu_ctx* c, const int8_t* d_hist, size_t n_ens, size_t ens_stride, int hist_frames,
                          int newest_frame_slot, const int32_t* d_slots, const dabgpu_subchannel* h_sub, int n_sub, uint8_t* d_out,
                          size_t out_ens_stride, dabgpu_codeword_result* d_results, int tie_rule, void* stream,
                          int bits_layout = DABGPU_BITS_NATURAL, const fic_request* fic = nullptr) {
    const msc_request r = {d_hist, ens_stride, hist_frames, newest_frame_slot, d_slots, d_out, out_ens_stride, d_results, tie_rule, bits_layout};
    if (!c || !r.d_hist || !h_sub || !r.d_out || !r.d_results) { dabgpu_set_error("msc_decode_frames: null argument"); return DABGPU_ERR_INVALID_ARG; }
    if (dabgpu_check_bits_layout("msc_decode_frames", r.bits_layout)) return DABGPU_ERR_INVALID_ARG;
    if (n_ens == 0 || n_sub == 0) return DABGPU_OK;
    if (r.hist_frames < 5 || r.newest_frame_slot < 0 || r.newest_frame_slot >= r.hist_frames || n_sub < 0) {
        dabgpu_set_error("msc_decode_frames: history_frames must be >= 5 (16 CIFs of delay + the 4 new ones) and 0 <= newest < history_frames");
        return DABGPU_ERR_INVALID_ARG;
    }
    const dabgpu_decode_limits lim = decode_limits(c);
    dabgpu_decode_plan p;
    int st = dabgpu_host_plan_decode(h_sub, n_sub, n_ens, r.hist_frames, fic != nullptr, lim, &p);
    if (st) return st;
    if (r.out_ens_stride < (size_t)4 * p.cif_out_bytes) {
        dabgpu_set_error("msc_decode_frames: out_ensemble_stride %zu < 4 x %u", r.out_ens_stride, p.cif_out_bytes); return DABGPU_ERR_INVALID_ARG;
    }
    DABGPU_BIND(c);
    hipStream_t s = (hipStream_t)stream;
    dabgpu_cw_desc* d_descs = nullptr;
    dabgpu_msc_plan* d_plans = nullptr;
    if ((st = dabgpu_scratch(c, SCR_CW_DESCS, p.descs_bytes, (void**)&d_descs, s))) return st;
    if ((st = dabgpu_scratch(c, SCR_MSC_PLANS, p.plans_bytes, (void**)&d_plans, s))) return st;
    const int8_t* fic_bits = r.newest_bits();
    // (first on the stream, in the FIC's own copies of the scratch slots, before the plans are staged and the descriptors built)
    if (p.fic == DABGPU_FIC_OWN_LAUNCH &&
        (st = fic_decode_any(c, &lim, fic_bits, n_ens, r.ens_stride, r.d_slots, fic->d_fib_bytes, fic->d_results, r.tie_rule, stream))) return st;
    if ((st = dabgpu_stage_h2d_cached(c, 0, d_plans, p.subs.data(), p.plans_bytes, s))) return st;
    // (the FIB groups' descriptors behind the sub-channels' when they join the sub-channels' trellis launch)
    if (p.fic == DABGPU_FIC_IN_LANES || p.fic == DABGPU_FIC_IN_WAVE)
        st = dabgpu_check_hip(dabgpu_launch_msc_fic_build(d_descs, r.d_hist, n_ens, r.ens_stride, r.hist_frames, r.newest_frame_slot, d_plans, n_sub, r.d_out,
                                                          r.out_ens_stride, (int)p.cif_out_bytes, r.d_slots, r.classed(), fic_bits, fic->d_fib_bytes, s), "msc_fic_build_descs launch");
    else
        st = dabgpu_check_hip(dabgpu_launch_msc_build(d_descs, r.d_hist, n_ens, r.ens_stride, r.hist_frames, r.newest_frame_slot, d_plans, n_sub, r.d_out,
                                                      r.out_ens_stride, (int)p.cif_out_bytes, r.d_slots, r.classed(), s), "msc_build_descs launch");
    if (st) return st;
    if (p.n_lane > 0 && (st = run_msc_lanes(c, p, r, fic, d_descs, d_plans, s))) return st;
    if (p.k_wave == 0) return DABGPU_OK;
    if (p.fic == DABGPU_FIC_IN_WAVE)        // the FIB groups ride in the sub-channels' launch as codewords n_cw .. with their own result array
        return dabgpu_run_viterbi(c, d_descs, p.n_cw + p.n_fic_cw, p.max_steps, p.max_out_bytes, r.tie_rule, r.d_results, s, false, p.n_cw, fic->d_results);
    return dabgpu_run_viterbi(c, d_descs, p.n_cw, p.max_steps, p.max_out_bytes, r.tie_rule, r.d_results, s);
}

// which mapping dabgpu_msc_decode_frames* / dabgpu_decode_frames_layout take for this multiplex and batch right now (the context's setting, or
// the cost model's choice under DABGPU_VIT_MAP_AUTO), and what the model expects of each
extern "C" int dabgpu_multiplex_mapping(dabgpu_ctx* c, size_t n_ens, const dabgpu_subchannel* h_sub, int n_sub, int* mapping, double* model_us3) {
    if (!c || !h_sub || n_sub <= 0 || !mapping) { dabgpu_set_error("multiplex_mapping: null argument"); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_decode_plan p;       // (the shortest history there is: this call does not know the ring, whose size can only rule the batch mappings out)
    const int pst = dabgpu_host_plan_decode(h_sub, n_sub, n_ens, 5, false, decode_limits(c), &p);
    if (pst) return pst;
    *mapping = p.mapping;
    if (model_us3) memcpy(model_us3, p.model_us, sizeof(p.model_us));
    return DABGPU_OK;
}

extern "C" int dabgpu_msc_decode_frames(dabgpu_ctx* c, const int8_t* d_hist, size_t n_ens, size_t ens_stride, int hist_frames,
                                        int newest_frame_slot, const dabgpu_subchannel* h_sub, int n_sub, uint8_t* d_out,
                                        size_t out_ens_stride, dabgpu_codeword_result* d_results, int tie_rule, void* stream) {
    return msc_decode_any(c, d_hist, n_ens, ens_stride, hist_frames, newest_frame_slot, nullptr, h_sub, n_sub, d_out, out_ens_stride,
                          d_results, tie_rule, stream);
}

extern "C" int dabgpu_msc_decode_frames_layout(dabgpu_ctx* c, const int8_t* d_hist, size_t n_ens, size_t ens_stride, int hist_frames,
                                               int newest_frame_slot, const dabgpu_subchannel* h_sub, int n_sub, uint8_t* d_out,
                                               size_t out_ens_stride, dabgpu_codeword_result* d_results, int tie_rule, int bits_layout,
                                               void* stream) {
    return msc_decode_any(c, d_hist, n_ens, ens_stride, hist_frames, newest_frame_slot, nullptr, h_sub, n_sub, d_out, out_ens_stride,
                          d_results, tie_rule, stream, bits_layout);
}

extern "C" int dabgpu_msc_decode_ring_layout(dabgpu_ctx* c, const int8_t* d_hist, size_t n_ens, size_t ens_stride, int hist_frames,
                                             const int32_t* d_newest_slot, const dabgpu_subchannel* h_sub, int n_sub, uint8_t* d_out,
                                             size_t out_ens_stride, dabgpu_codeword_result* d_results, int tie_rule, int bits_layout,
                                             void* stream) {
    if (!d_newest_slot) { dabgpu_set_error("msc_decode_ring: null slot array"); return DABGPU_ERR_INVALID_ARG; }
    return msc_decode_any(c, d_hist, n_ens, ens_stride, hist_frames, 0, d_newest_slot, h_sub, n_sub, d_out, out_ens_stride, d_results,
                          tie_rule, stream, bits_layout);
}

// FIC + MSC of one transmission frame of every ensemble in one call (what BasicRadio::Process fans out to its FIC runner and MSC
// runners, src/basic_radio/basic_radio.cpp:41-65)
extern "C" int dabgpu_decode_frames_layout(dabgpu_ctx* c, const int8_t* d_hist, size_t n_ens, size_t ens_stride, int hist_frames,
                                           int newest_frame_slot, const dabgpu_subchannel* h_sub, int n_sub, uint8_t* d_fib_bytes,
                                           dabgpu_codeword_result* d_fic_results, uint8_t* d_msc_out, size_t out_ens_stride,
                                           dabgpu_codeword_result* d_msc_results, int tie_rule, int bits_layout, void* stream) {
    if (!c || !d_hist || !d_fib_bytes || !d_fic_results) { dabgpu_set_error("decode_frames: null argument"); return DABGPU_ERR_INVALID_ARG; }
    if (ens_stride < DABGPU_NB_FIC_BITS) { dabgpu_set_error("decode_frames: ensemble_stride %zu < 9216", ens_stride); return DABGPU_ERR_INVALID_ARG; }
    if (n_ens == 0) return DABGPU_OK;
    if (hist_frames < 1 || newest_frame_slot < 0 || newest_frame_slot >= hist_frames) {
        dabgpu_set_error("decode_frames: 0 <= newest_frame_slot < history_frames"); return DABGPU_ERR_INVALID_ARG;
    }
    if (n_sub == 0)       // nothing but the FIC
        return dabgpu_fic_decode_frames(c, d_hist + (size_t)newest_frame_slot * DABGPU_NB_FRAME_BITS, n_ens, ens_stride, d_fib_bytes, d_fic_results, tie_rule, stream);
    const fic_request fic = {d_fib_bytes, d_fic_results};
    return msc_decode_any(c, d_hist, n_ens, ens_stride, hist_frames, newest_frame_slot, nullptr, h_sub, n_sub, d_msc_out, out_ens_stride,
                          d_msc_results, tie_rule, stream, bits_layout, &fic);
}

extern "C" int dabgpu_decode_ring_layout(dabgpu_ctx* c, const int8_t* d_hist, size_t n_ens, size_t ens_stride, int hist_frames,
                                         const int32_t* d_newest_slot, const dabgpu_subchannel* h_sub, int n_sub, uint8_t* d_fib_bytes,
                                         dabgpu_codeword_result* d_fic_results, uint8_t* d_msc_out, size_t out_ens_stride,
                                         dabgpu_codeword_result* d_msc_results, int tie_rule, int bits_layout, void* stream) {
    if (!c || !d_hist || !d_fib_bytes || !d_fic_results || !d_newest_slot) { dabgpu_set_error("decode_ring: null argument"); return DABGPU_ERR_INVALID_ARG; }
    if (ens_stride < DABGPU_NB_FIC_BITS) { dabgpu_set_error("decode_ring: ensemble_stride %zu < 9216", ens_stride); return DABGPU_ERR_INVALID_ARG; }
    if (n_ens == 0) return DABGPU_OK;
    if (n_sub == 0) return dabgpu_fic_decode_ring(c, d_hist, n_ens, ens_stride, d_newest_slot, d_fib_bytes, d_fic_results, tie_rule, stream);
    const fic_request fic = {d_fib_bytes, d_fic_results};
    return msc_decode_any(c, d_hist, n_ens, ens_stride, hist_frames, 0, d_newest_slot, h_sub, n_sub, d_msc_out, out_ens_stride, d_msc_results,
                          tie_rule, stream, bits_layout, &fic);
}

extern "C" int dabgpu_msc_decode_ring(dabgpu_ctx* c, const int8_t* d_hist, size_t n_ens, size_t ens_stride, int hist_frames,
                                      const int32_t* d_newest_slot, const dabgpu_subchannel* h_sub, int n_sub, uint8_t* d_out,
                                      size_t out_ens_stride, dabgpu_codeword_result* d_results, int tie_rule, void* stream) {
    return dabgpu_msc_decode_ring_layout(c, d_hist, n_ens, ens_stride, hist_frames, d_newest_slot, h_sub, n_sub, d_out, out_ens_stride,
                                         d_results, tie_rule, DABGPU_BITS_NATURAL, stream);
}
