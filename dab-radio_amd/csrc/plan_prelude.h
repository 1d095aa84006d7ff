// plan_prelude.h -- the checks that the per-frame estimators' planners (dabgpu_noise_plan, _noise_profile_plan, _dd_profile_plan,
// _sym_profile_plan, _clock_estimate_plan, _clock_derotate_plan in dabgpu_host_logic.cpp), the TII bank's process call and the NULL-window
// host forms share.  Plain C++ (no HIP header).  Each takes `who`, the entry point's name as the refusal words it, and returns DABGPU_OK
// or DABGPU_ERR_INVALID_ARG with the reason set; a planner chains them with || in the order its header documents (the first refusal ends
// the chain) and adds its own rules between.
#pragma once
#include "dabgpu_host_logic.h"
#include "tii_core.h"

namespace dabgpu {

template <class... P> inline uintptr_t plan_or(const P*... p) { return (uintptr_t(0) | ... | (uintptr_t)p); }

// the opening of every planner: a result to write, cleared; mode I; 1 .. 2^24 frames
template <class Geometry> inline int plan_open(const char* who, Geometry* out, int transmission_mode, size_t n_frames) {
    if (!out) { dabgpu_set_error("%s: null result", who); return DABGPU_ERR_INVALID_ARG; }
    *out = Geometry{};                                        // a refusal leaves no geometry behind
    if (transmission_mode != 1) { dabgpu_set_error("%s: transmission mode %d (mode I only)", who, transmission_mode); return DABGPU_ERR_INVALID_ARG; }
    if (n_frames == 0 || n_frames > ((size_t)1 << 24)) { dabgpu_set_error("%s: n_frames %zu outside 1 .. 16777216", who, n_frames); return DABGPU_ERR_INVALID_ARG; }
    return DABGPU_OK;
}
// bits = plan_or of one pointer or several (NULL passes); nouns = the list as the caller words it ("records, offsets and outputs")
inline int plan_aligned(const char* who, uintptr_t bits, unsigned align, const char* nouns) {
    if (bits & (align - 1)) { dabgpu_set_error("%s: %s must be %u-byte aligned", who, nouns, align); return DABGPU_ERR_INVALID_ARG; }
    return DABGPU_OK;
}
// a required input (bits = 0: missing): noun = what is missing ("samples"), name = what is misaligned ("d_iq")
inline int plan_input(const char* who, uintptr_t bits, unsigned align, const char* noun, const char* name) {
    if (!bits) { dabgpu_set_error("%s: null %s", who, noun); return DABGPU_ERR_INVALID_ARG; }
    return plan_aligned(who, bits, align, name);
}
// a stream's slice holds the NULL window (reach samples from null_offset) wherever a sync record may move it (+ 1543)
inline int plan_null_reach(const char* who, size_t stride, size_t null_offset, size_t reach, bool records) {
    if (records) reach += 1543u;
    if (null_offset > ((size_t)1 << 40) || stride > ((size_t)1 << 40) || stride < null_offset + reach) {
        dabgpu_set_error("%s: stream_stride_samples %zu does not hold null_offset_samples %zu + %zu", who, stride, null_offset, reach);
        return DABGPU_ERR_INVALID_ARG;
    }
    return DABGPU_OK;
}
// state that is read and written: the same buffer (in place) or two that do not overlap; either may be NULL
inline int plan_in_place(const char* who, const void* in, const void* out, uintptr_t bytes, const char* in_name, const char* out_name) {
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    if (a && b && a != b && a < b + bytes && b < a + bytes) {
        dabgpu_set_error("%s: %s and %s overlap without being the same buffer", who, in_name, out_name); return DABGPU_ERR_INVALID_ARG;
    }
    return DABGPU_OK;
}
// outputs = plan_or of every output
inline int plan_any_output(const char* who, uintptr_t outputs) {
    if (!outputs) { dabgpu_set_error("%s: no output at all", who); return DABGPU_ERR_INVALID_ARG; }
    return DABGPU_OK;
}
// the geometry of an accepted call: one workgroup per frame
inline int plan_per_frame(dabgpu_noise_geometry* out, size_t n_frames, uint32_t threads, uint32_t lds_bytes) {
    *out = dabgpu_noise_geometry{(uint32_t)n_frames, threads, lds_bytes};
    return DABGPU_OK;
}

// the single-frame host forms over a NULL window: the first sample that travels, null_offset + fine_time_offset + lead, when `reach`
// samples from there lie inside the caller's n_samples; else -1 with the refusal set.  what, leaves: the window as the entry point words it
// ("the NULL at", "leaves").  check_offset: the offset's own range first (the TII bank's host form takes any)
inline long long host_window_first(const char* who, size_t n_samples, size_t null_offset, int fine_time_offset, bool check_offset, int lead,
                                   size_t reach, const char* what, const char* leaves) {
    if (check_offset && !tii_time_offset_ok(fine_time_offset)) {
        dabgpu_set_error("%s: fine_time_offset %d outside -504 .. 1543", who, fine_time_offset); return -1;
    }
    const long long first = (null_offset > ((size_t)1 << 40)) ? -1 : (long long)null_offset + fine_time_offset + lead;
    if (n_samples > ((size_t)1 << 40) || first < 0 || (size_t)first + reach > n_samples) {
        dabgpu_set_error("%s: %s null_offset_samples %zu + fine_time_offset %d %s the %zu samples", who, what, null_offset, fine_time_offset, leaves,
                         n_samples);
        return -1;
    }
    return first;
}

}  // namespace dabgpu
