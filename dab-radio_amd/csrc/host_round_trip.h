// host_round_trip.h -- the single-frame host forms of the per-frame estimators (noise.hip, noise_profile.hip, dd_profile.hip,
// sym_profile.hip, clock.hip), behind each entry point's own argument check: one frame's payload to a scratch slot, the optional inputs
// into one block of small words in SCR_HOST_FREQ, the entry point's launch, the optional outputs back, all on the context's stream,
// which is waited for once.  The layout of the block and the launch stay with the entry point (signal_bank.h is the same move for the
// banks of the signal path).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "dabgpu.h"
#include "dabgpu_internal.h"

namespace dabgpu {

// HOST_LATE: an output that reaches the caller behind the synchronise (the scalars: mean, valid, the slope).  All late fields of a call,
// given or not, come back in ONE copy, from the first one's first word to the last one's last, into a local
constexpr unsigned HOST_IN = 1u, HOST_OUT = 2u, HOST_LATE = 4u, HOST_LATE_WORDS = 8u;
// `words` 32-bit words at word `at` of the block; host: the caller's pointer, NULL: not given (nothing of it is copied either way)
struct HostField { size_t at, words; void* host; unsigned dir; };
// the payload goes up whole; back (NULL: no) receives it again behind the launch, in front of the fields
struct HostPayload { dabgpu_scratch_slot slot; const void* host; size_t bytes; void* back; };

// launch(d_payload, d_small, s): the entry point's own launches on what is on the device; who names the entry point in a runtime failure
template <size_t N, class Launch>
int host_round_trip(dabgpu_ctx* c, const char* who, const HostPayload& p, size_t small_words, const HostField (&fields)[N], Launch launch) {
    DABGPU_BIND(c);
    DABGPU_HOST_LOCK(c);
    int st;
    hipStream_t s = c->stream;
    auto ck = [&](hipError_t e, const char* what) {
        if (e != hipSuccess) dabgpu_set_error("%s: %s: %s", who, what, hipGetErrorString(e));
        return e == hipSuccess ? DABGPU_OK : DABGPU_ERR_HIP;
    };
    float *d_payload, *d_small;
    if ((st = dabgpu_scratch(c, p.slot, p.bytes, (void**)&d_payload))) return st;
    if ((st = dabgpu_scratch(c, SCR_HOST_FREQ, small_words * 4, (void**)&d_small))) return st;
    if ((st = ck(hipMemcpyAsync(d_payload, p.host, p.bytes, hipMemcpyHostToDevice, s), "payload to the device"))) return st;
    size_t late0 = small_words, late1 = 0;
    for (const HostField& f : fields) {
        if ((f.dir & HOST_IN) && f.host && (st = ck(hipMemcpyAsync(d_small + f.at, f.host, f.words * 4, hipMemcpyHostToDevice, s), "input to the device")))
            return st;
        if (f.dir & HOST_LATE) { late0 = f.at < late0 ? f.at : late0; late1 = f.at + f.words > late1 ? f.at + f.words : late1; }
    }
    if ((st = launch(d_payload, d_small, s))) return st;
    if (p.back && (st = ck(hipMemcpyAsync(p.back, d_payload, p.bytes, hipMemcpyDeviceToHost, s), "payload to the host"))) return st;
    for (const HostField& f : fields)
        if ((f.dir & (HOST_OUT | HOST_LATE)) == HOST_OUT && f.host &&
            (st = ck(hipMemcpyAsync(f.host, d_small + f.at, f.words * 4, hipMemcpyDeviceToHost, s), "output to the host")))
            return st;
    uint32_t late[HOST_LATE_WORDS];
    if (late1 > late0 + HOST_LATE_WORDS) { dabgpu_set_error("%s: %zu late words", who, late1 - late0); return DABGPU_ERR_INVALID_ARG; }
    if (late1 > late0 && (st = ck(hipMemcpyAsync(late, d_small + late0, (late1 - late0) * 4, hipMemcpyDeviceToHost, s), "scalars to the host"))) return st;
    if ((st = ck(hipStreamSynchronize(s), "hipStreamSynchronize"))) return st;
    for (const HostField& f : fields)
        if ((f.dir & HOST_LATE) && f.host) memcpy(f.host, late + (f.at - late0), f.words * 4);
    return DABGPU_OK;
}

}  // namespace dabgpu
