// signal_bank.hip -- see signal_bank.h
#include "signal_bank.h"

#include <stdio.h>

namespace dabgpu {

__global__ void signal_advance_kernel(uint64_t* pos, uint64_t n) { *pos += n; }

void sb_enqueue_advance(uint64_t* d_pos, size_t n_out, hipStream_t s) {
    hipLaunchKernelGGL(signal_advance_kernel, dim3(1), dim3(1), 0, s, d_pos, (uint64_t)n_out);
}

int sb_alloc(SignalBank* b, size_t payload_bytes, const char* label, uint8_t** payload) {
    char what[64];
    snprintf(what, sizeof(what), "hipMalloc(%s bank)", label);
    int st = b->d_mem.alloc(16 + payload_bytes, what);
    if (st) return st;
    b->d_pos = static_cast<uint64_t*>(b->d_mem.get());
    *payload = static_cast<uint8_t*>(b->d_mem.get()) + 16;
    snprintf(what, sizeof(what), "hipMemsetAsync(%s position)", label);
    return dabgpu_check_hip(hipMemsetAsync(b->d_pos, 0, 16, b->ctx->stream), what);
}

int sb_seek(SignalBank* b, const char* who, uint64_t position, uint64_t cap, const char* cap_text, void* stream) {
    if (!b) { dabgpu_set_error("%s: null bank", who); return DABGPU_ERR_INVALID_ARG; }
    if (position > cap) { dabgpu_set_error("%s: position above %s", who, cap_text); return DABGPU_ERR_INVALID_ARG; }
    DABGPU_BIND(b->ctx);
    return dabgpu_stage_h2d(b->ctx, b->d_pos, &position, sizeof(position), (hipStream_t)stream);
}

}  // namespace dabgpu
