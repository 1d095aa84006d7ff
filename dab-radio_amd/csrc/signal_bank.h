// signal_bank.h -- what the banks of the signal path (channel.hip, resample.hip, channelise.hip) share on the host: the position word on the
// device, the grow-only buffers of the host forms and the host round trip itself.  The kernels and their dispatch stay with each bank.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dabgpu.h"
#include "dabgpu_internal.h"

namespace dabgpu {

// the base of dabgpu_channel_bank, dabgpu_resample_bank and dabgpu_channeliser_bank
struct SignalBank {
    dabgpu_ctx* ctx = nullptr;
    DeviceBuffer<> d_mem;                       // one allocation: position (16 bytes) | the bank's own payload
    uint64_t* d_pos = nullptr;                  // (into d_mem)
    DeviceBuffer<> buf[2];                      // host form: [0] input, [1] output (grow only)
};

// d_mem = 16 + payload_bytes, the position zeroed on the context's stream; *payload = byte 16, for the bank to lay out.  label names the
// bank in a failure ("channel": "hipMalloc(channel bank)")
int sb_alloc(SignalBank* b, size_t payload_bytes, const char* label, uint8_t** payload);
// behind the work kernel on the same stream: the next call (or graph replay) continues where this one ended
void sb_enqueue_advance(uint64_t* d_pos, size_t n_out, hipStream_t s);
// who = the entry point's name, cap_text = the cap as the refusal words it ("2^62")
int sb_seek(SignalBank* b, const char* who, uint64_t position, uint64_t cap, const char* cap_text, void* stream);
// the host form behind an entry point's argument check: the rows to the buffers (input rows an even count apart, output rows a multiple of
// 16 bytes apart, zeroed first on request), the launch, the rows back, all on the context's stream, which is waited for.
// launch(d_in, d_in_stride, d_out, d_out_stride, s): the bank's own launch (work kernel, advance) on rows that are on the device
template <class Launch>
int sb_host_round_trip(SignalBank* b, size_t in_rows, size_t out_rows, bool zero_out, const float* h_in, size_t in_stride_samples, size_t n_in,
                       size_t n_out, void* h_out, int out_format, size_t out_stride_bytes, Launch launch) {
    int st;
    dabgpu_ctx* c = b->ctx;
    DABGPU_BIND(c);
    DABGPU_HOST_LOCK(c);
    hipStream_t s = c->stream;
    const size_t row_bytes = n_out * (out_format == DABGPU_IQ_RAW_F32L ? 8 : 2), d_out_stride = (row_bytes + 15) & ~(size_t)15;
    const size_t d_in_stride = in_stride_samples ? (n_in + 1) & ~(size_t)1 : 0, n_rows = in_stride_samples ? in_rows : 1;
    const size_t need[2] = {(n_rows * (d_in_stride ? d_in_stride : n_in)) * 8, out_rows * d_out_stride};
    for (int k = 0; k < 2; k++)
        if (b->buf[k].needs(need[k])) {             // one that is too small is freed behind a hipDeviceSynchronize and allocated anew
            if (b->buf[k]) DABGPU_CK(hipDeviceSynchronize());
            if ((st = b->buf[k].regrow(need[k], "hipMalloc(&b->buf[which], bytes)"))) return st;
        }
    void *d_in = b->buf[0].get(), *d_out = b->buf[1].get();
    DABGPU_CK(hipMemcpy2DAsync(d_in, (d_in_stride ? d_in_stride : n_in) * 8, h_in, (in_stride_samples ? in_stride_samples : n_in) * 8, n_in * 8, n_rows,
                               hipMemcpyHostToDevice, s));
    if (zero_out) DABGPU_CK(hipMemsetAsync(d_out, 0, out_rows * d_out_stride, s));
    if ((st = launch(static_cast<const float*>(d_in), d_in_stride, d_out, d_out_stride, s))) return st;
    DABGPU_CK(hipMemcpy2DAsync(h_out, out_stride_bytes, d_out, d_out_stride, row_bytes, out_rows, hipMemcpyDeviceToHost, s));   // the rows only
    DABGPU_CK(hipStreamSynchronize(s));
    return DABGPU_OK;
}

}  // namespace dabgpu
