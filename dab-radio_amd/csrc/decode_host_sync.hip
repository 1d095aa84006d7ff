// decode_host_sync.hip -- single-codeword host-buffer forms of the channel decoder and dabgpu_msc_stream (include/dabgpu.h): what the C++
// mirror classes call once per FIB group / CIF.  Host side only; the arithmetic is in viterbi.hip.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <vector>

#include "dabgpu.h"
#include "dabgpu_internal.h"

// ------------------------------------------------------------------------------------------------
// single-stream host-buffer forms (C++ mirror classes)
// ------------------------------------------------------------------------------------------------
static int decode_one_sync(dabgpu_ctx* c, dabgpu_cw_desc D, const int8_t* h_src, size_t n_src, uint8_t* h_out, size_t n_out,
                           dabgpu_codeword_result* h_res, int tie_rule) {
    DABGPU_BIND(c);
    int st;
    int8_t* d_src = nullptr; uint8_t* d_out; dabgpu_codeword_result* d_res; dabgpu_cw_desc* d_desc;
    if (h_src && (st = dabgpu_scratch(c, SCR_CW_SRC, n_src, (void**)&d_src))) return st;
    // (the kernel writes (n_steps - 6) / 8 bytes whatever part of them the caller wants back)
    const size_t kernel_out = D.n_steps > 6 ? (size_t)(D.n_steps - 6) / 8 : 0;
    if ((st = dabgpu_scratch(c, SCR_CW_OUT, std::max<size_t>(std::max(n_out, kernel_out), 16), (void**)&d_out))) return st;
    if ((st = dabgpu_scratch(c, SCR_CW_RESULT, sizeof(dabgpu_codeword_result), (void**)&d_res))) return st;
    if ((st = dabgpu_scratch(c, SCR_CW_DESCS, sizeof(dabgpu_cw_desc), (void**)&d_desc))) return st;
    hipStream_t s = c->stream;
    if (h_src) D.d_src = (uint64_t)(uintptr_t)d_src;
    D.d_out = (uint64_t)(uintptr_t)d_out;
    if ((st = dabgpu_host_validate_codeword(D, 0))) return st;
    if (h_src) DABGPU_CK(hipMemcpyAsync(d_src, h_src, n_src, hipMemcpyHostToDevice, s));
    DABGPU_CK(hipMemcpyAsync(d_desc, &D, sizeof(D), hipMemcpyHostToDevice, s));
    if ((st = dabgpu_run_viterbi(c, d_desc, 1, D.n_steps, D.n_steps > 6 ? (D.n_steps - 6) / 8 : 0, tie_rule, d_res, s))) return st;
    if (n_out) DABGPU_CK(hipMemcpyAsync(h_out, d_out, n_out, hipMemcpyDeviceToHost, s));
    DABGPU_CK(hipMemcpyAsync(h_res, d_res, sizeof(*h_res), hipMemcpyDeviceToHost, s));
    DABGPU_CK(hipStreamSynchronize(s));
    return DABGPU_OK;
}

extern "C" int dabgpu_fic_decode_group_host_sync(dabgpu_ctx* c, const int8_t* h_bits, uint8_t* h_bytes, uint32_t* crc_ok_mask,
                                                 uint64_t* path_error, int tie_rule) {
    if (!c || !h_bits || !h_bytes) { dabgpu_set_error("fic_decode_group_host_sync: null argument"); return DABGPU_ERR_INVALID_ARG; }
    DABGPU_HOST_LOCK(c);
    dabgpu_cw_desc D = {};
    dabgpu_cw_set_fic(&D);
    D.d_src = 1;    // placeholder, replaced by the staging buffer
    dabgpu_codeword_result R;
    const int st = decode_one_sync(c, D, h_bits, DABGPU_NB_FIB_GROUP_BITS, h_bytes, DABGPU_FIC_OUT_BYTES, &R, tie_rule);
    if (st) return st;
    if (crc_ok_mask) *crc_ok_mask = R.crc_ok_mask;
    if (path_error) *path_error = R.path_error;
    return DABGPU_OK;
}

extern "C" int dabgpu_viterbi_decode_host_sync(dabgpu_ctx* c, const int8_t* h_src, size_t n_src, const uint32_t* seg_pi,
                                               const uint32_t* seg_steps, uint32_t start_state, uint32_t end_state, uint32_t flags,
                                               uint8_t* h_out, size_t n_out_bytes, uint64_t* path_error, int tie_rule) {
    if (!c || !h_src || !seg_pi || !seg_steps || !h_out) { dabgpu_set_error("viterbi_decode_host_sync: null argument"); return DABGPU_ERR_INVALID_ARG; }
    DABGPU_HOST_LOCK(c);
    dabgpu_cw_desc D = {};
    dabgpu_cw_set_segments(&D, seg_pi, seg_steps);
    const uint32_t steps = D.n_steps - 6;
    size_t need = 12;
    for (int k = 0; k < 4; k++) need += (size_t)(seg_steps[k] / 8) * (8 + seg_pi[k]);
    D.start_state = start_state; D.end_state = end_state; D.flags = flags;
    D.d_src = 1;
    if (n_src < need || n_out_bytes * 8 != steps) {
        dabgpu_set_error("viterbi_decode_host_sync: %zu soft bits given, %zu needed; %zu output bytes for %u information bits", n_src, need, n_out_bytes, steps);
        return DABGPU_ERR_INVALID_ARG;
    }
    dabgpu_codeword_result R;
    const int st = decode_one_sync(c, D, h_src, need, h_out, n_out_bytes, &R, tie_rule);
    if (st) return st;
    if (path_error) *path_error = R.path_error;
    return DABGPU_OK;
}

extern "C" int dabgpu_viterbi_decode_depunctured_host_sync(dabgpu_ctx* c, const int8_t* h_mother, size_t n_steps, uint32_t start_state,
                                                           uint32_t end_state, uint8_t* h_out, size_t n_out_bytes, uint64_t* path_error, int tie_rule) {
    if (!c || !h_mother || (!h_out && n_out_bytes)) { dabgpu_set_error("viterbi_decode_depunctured_host_sync: null argument"); return DABGPU_ERR_INVALID_ARG; }
    if (n_steps < 1 || n_steps > DABGPU_MAX_TRELLIS_STEPS) {
        dabgpu_set_error("viterbi_decode_depunctured_host_sync: n_steps %zu out of range (1 .. %u)", n_steps, (unsigned)DABGPU_MAX_TRELLIS_STEPS);
        return DABGPU_ERR_INVALID_ARG;
    }
    if (n_out_bytes && n_out_bytes * 8 + 6 > n_steps) {
        dabgpu_set_error("viterbi_decode_depunctured_host_sync: a trace-back of %zu bytes starts at decision word %zu, only %zu steps were decoded",
                         n_out_bytes, n_out_bytes * 8 + 5, n_steps);
        return DABGPU_ERR_INVALID_ARG;
    }
    DABGPU_HOST_LOCK(c);
    dabgpu_cw_desc D = {};
    D.start_state = start_state; D.end_state = end_state; D.flags = DABGPU_CW_RAW | DABGPU_CW_DEPUNCTURED;
    D.d_src = 1;
    dabgpu_codeword_result R;
    // whole length: the path error (and the bytes, when the trace-back starts at the last step)
    const bool same = n_out_bytes * 8 + 6 == n_steps;
    D.n_steps = (uint32_t)n_steps;
    int st = decode_one_sync(c, D, h_mother, 4 * n_steps, h_out, same ? n_out_bytes : 0, &R, tie_rule);
    if (st) return st;
    if (path_error) *path_error = R.path_error;
    if (same || n_out_bytes == 0) return DABGPU_OK;
    // the trace-back starts earlier: decode the prefix that ends there (same decisions for its steps), from the same end state
    D.n_steps = (uint32_t)(n_out_bytes * 8 + 6);
    return decode_one_sync(c, D, h_mother, 4 * (size_t)D.n_steps, h_out, n_out_bytes, &R, tie_rule);
}

struct dabgpu_msc_stream {
    dabgpu_ctx* ctx;
    dabgpu_subchannel sc;
    dabgpu_cw_desc proto;       // plan with ring geometry, d_src = ring base
    dabgpu::DeviceBuffer<int8_t> d_ring;
    dabgpu::DeviceBuffer<int8_t> d_logical;
    int n_bits;
    int n_out_bytes;
    int next_slot;
    int stored;
    // Consume (push_cif) only files the CIF in this page-locked twin of the ring; a slot crosses to the device when a call that reads the
    // device ring comes (deinterleave_sync / decode_sync).  A decoder whose results come from its demodulator's frame session
    // (dab-radio_amd/host/dab/dabgpu_frame_batcher.h) never reads its own ring: its DecodeCIF then costs a 3 KB host copy, not a DMA.
    dabgpu::PinnedBuffer<int8_t> h_ring;
    uint32_t dirty;             // bit k: slot k of h_ring is newer than the device's
};

// the slots filed since the last device read, uploaded on the context's stream (the callers synchronise with it before they return, so
// h_ring is not overwritten under a copy in flight)
static int msc_stream_flush(dabgpu_msc_stream* s) {
    for (int k = 0; k < 16 && s->dirty; k++) {
        if (!(s->dirty >> k & 1u)) continue;
        const int st = dabgpu_check_hip(hipMemcpyAsync(s->d_ring.get() + (size_t)k * s->n_bits, s->h_ring.get() + (size_t)k * s->n_bits, (size_t)s->n_bits,
                                                       hipMemcpyHostToDevice, s->ctx->stream), "hipMemcpyAsync(msc stream ring)");
        if (st) return st;
        s->dirty &= ~(1u << k);
    }
    return DABGPU_OK;
}

extern "C" int dabgpu_msc_stream_create(dabgpu_ctx* c, const dabgpu_subchannel* sc, dabgpu_msc_stream** out) {
    if (!c || !sc || !out) return DABGPU_ERR_INVALID_ARG;
    *out = nullptr;
    int pi[4], lx[4], nb = 0;
    {   // the same checks as the batch decoders': a valid profile, inside the CIF, consuming no more soft bits than the sub-channel holds
        std::vector<dabgpu_msc_plan> one;
        const int pst = dabgpu_host_build_msc_plans(sc, 1, one, nullptr, nullptr, nullptr);
        if (pst) return pst;
    }
    if (dabgpu_subchannel_plan(sc, pi, lx, &nb) < 0) { dabgpu_set_error("msc_stream_create: invalid protection profile"); return DABGPU_ERR_INVALID_ARG; }
    DABGPU_BIND(c);
    dabgpu_msc_stream* s = new (std::nothrow) dabgpu_msc_stream();
    if (!s) return DABGPU_ERR_HIP;
    s->ctx = c; s->sc = *sc; s->n_bits = sc->length * 64; s->n_out_bytes = nb; s->next_slot = 0; s->stored = 0;
    s->dirty = 0;
    int st = s->d_ring.alloc((size_t)16 * s->n_bits, "hipMalloc(ring)");
    if (!st) st = s->h_ring.alloc((size_t)16 * s->n_bits, "hipHostMalloc(ring)");
    if (!st) st = s->d_logical.alloc((size_t)s->n_bits, "hipMalloc(logical)");
    // on the context's own stream and waited for: hipMemset runs on the NULL stream, with which a hipStreamNonBlocking stream does not synchronise -- a
    // ring uploaded right after creation (MSC_Decoder creates its stream on its first call-by-call decode) was overwritten by the late zeros
    if (!st) st = dabgpu_check_hip(hipMemsetAsync(s->d_ring.get(), 0, (size_t)16 * s->n_bits, c->stream), "hipMemsetAsync(ring)");
    if (!st) st = dabgpu_check_hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize(ring)");
    if (st) { dabgpu_msc_stream_destroy(s); return st; }
    dabgpu_cw_desc& D = s->proto;
    D = dabgpu_cw_desc{};
    const uint32_t seg_pi[4] = {(uint32_t)pi[0], (uint32_t)pi[1], (uint32_t)pi[2], (uint32_t)pi[3]};
    const uint32_t seg_steps[4] = {32u * (uint32_t)lx[0], 32u * (uint32_t)lx[1], 32u * (uint32_t)lx[2], 32u * (uint32_t)lx[3]};
    dabgpu_cw_set_segments(&D, seg_pi, seg_steps);
    D.d_src = (uint64_t)(uintptr_t)s->d_ring.get();
    D.n_slots = 16; D.cifs_per_frame = 1; D.frame_stride = (uint32_t)s->n_bits; D.cif_stride = 0;
    *out = s;
    return DABGPU_OK;
}

extern "C" void dabgpu_msc_stream_destroy(dabgpu_msc_stream* s) {
    if (!dabgpu_destroy_begin(s, s ? s->ctx : nullptr, false)) return;
    if (s->h_ring) (void)hipStreamSynchronize(s->ctx->stream);         // (an upload of the ring's twin may be in flight)
    delete s;
}

extern "C" int dabgpu_msc_stream_push_cif(dabgpu_msc_stream* s, const int8_t* h_bits) {
    if (!s || !h_bits) return DABGPU_ERR_INVALID_ARG;
    DABGPU_HOST_LOCK(s->ctx);
    // copied here and now: the caller's span is only valid during DecodeCIF (SURVEY 8b ownership)
    memcpy(s->h_ring.get() + (size_t)s->next_slot * s->n_bits, h_bits, (size_t)s->n_bits);
    s->dirty |= 1u << s->next_slot;
    s->next_slot = (s->next_slot + 1) % 16;                    // cif_deinterleaver.cpp:28-33
    if (s->stored < 16) s->stored++;
    return DABGPU_OK;
}

extern "C" int dabgpu_msc_stream_deinterleave_sync(dabgpu_msc_stream* s, int8_t* h_out) {
    if (!s || !h_out) return DABGPU_ERR_INVALID_ARG;
    DABGPU_HOST_LOCK(s->ctx);
    if (s->stored < 16) return DABGPU_ERR_NOT_READY;           // cif_deinterleaver.cpp:40-42
    DABGPU_BIND(s->ctx);
    hipStream_t q = s->ctx->stream;
    int st = msc_stream_flush(s);
    if (!st) st = dabgpu_check_hip(dabgpu_launch_cif_deinterleave(s->d_ring.get(), s->n_bits, 16, (s->next_slot + 15) % 16, s->d_logical.get(), q),
                              "cif_deinterleave launch");
    if (!st) st = dabgpu_check_hip(hipMemcpyAsync(h_out, s->d_logical.get(), (size_t)s->n_bits, hipMemcpyDeviceToHost, q), "hipMemcpyAsync");
    if (!st) st = dabgpu_check_hip(hipStreamSynchronize(q), "hipStreamSynchronize");
    return st;
}

extern "C" int dabgpu_msc_stream_decode_sync(dabgpu_msc_stream* s, uint8_t* h_out, size_t* n_out, uint64_t* path_error, int tie_rule) {
    if (!s || !h_out || !n_out) return DABGPU_ERR_INVALID_ARG;
    DABGPU_HOST_LOCK(s->ctx);
    *n_out = 0;
    if (s->stored < 16) return DABGPU_ERR_NOT_READY;           // msc_decoder.cpp:60-63
    DABGPU_BIND(s->ctx);
    const int fst = msc_stream_flush(s);
    if (fst) return fst;
    dabgpu_cw_desc D = s->proto;
    D.newest_slot = (uint32_t)((s->next_slot + 15) % 16);
    dabgpu_codeword_result R;
    const int st = decode_one_sync(s->ctx, D, nullptr, 0, h_out, (size_t)s->n_out_bytes, &R, tie_rule);
    if (st) return st;
    *n_out = (size_t)s->n_out_bytes;
    if (path_error) *path_error = R.path_error;
    return DABGPU_OK;
}
