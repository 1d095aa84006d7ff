// dab_encode.hip -- channel encoder bank (include/dabgpu.h, "Channel encoder"): FIB bodies and sub-channel bytes of n ensembles ->
// the frames' hard bits in the layout the modulator reads.  ETSI EN 300 401 5.2.1, 10, 11, 12 in the transmit direction.
//
// One workgroup per (ensemble, sub-channel), one more per ensemble for the FIC and the capacity units nobody occupies; each walks the
// call's frames in order.  Per frame a sub-channel's workgroup
//   1. encodes its four logical frames into LDS, one thread per 32 input bits (dab_encode_core.h): the four generator outputs are
//      shift-and-XOR of a 64-bit window over the scrambled data, each run of 32 mother bits is punctured with the schedule entry's
//      keep mask and OR-ed into the code word at the entry's bit offset;
//   2. emits the frame's four CIFs for its own bit range: the 16 class rows of ring slot (CIF mod 16) are read, transposed to natural
//      order, and the classes whose delay does not reach back beyond this frame are taken from LDS instead;
//   3. files what later frames will send: logical frame q's class c row goes to ring slot (CIF + delay(c)) mod 16.
// The ring holds partly filled TRANSMITTED CIFs in class order, bit i of a sub-channel at row i % 16, position i / 16 -- the transmit
// twin of DABGPU_BITS_MSC_CLASSED, per sub-channel because a capacity unit is only 4 bits of a class row.  Every (slot, row) is written
// once per 16 CIFs by plain stores and read once: 6912 B each way per full CIF.  Sub-channels start on multiples of 64 bits, so the
// class of a bit is the same in the sub-channel and in the CIF, and no workgroup ever touches another's rows or output bytes.
// The frame counter (which slot is "now") is read from device memory and advanced by a second, one-thread kernel: a captured call
// replays onto the following frames.
#include <hip/hip_runtime.h>
#include <string.h>
#include <new>

#include "dab_encode_core.h"
#include "dabgpu_internal.h"

namespace dabgpu {

#define TX_FIC_BYTES (DABGPU_NB_FIC_BITS / 8)               // 1152
#define TX_CIF_BYTES (DABGPU_NB_CIF_BITS / 8)               // 6912
#define TX_FRAME_BYTES (DABGPU_NB_FRAME_BITS / 8)           // 28800

__global__ __launch_bounds__(256)
void tx_encode_kernel(const dabgpu_tx_sub_plan* __restrict__ subs, const dabgpu_tx_sched_entry* __restrict__ sched, const uint32_t* __restrict__ gaps,
                      int n_gaps, const uint32_t* __restrict__ prbs, int n_sub, uint32_t n_frames, uint32_t cif_in_bytes, uint32_t ring_slot_dwords,
                      const uint8_t* __restrict__ fib, const uint8_t* __restrict__ payload, uint32_t* ring, const uint32_t* __restrict__ count,
                      uint8_t* out, size_t frame_stride) {
    extern __shared__ uint32_t lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t ens = blockIdx.x / (uint32_t)(n_sub + 1), s = blockIdx.x % (uint32_t)(n_sub + 1);
    const dabgpu_tx_sub_plan P = subs[s];
    const dabgpu_tx_sched_entry* sch = sched + P.sched_offset;
    const uint32_t first_frame = *count;
    const uint32_t nw1 = P.n_words + 1;

    if (s == (uint32_t)n_sub) {
        // FIC: 4 groups of 3 FIBs -> 4 x 2304 bits at the head of the frame; and the zeros of the unoccupied capacity units
        uint32_t* in = lds;                      // [4][24] dwords: 3 x (30 bytes + CRC) per group
        uint32_t* cw = lds + 96;                 // [4][72]
        for (uint32_t f = 0; f < n_frames; f++) {
            const size_t frame = (size_t)ens * n_frames + f;
            uint8_t* o = out + frame * frame_stride;
            for (uint32_t i = tid; i < 288; i += 256) cw[i] = 0;
            if (tid < 12) {
                const uint8_t* b = fib + (frame * 12 + tid) * 30;
                uint8_t* d = reinterpret_cast<uint8_t*>(in) + 32 * tid;
                uint32_t crc = 0xFFFFu;
                for (int k = 0; k < 30; k++) { const uint32_t v = b[k]; d[k] = (uint8_t)v; crc = tx_crc16_step(crc, v); }
                crc ^= 0xFFFFu;
                d[30] = (uint8_t)(crc >> 8); d[31] = (uint8_t)(crc & 0xFFu);
            }
            __syncthreads();
            for (uint32_t it = tid; it < 4 * nw1; it += 256) tx_encode_word(in + 24 * (it / nw1), it % nw1, P.n_words, sch, prbs, cw + 72 * (it / nw1));
            __syncthreads();
            for (uint32_t i = tid; i < 288; i += 256) reinterpret_cast<uint32_t*>(o)[i] = cw[i];
            for (int gi = 0; gi < n_gaps; gi++) {
                const uint32_t gs = gaps[2 * gi], gl = gaps[2 * gi + 1];
                for (uint32_t it = tid; it < 4 * gl; it += 256)
                    *reinterpret_cast<uint2*>(o + TX_FIC_BYTES + (size_t)(it / gl) * TX_CIF_BYTES + (size_t)(gs + it % gl) * 8) = make_uint2(0u, 0u);
            }
            __syncthreads();
        }
        return;
    }

    const uint32_t nblk = P.ring_row_dwords;    // blocks of 512 bits = dwords of a class row
    const uint32_t cw_dwords = 16 * nblk;       // one logical frame in LDS, the last block zero padded
    uint32_t* ring_e = ring + (size_t)ens * 16 * ring_slot_dwords + P.ring_offset;
    for (uint32_t f = 0; f < n_frames; f++) {
        const size_t frame = (size_t)ens * n_frames + f;
        const uint32_t slot0 = 4u * ((first_frame + f) & 3u);                   // ring slot of the frame's first CIF
        for (uint32_t i = tid; i < 4 * cw_dwords; i += 256) lds[i] = 0;
        __syncthreads();
        for (uint32_t it = tid; it < 4 * nw1; it += 256) {
            const uint32_t q = it / nw1;
            const uint32_t* src = reinterpret_cast<const uint32_t*>(payload + (frame * 4 + q) * (size_t)cif_in_bytes + P.in_offset);
            tx_encode_word(src, it % nw1, P.n_words, sch, prbs, lds + q * cw_dwords);
        }
        __syncthreads();
        // emit the frame's CIFs
        for (uint32_t it = tid; it < 4 * nblk; it += 256) {
            const uint32_t q = it / nblk, k = it % nblk;
            uint32_t a[16];
            tx_emit_block(ring_e + (size_t)((slot0 + q) & 15u) * ring_slot_dwords + k, nblk, lds, cw_dwords, q, k, a);
            uint8_t* o = out + frame * frame_stride + TX_FIC_BYTES + (size_t)q * TX_CIF_BYTES + (size_t)P.start_address * 8 + (size_t)k * 64;
            const uint32_t nd = min(16u, 2u * P.length - 16u * k);             // dwords of this block inside the sub-channel (even)
#pragma unroll
            for (uint32_t j = 0; j < 8; j++)
                if (2 * j < nd) reinterpret_cast<uint2*>(o)[j] = make_uint2(a[2 * j], a[2 * j + 1]);
        }
        __syncthreads();
        // file what later frames send
        for (uint32_t it = tid; it < 4 * nblk; it += 256) {
            const uint32_t q = it / nblk, k = it % nblk;
            tx_file_block(ring_e, ring_slot_dwords, nblk, slot0, lds, cw_dwords, q, k);
        }
        __threadfence_block();
        __syncthreads();
    }
}

__global__ void tx_advance_kernel(uint32_t* count, uint32_t n_frames) { *count += n_frames; }

}  // namespace dabgpu

using namespace dabgpu;

struct dabgpu_tx_bank {
    dabgpu_ctx* ctx = nullptr;
    size_t n_ens = 0;
    int n_sub = 0;
    dabgpu_tx_plan plan;
    DeviceBuffer<> d_tables;                    // one allocation: sub plans | schedules | gaps | energy-dispersal words
    dabgpu_tx_sub_plan* d_subs = nullptr;       // (these four into d_tables)
    dabgpu_tx_sched_entry* d_sched = nullptr;
    uint32_t* d_gaps = nullptr;
    uint32_t* d_prbs = nullptr;
    DeviceBuffer<uint32_t> d_ring;              // [n_ens][16][ring_slot_dwords] | frame counter
    size_t ring_bytes = 0;
    uint32_t* d_count = nullptr;                // (into d_ring)
    size_t lds_bytes = 0;
    // grow-only buffers: [0] transmit_frames' frame bits; host forms: [1] FIB bodies, [2] payload, [3] frame bits / IQ out
    DeviceBuffer<> buf[4];
};

// room for `bytes` in a grow-only buffer: never while `user` captures a graph (it would hold the old address), else behind a hipDeviceSynchronize
static int tx_grow(DeviceBuffer<>& buf, size_t bytes, hipStream_t user, const char* who) {
    int st = DABGPU_OK;
    if (buf.needs(bytes)) {
        if (dabgpu_stream_capturing(user)) {
            dabgpu_set_error("%s: this call needs more frame-bit scratch than the bank holds (%zu -> %zu bytes): run it once with this frame count before capturing",
                             who, buf.capacity(), bytes);
            return DABGPU_ERR_INVALID_ARG;
        }
        if (buf) DABGPU_CK(hipDeviceSynchronize());
        st = buf.regrow(bytes, "hipMalloc(&b->buf[which], bytes)");
    }
    return st;
}

// arguments of an encode call, before any device call
static int tx_bank_check(const dabgpu_tx_bank* b, const void* fib, const void* payload, size_t F, const char* who) {
    if (!b) { dabgpu_set_error("%s: null bank", who); return DABGPU_ERR_INVALID_ARG; }
    if (F > (size_t)(1 << 22) / b->n_ens) { dabgpu_set_error("%s: too many frames (ensembles x frames <= 4194304)", who); return DABGPU_ERR_INVALID_ARG; }
    if (F > 0 && (!fib || (!payload && b->plan.cif_in_bytes > 0))) { dabgpu_set_error("%s: null FIB data / payload", who); return DABGPU_ERR_INVALID_ARG; }
    return DABGPU_OK;
}

static int tx_launch_encode(dabgpu_tx_bank* b, const uint8_t* d_fib, const uint8_t* d_payload, size_t F, uint8_t* d_bits, size_t stride, hipStream_t s) {
    const unsigned grid = (unsigned)(b->n_ens * (size_t)(b->n_sub + 1));
    hipLaunchKernelGGL(tx_encode_kernel, dim3(grid), dim3(256), b->lds_bytes, s, b->d_subs, b->d_sched, b->d_gaps, (int)(b->plan.gaps.size() / 2),
                       b->d_prbs, b->n_sub, (uint32_t)F, b->plan.cif_in_bytes, b->plan.ring_slot_dwords, d_fib, d_payload, b->d_ring.get(), b->d_count, d_bits,
                       stride);
    hipLaunchKernelGGL(tx_advance_kernel, dim3(1), dim3(1), 0, s, b->d_count, (uint32_t)F);
    return dabgpu_check_hip(hipGetLastError(), "tx_encode_kernel launch");
}

extern "C" {

int dabgpu_tx_bank_create(dabgpu_ctx* c, size_t n_ens, const dabgpu_subchannel* subs, int n_sub, dabgpu_tx_bank** out) {
    if (!c || !out) { dabgpu_set_error("tx_bank_create: null context / result"); return DABGPU_ERR_INVALID_ARG; }
    *out = nullptr;
    if (n_ens == 0 || n_ens > (size_t)(1 << 20)) { dabgpu_set_error("tx_bank_create: %zu ensembles (1..1048576 are accepted)", n_ens); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_tx_bank* b = new (std::nothrow) dabgpu_tx_bank;
    if (!b) return DABGPU_ERR_HIP;
    int st = dabgpu_host_tx_plan(subs, n_sub, &b->plan);
    if (st) { delete b; return st; }
    b->ctx = c; b->n_ens = n_ens; b->n_sub = n_sub;
    const dabgpu_tx_plan& P = b->plan;
    b->lds_bytes = std::max<size_t>((96 + 288) * 4, (size_t)4 * 16 * ((P.max_length + 7) / 8) * 4);
    auto fail = [&](int status) { dabgpu_tx_bank_destroy(b); return status; };
    if ((st = dabgpu_bind_device(c))) return fail(st);
    // tables
    dabgpu_vit_tables vt;
    dabgpu_host_fill_vit_tables(&vt);
    std::vector<uint32_t> prbs(TX_PRBS_WORDS);
    for (int j = 0; j < TX_PRBS_WORDS; j++)
        for (int k = 0; k < 4; k++) prbs[(size_t)j] |= (uint32_t)vt.prbs[(4 * j + k) % 511] << (8 * k);
    const size_t subs_bytes = P.subs.size() * sizeof(dabgpu_tx_sub_plan), sched_bytes = P.sched.size() * sizeof(dabgpu_tx_sched_entry);
    const size_t gaps_bytes = std::max<size_t>(P.gaps.size(), 2) * 4, prbs_bytes = prbs.size() * 4;
    std::vector<unsigned char> img(subs_bytes + sched_bytes + gaps_bytes + prbs_bytes, 0);
    memcpy(img.data(), P.subs.data(), subs_bytes);
    memcpy(img.data() + subs_bytes, P.sched.data(), sched_bytes);
    if (!P.gaps.empty()) memcpy(img.data() + subs_bytes + sched_bytes, P.gaps.data(), P.gaps.size() * 4);
    memcpy(img.data() + subs_bytes + sched_bytes + gaps_bytes, prbs.data(), prbs_bytes);
    if ((st = b->d_tables.alloc(img.size(), "hipMalloc(tx tables)"))) return fail(st);
    unsigned char* t = static_cast<unsigned char*>(b->d_tables.get());
    b->d_subs = reinterpret_cast<dabgpu_tx_sub_plan*>(t);
    b->d_sched = reinterpret_cast<dabgpu_tx_sched_entry*>(t + subs_bytes);
    b->d_gaps = reinterpret_cast<uint32_t*>(t + subs_bytes + sched_bytes);
    b->d_prbs = reinterpret_cast<uint32_t*>(t + subs_bytes + sched_bytes + gaps_bytes);
    b->ring_bytes = n_ens * 16 * (size_t)P.ring_slot_dwords * 4;
    if ((st = b->d_ring.alloc(b->ring_bytes / 4 + 4, "hipMalloc(tx ring)"))) return fail(st);
    b->d_count = b->d_ring.get() + b->ring_bytes / 4;
    if ((st = tx_grow(b->buf[0], n_ens * TX_FRAME_BYTES, c->stream, "tx_bank_create"))) return fail(st);
    if ((st = dabgpu_check_hip(hipMemcpyAsync(t, img.data(), img.size(), hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync(tx tables)"))) return fail(st);
    if ((st = dabgpu_tx_bank_reset(b, c->stream))) return fail(st);
    if ((st = dabgpu_check_hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize(tx_bank_create)"))) return fail(st);
    *out = b;
    return DABGPU_OK;
}

void dabgpu_tx_bank_destroy(dabgpu_tx_bank* b) {
    if (!dabgpu_destroy_begin(b, b ? b->ctx : nullptr)) return;
    delete b;
}

int dabgpu_tx_bank_reset(dabgpu_tx_bank* b, void* stream) {
    if (!b) { dabgpu_set_error("tx_bank_reset: null bank"); return DABGPU_ERR_INVALID_ARG; }
    DABGPU_BIND(b->ctx);
    return dabgpu_check_hip(hipMemsetAsync(b->d_ring.get(), 0, b->ring_bytes + 16, (hipStream_t)stream), "hipMemsetAsync(tx ring)");
}

int dabgpu_tx_bank_encode_frames(dabgpu_tx_bank* b, const uint8_t* d_fib, const uint8_t* d_payload, size_t F, uint8_t* d_bits, size_t frame_stride,
                                 void* stream) {
    int st = tx_bank_check(b, d_fib, d_payload, F, "tx_bank_encode_frames");
    if (st || F == 0) return st;
    if (frame_stride == 0) frame_stride = TX_FRAME_BYTES;
    if (!d_bits || ((uintptr_t)d_bits & 15) || frame_stride < TX_FRAME_BYTES || (frame_stride & 15) || ((uintptr_t)d_payload & 3)) {
        dabgpu_set_error("tx_bank_encode_frames: d_frame_bits must be 16-byte aligned, frame_stride 0 or a multiple of 16 >= 28800, d_payload 4-byte aligned");
        return DABGPU_ERR_INVALID_ARG;
    }
    DABGPU_BIND(b->ctx);
    return tx_launch_encode(b, d_fib, d_payload, F, d_bits, frame_stride, (hipStream_t)stream);
}

static int tx_format_check(const void* out, int out_format, size_t F, const char* who) {
    if (out_format != DABGPU_IQ_RAW_F32L && out_format != DABGPU_IQ_RAW_U8) {
        dabgpu_set_error("%s: output format %d (DABGPU_IQ_RAW_F32L or DABGPU_IQ_RAW_U8 only)", who, out_format); return DABGPU_ERR_INVALID_ARG;
    }
    if (F > 0 && !out) { dabgpu_set_error("%s: null output", who); return DABGPU_ERR_INVALID_ARG; }
    return DABGPU_OK;
}

int dabgpu_tx_bank_transmit_frames(dabgpu_tx_bank* b, const uint8_t* d_fib, const uint8_t* d_payload, size_t F, float freq_norm, void* d_out,
                                   int out_format, void* stream) {
    int st = tx_bank_check(b, d_fib, d_payload, F, "tx_bank_transmit_frames");
    if (st) return st;
    if ((st = tx_format_check(d_out, out_format, F, "tx_bank_transmit_frames")) || F == 0) return st;
    if (((uintptr_t)d_out & 15) || ((uintptr_t)d_payload & 3)) {
        dabgpu_set_error("tx_bank_transmit_frames: d_out must be 16-byte, d_payload 4-byte aligned"); return DABGPU_ERR_INVALID_ARG;
    }
    DABGPU_BIND(b->ctx);
    hipStream_t s = (hipStream_t)stream;
    if ((st = tx_grow(b->buf[0], b->n_ens * F * TX_FRAME_BYTES, s, "tx_bank_transmit_frames"))) return st;
    uint8_t* bits = static_cast<uint8_t*>(b->buf[0].get());
    if ((st = tx_launch_encode(b, d_fib, d_payload, F, bits, TX_FRAME_BYTES, s))) return st;
    return dabgpu_launch_ofdm_mod(b->ctx, 1, bits, DABGPU_TX_PAYLOAD_FRAME_BITS, b->n_ens * F, nullptr, freq_norm, d_out,
                                  out_format, s);
}

// host forms: inputs up, the batch call on the context's stream, result down
static int tx_host(dabgpu_tx_bank* b, const uint8_t* h_fib, const uint8_t* h_payload, size_t F, bool iq, float freq_norm, void* h_out, int out_format,
                   const char* who) {
    int st = tx_bank_check(b, h_fib, h_payload, F, who);
    if (st) return st;
    if (iq && (st = tx_format_check(h_out, out_format, F, who))) return st;
    if (F == 0) return DABGPU_OK;
    if (!h_out) { dabgpu_set_error("%s: null output", who); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_ctx* c = b->ctx;
    DABGPU_BIND(c);
    DABGPU_HOST_LOCK(c);
    hipStream_t s = c->stream;
    const size_t n = b->n_ens * F;
    const size_t fib_bytes = n * 360, pay_bytes = n * 4 * (size_t)b->plan.cif_in_bytes;
    const size_t out_bytes = iq ? n * DABGPU_NB_FRAME_SAMPLES * (out_format == DABGPU_IQ_RAW_F32L ? 8 : 2) : n * TX_FRAME_BYTES;
    if ((st = tx_grow(b->buf[1], fib_bytes, s, who))) return st;
    if (pay_bytes && (st = tx_grow(b->buf[2], pay_bytes, s, who))) return st;
    if ((st = tx_grow(b->buf[3], out_bytes, s, who))) return st;
    void *d_fib = b->buf[1].get(), *d_pay = pay_bytes ? b->buf[2].get() : nullptr, *d_out = b->buf[3].get();
    DABGPU_CK(hipMemcpyAsync(d_fib, h_fib, fib_bytes, hipMemcpyHostToDevice, s));
    if (pay_bytes) DABGPU_CK(hipMemcpyAsync(d_pay, h_payload, pay_bytes, hipMemcpyHostToDevice, s));
    st = iq ? dabgpu_tx_bank_transmit_frames(b, static_cast<uint8_t*>(d_fib), static_cast<uint8_t*>(d_pay), F, freq_norm, d_out, out_format, s)
            : dabgpu_tx_bank_encode_frames(b, static_cast<uint8_t*>(d_fib), static_cast<uint8_t*>(d_pay), F, static_cast<uint8_t*>(d_out), 0, s);
    if (st) return st;
    DABGPU_CK(hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, s));
    DABGPU_CK(hipStreamSynchronize(s));
    return DABGPU_OK;
}

int dabgpu_tx_bank_encode_frames_host_sync(dabgpu_tx_bank* b, const uint8_t* h_fib, const uint8_t* h_payload, size_t F, uint8_t* h_frame_bits) {
    return tx_host(b, h_fib, h_payload, F, false, 0.0f, h_frame_bits, 0, "tx_bank_encode_frames_host_sync");
}

int dabgpu_tx_bank_transmit_frames_host_sync(dabgpu_tx_bank* b, const uint8_t* h_fib, const uint8_t* h_payload, size_t F, float freq_norm, void* h_out,
                                             int out_format) {
    return tx_host(b, h_fib, h_payload, F, true, freq_norm, h_out, out_format, "tx_bank_transmit_frames_host_sync");
}

}  // extern "C"
