// channel_ber.hip -- channel ("pre-Viterbi") bit error rate of decoded code words (include/dabgpu.h, "Channel BER"): the decoder's output
// bytes are encoded again and compared with the hard decisions of the soft bits the decoder consumed, read where the decoder read them.
//
// One wavefront per code word -- (ensemble, CIF, sub-channel) and (ensemble, FIB group) -- four of them to a workgroup:
//   1. the code word is built once in the wavefront's LDS, one lane per 32 input bits (tx_encode_word of dab_encode_core.h over the
//      schedule of dabgpu_tx_encode_plan: energy dispersal, K = 7 rate-1/4 code with zero tail, puncturing);
//   2. the soft bits are read once, straight from the frame-history ring (nothing intermediate in device memory):
//        FIB group / direct code word   contiguous, one dword (4 soft bits) per lane;
//        DABGPU_BITS_NATURAL            bit i from the CIF that is 15 - bitrev4(i mod 16) CIFs older: a lane keeps its class, one byte each;
//        DABGPU_BITS_MSC_CLASSED        each class row is contiguous: the LDS code word is transposed per block of 512 bits
//                                       (tx_natural_to_classes) so that 32 soft bits of a class meet one dword, and a lane reads 16 bytes
//                                       of its class row.  A row starts at 4 x start_address bytes: the loads start at the 16-byte
//                                       boundary below it and the bytes in front of the row (and behind it) are masked out;
//   3. four soft bits at a time are compared with packed integer operations, the four sums are reduced across the wavefront and lane 0
//      writes the record with one 16-byte store.  No global atomics.
// The in-place transpose reads LDS 16 dwords apart (lanes of a wavefront share banks); it is one pass per code word against the many of
// the comparison.
#include <hip/hip_runtime.h>
#include <string.h>

#include "dab_encode_core.h"
#include "dabgpu_internal.h"

namespace dabgpu {

static_assert(sizeof(dabgpu_ber_result) == 16, "one record = one 16-byte store");

struct ber_args {
    const int8_t* hist;                     // ring of the first ensemble; direct: the code word's soft bits
    size_t ens_stride;
    int hist_frames, newest;
    const int32_t* slots;                   // ring form: newest slot per ensemble
    const dabgpu_tx_sub_plan* subs;         // [n_sub + 1], the last the FIB group
    const dabgpu_tx_sched_entry* sched;
    const uint32_t* prbs;                   // [TX_PRBS_WORDS]
    uint32_t n_sub;
    uint32_t msc_cw, fic_cw;                // code words per ensemble of each half: 4 n_sub or 0, 4 or 0
    const uint8_t* fib;                     // [n_ens][4][96]
    const uint8_t* msc;                     // decoded sub-channel bytes; direct: the code word's bytes
    size_t out_ens_stride;
    uint32_t cif_bytes;
    dabgpu_ber_result* fic_res;
    dabgpu_ber_result* msc_res;             // direct: the one record
    uint32_t classed;
    int direct_sub;                         // >= 0: ONE code word of subs[direct_sub], soft bits contiguous at hist
    uint32_t cw_dwords;                     // LDS dwords per wavefront
    size_t n_cw;
};

struct ber_sums { uint32_t n_bits, n_err, err_w, tot_w; };

// four soft bits (the bytes of s4, lowest first) against code bits 0..3 of e4; `valid` = 0xFF in the bytes that count
__device__ __forceinline__ void ber_add4(ber_sums& A, uint32_t s4, uint32_t e4, uint32_t valid) {
    const uint32_t neg = (s4 >> 7) & 0x01010101u;
    const uint32_t mag = ((s4 ^ (neg * 0xFFu)) + neg) & valid;              // |s| per byte (~s + 1 <= 0x80: no carry leaves a byte), |-128| = 128
    const uint32_t nz = ((mag + 0x7F7F7F7Fu) >> 7) & 0x01010101u;           // mag <= 0x80: no carry either
    const uint32_t e = ((e4 & 15u) * 0x00204081u) & 0x01010101u;            // code bit b -> bit 0 of byte b
    const uint32_t err = nz & (neg ^ 0x01010101u ^ e);                      // hard decision (s >= 0) != code bit
    A.n_bits += (uint32_t)__popc(nz);
    A.n_err += (uint32_t)__popc(err);
    A.tot_w = __builtin_amdgcn_sad_u8(mag, 0u, A.tot_w);
    A.err_w = __builtin_amdgcn_sad_u8(mag & (err * 0xFFu), 0u, A.err_w);
}

__device__ __forceinline__ uint32_t ber_wave_sum(uint32_t v) {
#pragma unroll
    for (int m = 32; m; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}

// byte offset inside an ensemble's ring of the CIF the time de-interleaver takes class c from, for the code word of CIF q of the newest frame
__device__ __forceinline__ size_t ber_class_cif(uint32_t c, int newest, uint32_t q, int hist_frames) {
    const int age = 15 - (int)tx_cif_delay(c);
    int slot = 4 * newest + (int)q - age;
    if (slot < 0) slot += 4 * hist_frames;
    return (size_t)(slot >> 2) * DABGPU_NB_FRAME_BITS + DABGPU_NB_FIC_BITS + (size_t)(slot & 3) * DABGPU_NB_CIF_BITS;
}

__global__ __launch_bounds__(64 * DABGPU_BER_WAVES)
void ber_kernel(const ber_args a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t ber_lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t* cw = ber_lds + wave * a.cw_dwords;
    const size_t id = (size_t)blockIdx.x * DABGPU_BER_WAVES + wave;
    const uint32_t per = a.msc_cw + a.fic_cw;

    // which code word: all of this is uniform across the wavefront
    bool active = id < a.n_cw;
    uint32_t s = a.n_sub, q = 0;
    const int8_t* bits = a.hist;            // contiguous soft bits (FIB group, direct code word); ring forms: the ensemble's ring
    const uint8_t* bytes = a.msc;
    dabgpu_ber_result* res = a.msc_res;
    bool ring = false;
    int newest = a.newest;
    if (active && a.direct_sub >= 0) {
        s = (uint32_t)a.direct_sub;
    } else if (active) {
        const size_t ens = id / per;
        const uint32_t r = (uint32_t)(id - ens * per);
        bits = a.hist + ens * a.ens_stride;
        if (a.slots) newest = a.slots[ens];
        if (r < a.msc_cw) {
            q = r / a.n_sub; s = r - q * a.n_sub;
            res = a.msc_res + (ens * 4 + q) * a.n_sub + s;
            bytes = a.msc + ens * a.out_ens_stride + (size_t)q * a.cif_bytes;           // + the sub-channel's offset below
            ring = true;
        } else {
            const uint32_t g = r - a.msc_cw;
            res = a.fic_res + ens * 4 + g;
            bytes = a.fib + (ens * 4 + g) * 96;
            if (newest >= 0) bits += (size_t)newest * DABGPU_NB_FRAME_BITS + (size_t)g * DABGPU_NB_FIB_GROUP_BITS;
        }
        if (newest < 0) {                   // ring form: nothing new for this ensemble
            if (lane == 0) *reinterpret_cast<uint4*>(res) = make_uint4(0u, 0u, 0u, 0u);
            active = false;
        }
    }
    const dabgpu_tx_sub_plan P = a.subs[s];
    const uint32_t K = P.kept_bits;
    if (ring) bytes += P.in_offset;

    // 1. the code word, in natural bit order
    for (uint32_t i = lane; i < a.cw_dwords; i += 64) cw[i] = 0;
    __syncthreads();
    if (active) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(bytes);
        const dabgpu_tx_sched_entry* sch = a.sched + P.sched_offset;
        for (uint32_t w = lane; w <= P.n_words; w += 64) tx_encode_word(src, w, P.n_words, sch, a.prbs, cw);
    }
    __syncthreads();

    ber_sums A = {0u, 0u, 0u, 0u};
    if (active && !ring) {
        // 2a. contiguous soft bits: K is a multiple of 4 (12 tail bits + 4 x blocks x (8 + PI))
        const uint32_t* sb = reinterpret_cast<const uint32_t*>(bits);
        for (uint32_t d = lane; d < K / 4u; d += 64) ber_add4(A, sb[d], cw[d >> 3] >> (4u * (d & 7u)), 0xFFFFFFFFu);
    } else if (active && !a.classed) {
        // 2b. natural order: bit i of the sub-channel at frame bit 9216 + 55296 cif + 64 start + i of the CIF of its class; i = lane + 64 k keeps the class
        const int8_t* p = bits + ber_class_cif(lane & 15u, newest, q, a.hist_frames) + (size_t)P.start_address * 64u;
        for (uint32_t i = lane; i < K; i += 64) ber_add4(A, (uint32_t)(uint8_t)p[i], cw[i >> 5] >> (i & 31u), 0xFFu);
    }
    if (a.classed) {                        // (uniform across the workgroup: every wavefront meets the barrier)
        const uint32_t nblk = P.ring_row_dwords;        // blocks of 512 bits; 16 nblk <= cw_dwords (dabgpu_ber_cw_dwords)
        if (active && ring) {
            for (uint32_t k = lane; k < nblk; k += 64) {
                uint32_t t[16];
#pragma unroll
                for (int m = 0; m < 16; m++) t[m] = cw[16u * k + (uint32_t)m];
                tx_natural_to_classes(t);
#pragma unroll
                for (int m = 0; m < 16; m++) cw[16u * k + (uint32_t)m] = t[m];
            }
        }
        __syncthreads();
        if (active && ring) {
            // 2c. class order: bit i = 16 j + c of the sub-channel is byte 4 start + j of class row c (3456 bytes each) of that class's CIF; code bit
            // at bit j % 32 of cw[16 (j / 32) + c].  Lane = (class c, chunk): 16 bytes from the 16-byte boundary below the row's first byte on.
            const uint32_t c = lane & 15u;
            const uint32_t L = P.length;                                    // dwords of a row
            const uint32_t mis = P.start_address & 3u;                     // dwords between that boundary and the row
            const uint32_t jmax = K > c ? (K - c + 15u) / 16u : 0u;        // positions j of this class inside the code word
            const uint32_t nq = (L + mis + 3u) / 4u;
            const int8_t* row = bits + ber_class_cif(c, newest, q, a.hist_frames) + (size_t)c * (DABGPU_NB_CIF_BITS / 16) + (size_t)P.start_address * 4u;
            const uint4* chunks = reinterpret_cast<const uint4*>(row - 4u * mis);
            for (uint32_t qi = lane >> 4; qi < nq; qi += 4) {
                const uint4 v = chunks[qi];
                const uint32_t sv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (uint32_t r = 0; r < 4; r++) {
                    const uint32_t dd = 4u * qi + r;                        // dword of the aligned run; dd - mis = dword d of the row
                    if (dd < mis || dd - mis >= L) continue;
                    const uint32_t d = dd - mis;
                    if (4u * d >= jmax) continue;
                    const uint32_t nv = jmax - 4u * d;                      // bytes of this dword inside the code word
                    const uint32_t valid = nv >= 4u ? 0xFFFFFFFFu : (1u << (8u * nv)) - 1u;
                    ber_add4(A, sv[r], cw[16u * (d >> 3) + c] >> (4u * (d & 7u)), valid);
                }
            }
        }
    }

    // 3. reduce and store
    const uint32_t n_bits = ber_wave_sum(A.n_bits), n_err = ber_wave_sum(A.n_err), err_w = ber_wave_sum(A.err_w), tot_w = ber_wave_sum(A.tot_w);
    if (active && lane == 0) *reinterpret_cast<uint4*>(res) = make_uint4(n_bits, n_err, err_w, tot_w);
}

}  // namespace dabgpu

using namespace dabgpu;

// the device image of a multiplex's tables: energy-dispersal words | schedules | plans (the FIB group's last)
struct ber_image {
    std::vector<unsigned char> bytes;
    size_t sched_at = 0, subs_at = 0;
};
static ber_image ber_make_image(const dabgpu_tx_plan& P) {
    dabgpu_vit_tables vt;
    dabgpu_host_fill_vit_tables(&vt);
    uint32_t prbs[TX_PRBS_WORDS + 1] = {};
    for (int j = 0; j < TX_PRBS_WORDS; j++)
        for (int k = 0; k < 4; k++) prbs[j] |= (uint32_t)vt.prbs[(4 * j + k) % 511] << (8 * k);
    ber_image I;
    I.sched_at = sizeof(prbs);
    I.subs_at = I.sched_at + P.sched.size() * sizeof(dabgpu_tx_sched_entry);
    I.bytes.assign(I.subs_at + P.subs.size() * sizeof(dabgpu_tx_sub_plan), 0);
    memcpy(I.bytes.data(), prbs, sizeof(prbs));
    memcpy(I.bytes.data() + I.sched_at, P.sched.data(), P.sched.size() * sizeof(dabgpu_tx_sched_entry));
    memcpy(I.bytes.data() + I.subs_at, P.subs.data(), P.subs.size() * sizeof(dabgpu_tx_sub_plan));
    return I;
}
static void ber_point_tables(ber_args& a, const ber_image& I, const void* d_tables) {
    const unsigned char* t = static_cast<const unsigned char*>(d_tables);
    a.prbs = reinterpret_cast<const uint32_t*>(t);
    a.sched = reinterpret_cast<const dabgpu_tx_sched_entry*>(t + I.sched_at);
    a.subs = reinterpret_cast<const dabgpu_tx_sub_plan*>(t + I.subs_at);
}

static int ber_batch(dabgpu_ctx* c, const char* who, const int8_t* d_hist, size_t n_ens, size_t ens_stride, int hist_frames, int newest,
                     const int32_t* d_slots, bool ring_form, const dabgpu_subchannel* h_sub, int n_sub, const uint8_t* d_fib, const uint8_t* d_msc,
                     size_t out_ens_stride, dabgpu_ber_result* d_fic_ber, dabgpu_ber_result* d_msc_ber, int bits_layout, hipStream_t s) {
    if (!c) { dabgpu_set_error("%s: null context", who); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_ber_launch L;
    int st = dabgpu_host_ber_plan(h_sub, n_sub, n_ens, hist_frames, ens_stride, out_ens_stride, bits_layout, &L);
    if (st) return st;
    if (ring_form ? !d_slots : (newest < 0 || newest >= hist_frames)) {
        dabgpu_set_error(ring_form ? "%s: null d_newest_slot" : "%s: 0 <= newest_frame_slot < history_frames", who); return DABGPU_ERR_INVALID_ARG;
    }
    const bool fic = d_fib && d_fic_ber, msc = n_sub > 0 && d_msc && d_msc_ber;
    if (!fic && !msc) return DABGPU_OK;
    if (!d_hist || ((uintptr_t)d_hist & 15)) { dabgpu_set_error("%s: d_bits_history must be 16-byte aligned and not null", who); return DABGPU_ERR_INVALID_ARG; }
    if ((fic && (((uintptr_t)d_fib & 3) || ((uintptr_t)d_fic_ber & 15))) || (msc && (((uintptr_t)d_msc & 3) || ((uintptr_t)d_msc_ber & 15)))) {
        dabgpu_set_error("%s: the decoded bytes must be 4-byte, the records 16-byte aligned", who); return DABGPU_ERR_INVALID_ARG;
    }
    DABGPU_BIND(c);
    const ber_image I = ber_make_image(L.tx);
    void* d_tables;
    if ((st = dabgpu_scratch(c, SCR_BER_TABLES, I.bytes.size(), &d_tables, s))) return st;
    if ((st = dabgpu_stage_h2d_cached(c, 2, d_tables, I.bytes.data(), I.bytes.size(), s))) return st;
    ber_args a = {};
    ber_point_tables(a, I, d_tables);
    a.hist = d_hist; a.ens_stride = ens_stride; a.hist_frames = hist_frames; a.newest = ring_form ? 0 : newest; a.slots = ring_form ? d_slots : nullptr;
    a.n_sub = (uint32_t)n_sub; a.msc_cw = msc ? 4u * (uint32_t)n_sub : 0u; a.fic_cw = fic ? 4u : 0u;
    a.fib = d_fib; a.msc = d_msc; a.out_ens_stride = out_ens_stride; a.cif_bytes = L.geo.cif_bytes;
    a.fic_res = d_fic_ber; a.msc_res = d_msc_ber;
    a.classed = bits_layout == DABGPU_BITS_MSC_CLASSED; a.direct_sub = -1;
    a.cw_dwords = L.geo.lds_bytes / 4u;
    a.n_cw = n_ens * (size_t)(a.msc_cw + a.fic_cw);
    const unsigned grid = (unsigned)((a.n_cw + DABGPU_BER_WAVES - 1) / DABGPU_BER_WAVES);
    hipLaunchKernelGGL(ber_kernel, dim3(grid), dim3(64 * DABGPU_BER_WAVES), (size_t)L.geo.lds_bytes * DABGPU_BER_WAVES, s, a);
    return dabgpu_check_hip(hipGetLastError(), "ber_kernel launch");
}

// one code word of tx.subs[which] from and to host memory: tables | soft bits | bytes | record in one scratch block of the host forms
static int ber_host_one(dabgpu_ctx* c, const dabgpu_tx_plan& tx, int which, const int8_t* h_bits, const uint8_t* h_bytes,
                        dabgpu_ber_result* result) {
    const dabgpu_tx_sub_plan& P = tx.subs[(size_t)which];
    const ber_image I = ber_make_image(tx);
    const size_t bits_at = (I.bytes.size() + 15) & ~(size_t)15, bytes_at = bits_at + (((size_t)P.kept_bits + 15) & ~(size_t)15);
    const size_t res_at = bytes_at + (((size_t)P.in_bytes + 15) & ~(size_t)15);
    DABGPU_BIND(c);
    DABGPU_HOST_LOCK(c);
    int st;
    unsigned char* d;
    if ((st = dabgpu_scratch(c, SCR_BER_HOST, res_at + sizeof(dabgpu_ber_result), reinterpret_cast<void**>(&d)))) return st;
    hipStream_t s = c->stream;
    DABGPU_CK(hipMemcpyAsync(d, I.bytes.data(), I.bytes.size(), hipMemcpyHostToDevice, s));
    DABGPU_CK(hipMemcpyAsync(d + bits_at, h_bits, P.kept_bits, hipMemcpyHostToDevice, s));
    DABGPU_CK(hipMemcpyAsync(d + bytes_at, h_bytes, P.in_bytes, hipMemcpyHostToDevice, s));
    ber_args a = {};
    ber_point_tables(a, I, d);
    a.hist = reinterpret_cast<const int8_t*>(d + bits_at); a.msc = d + bytes_at; a.msc_res = reinterpret_cast<dabgpu_ber_result*>(d + res_at);
    a.n_sub = (uint32_t)tx.subs.size() - 1u; a.direct_sub = which;
    a.cw_dwords = dabgpu_ber_cw_dwords(P.length); a.n_cw = 1;
    hipLaunchKernelGGL(ber_kernel, dim3(1), dim3(64 * DABGPU_BER_WAVES), (size_t)a.cw_dwords * 4 * DABGPU_BER_WAVES, s, a);
    if ((st = dabgpu_check_hip(hipGetLastError(), "ber_kernel launch"))) return st;
    DABGPU_CK(hipMemcpyAsync(result, d + res_at, sizeof(dabgpu_ber_result), hipMemcpyDeviceToHost, s));
    DABGPU_CK(hipStreamSynchronize(s));
    return DABGPU_OK;
}

extern "C" {

int dabgpu_ber_frames_layout(dabgpu_ctx* c, const int8_t* d_hist, size_t n_ens, size_t ens_stride, int hist_frames, int newest_frame_slot,
                             const dabgpu_subchannel* h_sub, int n_sub, const uint8_t* d_fib, const uint8_t* d_msc, size_t out_ens_stride,
                             dabgpu_ber_result* d_fic_ber, dabgpu_ber_result* d_msc_ber, int bits_layout, void* stream) {
    return ber_batch(c, "ber_frames_layout", d_hist, n_ens, ens_stride, hist_frames, newest_frame_slot, nullptr, false, h_sub, n_sub, d_fib, d_msc,
                     out_ens_stride, d_fic_ber, d_msc_ber, bits_layout, (hipStream_t)stream);
}

int dabgpu_ber_ring_layout(dabgpu_ctx* c, const int8_t* d_hist, size_t n_ens, size_t ens_stride, int hist_frames, const int32_t* d_newest_slot,
                           const dabgpu_subchannel* h_sub, int n_sub, const uint8_t* d_fib, const uint8_t* d_msc, size_t out_ens_stride,
                           dabgpu_ber_result* d_fic_ber, dabgpu_ber_result* d_msc_ber, int bits_layout, void* stream) {
    return ber_batch(c, "ber_ring_layout", d_hist, n_ens, ens_stride, hist_frames, 0, d_newest_slot, true, h_sub, n_sub, d_fib, d_msc, out_ens_stride,
                     d_fic_ber, d_msc_ber, bits_layout, (hipStream_t)stream);
}

int dabgpu_ber_fib_group_host_sync(dabgpu_ctx* c, const int8_t* h_bits, const uint8_t* h_bytes, dabgpu_ber_result* result) {
    if (!c || !h_bits || !h_bytes || !result) { dabgpu_set_error("ber_fib_group_host_sync: null argument"); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_tx_plan tx;
    const int st = dabgpu_host_tx_plan(nullptr, 0, &tx);
    if (st) return st;
    return ber_host_one(c, tx, 0, h_bits, h_bytes, result);
}

int dabgpu_ber_codeword_host_sync(dabgpu_ctx* c, const dabgpu_subchannel* sc, const int8_t* h_bits, const uint8_t* h_bytes, dabgpu_ber_result* result) {
    if (!c || !sc || !h_bits || !h_bytes || !result) { dabgpu_set_error("ber_codeword_host_sync: null argument"); return DABGPU_ERR_INVALID_ARG; }
    int st = dabgpu_subchannel_validate(sc);
    if (st) return st;
    dabgpu_tx_plan tx;
    if ((st = dabgpu_host_tx_plan(sc, 1, &tx))) return st;
    return ber_host_one(c, tx, 0, h_bits, h_bytes, result);
}

}  // extern "C"
