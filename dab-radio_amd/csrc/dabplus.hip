// dabplus.hip -- the DAB+ outer code on the device: what AAC_Frame_Processor does between the channel
// decoder's bytes and the AAC access units (src/dab/audio/aac_frame_processor.cpp:127-361):
//   super-frame acquisition on the fire code (:162-166, :178-189), accumulation of 5 logical frames (:191-197),
//   RS(120,110) decoding of the byte-interleaved columns (:323-361; decoder: src/dab/algorithms/reed_solomon_decoder.cpp,
//   Berlekamp-Massey / Chien / Forney over GF(2^8), p(x) = x^8+x^4+x^3+x^2+1, roots alpha^0..alpha^9, shortened by 135),
//   fire code of the corrected super frame (:206-209), header walk (:215-283) and access-unit CRCs (:286-317),
//   re-acquisition after 10 failed super frames (:151-154).
// One wavefront per stream (an (ensemble, sub-channel) pair); its acquisition state and the super frame being collected
// live in HBM between calls.  Syndromes: every lane adds the terms of a share of one codeword's symbols for all ten roots
// (XOR shuffles fold the shares); a codeword with a non-zero syndrome gets its error locator from ONE lane (Berlekamp-Massey,
// all codewords of the super frame in parallel), the Chien search and Forney's corrections are dealt over all 64 lanes; the
// access-unit CRCs are shared by 8-32 lanes each.  LDS table look-ups throughout (GF(2^8) log / exp, CRC-16).  The Reed-Solomon arithmetic
// is rs_core.h's (host check: tests/test_rs_core_host.py), tables and the shared-lane CRC rs_device.h's: both shared with packet_fec.hip.
// Integer / byte work, bit-exact by construction; checked against the oracle and the reference-generated vectors.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <new>
#include <vector>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "dabplus_common.h"

namespace dabgpu {

struct DpLds {
    uint8_t exp[512];
    uint8_t log[256];
    // CRC-16 x^16+x^12+x^5+1 table, MSB first (access units) -- or, while a super frame's codewords are being corrected, one record per
    // codeword: error-locator coefficients C_1..C_10, then (word at +12) degree | roots found << 8.  The table is rebuilt afterwards.
    union {
        uint16_t crc_tab[256];
        uint8_t rs_rec[64 * 16];
    };
    uint8_t sf[DP_MAX_SF];
    uint8_t syn[64 * RS_ROOTS];
    int flags[4];
    int au[8];                       // access-unit start offsets of the super frame being checked
};

struct DpState {                     // per stream, persistent
    int wait_frame_start, curr_dab_frame, prev_n, synced, desync_count;
};

// RS(120,110) decoding of a super frame's codewords (the arithmetic: rs_core.h), in two phases:
// rs_locator: ONE lane per codeword with a non-zero syndrome runs Berlekamp-Massey, its polynomials in registers, and leaves the error
// locator (C_1..C_10, degree) in the codeword's record and the evaluator omega in place of the syndromes;
// rs_search_and_correct: the Chien search over alpha^1..alpha^255 and Forney's formula are shared by ALL lanes -- the wavefront's lanes are
// dealt to the codewords (64 / n_rs each), every lane scans its share of the 255 candidates and corrects the symbol of each root it
// finds, counting it in the record.  A locator of degree d has at most d roots, so scanning all candidates finds what the reference's scan
// (which stops after d) finds; corrections made for a codeword that then turns out uncorrectable (roots != degree) are undone by the
// caller from the received bytes.
__device__ void rs_locator(DpLds& L, int i) {
    uint8_t* const omega = &L.syn[i * RS_ROOTS];             // (the syndromes are done with once S holds them)
    uint8_t S[RS_ROOTS];
#pragma unroll
    for (int r = 0; r < RS_ROOTS; r++) S[r] = omega[r];
    uint8_t C[RS_ROOTS + 1], B[RS_ROOTS + 1], T[RS_ROOTS + 1];
    const int deg = rs::locator<RS_ROOTS>(L, S, C, B, T, omega);
#pragma unroll
    for (int k = 1; k <= RS_ROOTS; k++) L.rs_rec[i * 16 + k - 1] = C[k];
    *reinterpret_cast<int*>(&L.rs_rec[i * 16 + 12]) = deg;
}

__device__ void rs_search_and_correct(DpLds& L, int i, int q, int per, int n_rs) {
    int* const rec = reinterpret_cast<int*>(&L.rs_rec[i * 16 + 12]);
    const int deg = *rec & 0xFF;
    if (deg == 0) return;
    const int span = (255 + per - 1) / per, x0 = 1 + q * span, x1 = (x0 + span - 1 < 255) ? (x0 + span - 1) : 255;
    const uint8_t* const omega = &L.syn[i * RS_ROOTS];
    uint8_t C[RS_ROOTS + 1];
    int reg[RS_ROOTS + 1];
    C[0] = 1;
#pragma unroll
    for (int k = 1; k <= RS_ROOTS; k++) C[k] = L.rs_rec[i * 16 + k - 1];
    rs::chien_start<RS_ROOTS>(L, C, x0, reg);
    for (int x = x0; x <= x1; x++) {
        if (rs::chien_next<RS_ROOTS>(L, C, deg, reg)) continue;
        atomicAdd(rec, 0x100);
        const uint8_t val = rs::forney<RS_ROOTS>(L, C, omega, deg, x);
        const int loc = x - 1;
        if (val && loc >= RS_PAD) L.sf[i + (loc - RS_PAD) * n_rs] ^= val;
    }
}

// 9.6 KB of LDS per workgroup lets 16 single-wave workgroups share a CU = 4 per SIMD: hold the kernel to the 128 VGPRs that allows (the
// spilled values belong to the per-lane Berlekamp-Massey / Chien / Forney path; measured 0.224 / 0.169 / 0.153 ms per 18,432 clean super
// frames at 2 / 3 / 4 waves per SIMD, profiles/r04/ab_notes.md)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4)))
void dabplus_kernel(DpState* __restrict__ states, const uint8_t* __restrict__ frames, const unsigned long long* __restrict__ stream_offsets,
                    size_t frame_stride, const uint32_t* __restrict__ frame_bytes, int n_frames, uint8_t* __restrict__ sf_acc,
                    uint8_t* __restrict__ sf_out, size_t sf_out_stride, dabgpu_superframe_result* __restrict__ results, int max_sf,
                    int32_t* __restrict__ counts, int n_streams, const int32_t* __restrict__ active, int active_divisor)
{
    __shared__ DpLds L;
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= n_streams) return;
    if (active != nullptr && active[s / active_divisor] < 0) {           // nothing new for this stream's ensemble in this call
        if (lane == 0) { counts[4 * s] = 0; counts[4 * s + 1] = 0; counts[4 * s + 2] = 0; counts[4 * s + 3] = states[s].curr_dab_frame; }
        return;
    }
    load_gf_crc_tables(L, lane);
    DpState st = states[s];
    const int n = (int)frame_bytes[s];
    // what this kernel cannot hold is reported, not skipped in silence: logical frames above 1536 bytes (the reference accepts any
    // N >= 11, aac_frame_processor.cpp:129-137) -> counts[1] = -1; a super-frame slot smaller than 5 frames -> counts[1] = -2
    if (n > DP_MAX_FRAME_BYTES || (n >= 11 && (size_t)(5 * n) > sf_out_stride)) {
        if (lane == 0) { counts[4 * s] = 0; counts[4 * s + 1] = (n > DP_MAX_FRAME_BYTES) ? -1 : -2; counts[4 * s + 2] = 0; counts[4 * s + 3] = st.curr_dab_frame; }
        return;
    }
    uint8_t* acc = sf_acc + (size_t)s * DP_MAX_SF;
    const uint8_t* base = frames + stream_offsets[s];
    int n_sf = 0, n_wait_failed = 0, last_wait_crc = 0;
    __syncthreads();

    for (int f = 0; f < n_frames; f++) {
        const uint8_t* frame = base + (size_t)f * frame_stride;
        if (n < 11) continue;                                              // :129-137
        if (st.prev_n != n) { st.prev_n = n; st.curr_dab_frame = 0; st.wait_frame_start = 1; }       // :140-147
        if (st.desync_count >= 10) { st.desync_count = 0; st.synced = 0; }                           // :151-154
        if (st.synced) st.wait_frame_start = 0;                                                       // :158-160
        if (st.wait_frame_start) {                                                                    // :162-166
            const uint16_t rx = (uint16_t)((frame[0] << 8) | frame[1]);
            const uint16_t calc = firecode_wave(frame + 2, lane);
            const int ok = (rx == calc);
            if (!ok) last_wait_crc = (int)(((uint32_t)rx << 16) | calc);
            if (!ok) { n_wait_failed++; continue; }
            st.wait_frame_start = 0;
        }
        for (int k = lane; k < n; k += 64) acc[(size_t)st.curr_dab_frame * n + k] = frame[k];         // :191-197
        st.curr_dab_frame++;
        if (st.curr_dab_frame < 5) continue;

        // ---- ProcessSuperFrame (:199-321) ----
        st.wait_frame_start = 1;
        st.curr_dab_frame = 0;
        const int sf_bytes = 5 * n;
        const int n_rs = sf_bytes / RS_N;
        __syncthreads();                                                   // this wave's global writes of acc[] are visible to it
        for (int k = lane; k < sf_bytes; k += 64) L.sf[k] = acc[k];
        if (lane == 0) { L.flags[1] = -1; L.flags[2] = 0; }
        __syncthreads();
        // syndromes S_r(i) = sum_j c_j alpha^(r (119 - j)) -- what Horner's rule over the codeword (sy = sy alpha^r + c_j) evaluates.
        // When the codewords divide the wavefront (n_rs = 1, 2, 4, ... 64: every frame size of 24 x 2^k bytes, 192 among them) lane
        // (i, q) adds the terms of symbols j = q, q + 64 / n_rs, ... of codeword i for all ten roots -- independent table look-ups
        // instead of Horner's chain of 120 dependent ones -- and the partial sums of a codeword's lanes are folded by XOR shuffles
        // (GF(2^8) addition: exact, order-free).  Other sizes keep the (codeword, root) Horner form.
        if (n_rs > 0 && (64 % n_rs) == 0) {              // (frames below 24 bytes hold no codeword at all: n_rs = 0, nothing to correct)
            const int per = 64 / n_rs, i = lane % n_rs, q = lane / n_rs;
            uint32_t w[3] = {0, 0, 0};                                     // roots 0-3, 4-7, 8-9: one byte each
            for (int j = q; j < RS_N; j += per) rs::syndrome_add<RS_N, RS_ROOTS>(L, L.sf[i + j * n_rs], j, w);
            for (int sft = 32; sft >= n_rs; sft >>= 1) {
#pragma unroll
                for (int k = 0; k < 3; k++) w[k] ^= (uint32_t)__shfl_xor((int)w[k], sft);
            }
            if (q == 0) {
#pragma unroll
                for (int r = 0; r < RS_ROOTS; r++) L.syn[i * RS_ROOTS + r] = rs::packed_byte<RS_ROOTS>(w, r);
            }
        } else {
            for (int w = lane; w < n_rs * RS_ROOTS; w += 64) {             // work item = (codeword i, root r)
                const int i = w / RS_ROOTS, r = w - i * RS_ROOTS;
                uint8_t sy = 0;
                for (int j = 0; j < RS_N; j++) {
                    const uint8_t m = sy ? L.exp[L.log[sy] + r] : (uint8_t)0;
                    sy = (uint8_t)(m ^ L.sf[i + j * n_rs]);
                }
                L.syn[w] = sy;
            }
        }
        __syncthreads();
        int any = 0;
        if (lane < n_rs) {
#pragma unroll
            for (int r = 0; r < RS_ROOTS; r++) any |= L.syn[lane * RS_ROOTS + r];
        }
        const bool decode = __any(any != 0);               // (clean super frames skip all of this and keep the CRC table)
        int my_cnt = 0;
        if (decode) {
            __syncthreads();                                // every lane has read its syndromes; the records take the table's place
            if (lane < n_rs) {
                if (any) rs_locator(L, lane);
                else *reinterpret_cast<int*>(&L.rs_rec[lane * 16 + 12]) = 0;
            }
            __syncthreads();
            const int per = 64 / n_rs;                      // lanes per codeword (1 <= n_rs <= 64 here: a non-zero syndrome exists)
            if (lane < per * n_rs) rs_search_and_correct(L, lane % n_rs, lane / n_rs, per, n_rs);
            __syncthreads();
            if (lane < n_rs) {
                const int w = *reinterpret_cast<const int*>(&L.rs_rec[lane * 16 + 12]), deg = w & 0xFF, found = w >> 8;
                my_cnt = (found == deg) ? deg : -1;
            }
            __syncthreads();
            load_crc_table(L, lane);                        // back in its place
        }
        __syncthreads();
        if (lane == 0) L.flags[3] = 0x7FFFFFFF;
        __syncthreads();
        if (my_cnt < 0) atomicMin(&L.flags[3], lane);
        if (my_cnt > 0) atomicAdd(&L.flags[2], my_cnt);
        __syncthreads();
        const int first_fail = L.flags[3];
        dabgpu_superframe_result res;
        memset(&res, 0, sizeof(res));
        res.rs_failed_index = (first_fail == 0x7FFFFFFF) ? -1 : first_fail;
        res.au_walk_stopped_at = -1;
        res.frame_index = f;
        bool good = (res.rs_failed_index < 0);
        if (!good) {
            // the reference stops at the first uncorrectable codeword (:336-341): later codewords keep their received
            // symbols and the corrected-symbol count only covers the codewords before it
            // (and the failed codeword itself: the shared search corrects as it finds roots, before their number is known)
            for (int k = lane; k < sf_bytes; k += 64) if ((k % n_rs) >= first_fail) L.sf[k] = acc[k];
            if (lane == 0) L.flags[2] = 0;
            __syncthreads();
            if (my_cnt > 0 && lane < first_fail) atomicAdd(&L.flags[2], my_cnt);
            __syncthreads();
        }
        res.rs_corrected = L.flags[2];
        if (good) {
            const uint16_t rx = (uint16_t)((L.sf[0] << 8) | L.sf[1]);
            const uint16_t calc = firecode_wave(L.sf + 2, lane);
            good = (rx == calc);
            res.firecode_ok = good ? 1 : 0;
            res.firecode_rx_calc = ((uint32_t)rx << 16) | calc;
        }
        if (!good) {
            st.desync_count++;
        } else {
            st.desync_count = 0;
            st.synced = 1;
            const int descriptor = L.sf[2];
            const int dac_rate = (descriptor >> 6) & 1, sbr = (descriptor >> 5) & 1;
            res.header_valid = 1;
            res.descriptor = descriptor;
            const int num_aus = dac_rate ? (sbr ? 3 : 6) : (sbr ? 2 : 4);
            res.num_aus = num_aus;
            int bit = 0;
#pragma unroll
            for (int a = 1; a < 6; a++) {
                if (a < num_aus) {
                    int v = 0;
                    for (int b = 0; b < 12; b++, bit++) v = (v << 1) | ((L.sf[3 + (bit >> 3)] >> (7 - (bit & 7))) & 1);
                    res.au_start[a] = v;
                }
            }
            res.au_start[0] = 3 + ((bit + 7) >> 3);
#pragma unroll
            for (int a = 2; a <= 6; a++) if (a == num_aus) res.au_start[a] = 110 * n_rs;
            // the walk stops at the first access unit that fails the bounds test (:291-297)
            int stop = -1;
#pragma unroll
            for (int a = 5; a >= 0; a--) {
                if (a < num_aus) {
                    const int nb_data = res.au_start[a + 1] - res.au_start[a] - 2;
                    if (nb_data < 0 || res.au_start[a + 1] >= sf_bytes) stop = a;
                }
            }
            res.au_walk_stopped_at = stop;
            const int walked = (stop < 0) ? num_aus : stop;
            // access-unit CRCs (x^16+x^12+x^5+1, start value 0xFFFF, inverted), each unit shared by 32 / 16 / 8 lanes
            if (lane == 0) L.flags[0] = 0;
            if (lane == 0) {
#pragma unroll
                for (int a = 0; a <= 6; a++) L.au[a] = res.au_start[a];
            }
            __syncthreads();
            {
                const int lg = (num_aus <= 2) ? 5 : (num_aus <= 4) ? 4 : 3, per = 1 << lg;
                const int a = lane >> lg, q = lane & (per - 1);
                const bool mine = a < walked;
                const int a0 = mine ? L.au[a] : 0, nb_data = mine ? (L.au[a + 1] - a0 - 2) : 0;
                const uint16_t crc = au_crc_lanes([&](int k) { return (uint32_t)L.sf[a0 + k]; }, nb_data, L.crc_tab, lg, q);
                if (mine && q == per - 1) {
                    const uint16_t rx = (uint16_t)((L.sf[a0 + nb_data] << 8) | L.sf[a0 + nb_data + 1]);
                    if (rx == crc) atomicOr(&L.flags[0], 1 << a);
                    L.syn[2 * a] = (uint8_t)(crc >> 8); L.syn[2 * a + 1] = (uint8_t)(crc & 0xFF);       // syndromes are done with
                }
            }
            __syncthreads();
            res.au_crc_ok_mask = (uint32_t)L.flags[0];
#pragma unroll
            for (int a = 0; a < 6; a++) if (a < walked) res.au_crc_calc[a] = (uint16_t)((L.syn[2 * a] << 8) | L.syn[2 * a + 1]);
        }
        // hand the (corrected) super frame and its record to the caller
        if (n_sf < max_sf) {
            uint8_t* out = sf_out + ((size_t)s * max_sf + n_sf) * sf_out_stride;
            for (int k = lane; k < sf_bytes; k += 64) out[k] = L.sf[k];
            if (lane == 0) results[(size_t)s * max_sf + n_sf] = res;
        }
        n_sf++;
        __syncthreads();
    }
    if (lane == 0) {
        states[s] = st;
        counts[4 * s] = n_sf;
        counts[4 * s + 1] = n_wait_failed;
        counts[4 * s + 2] = last_wait_crc;
        counts[4 * s + 3] = st.curr_dab_frame;
    }
}

}  // namespace dabgpu

using namespace dabgpu;

struct dabgpu_dabplus_bank {
    dabgpu_ctx* ctx = nullptr;
    size_t n = 0;
    DeviceBuffer<DpState> d_states;
    DeviceBuffer<uint8_t> d_acc;
    // single-stream host-buffer path
    DeviceBuffer<uint8_t> d_frame; DeviceBuffer<unsigned long long> d_off; DeviceBuffer<uint32_t> d_n;
    DeviceBuffer<uint8_t> d_sf; DeviceBuffer<dabgpu_superframe_result> d_res; DeviceBuffer<int32_t> d_counts;   // d_counts [4]
};

extern "C" {

void dabgpu_dabplus_bank_destroy(dabgpu_dabplus_bank* b) {
    if (!dabgpu_destroy_begin(b, b ? b->ctx : nullptr)) return;
    delete b;
}

int dabgpu_dabplus_bank_reset(dabgpu_dabplus_bank* b, void* stream) {
    if (!b) { dabgpu_set_error("dabplus_bank_reset: null bank"); return DABGPU_ERR_INVALID_ARG; }
    DABGPU_BIND(b->ctx);
    // AAC_Frame_Processor's constructor state (:121-125): WAIT_FRAME_START, nothing collected, unsynchronised
    std::vector<DpState> init(b->n, DpState{1, 0, 0, 0, 0});
    int st = dabgpu_check_hip(hipMemcpyAsync(b->d_states.get(), init.data(), b->n * sizeof(DpState), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync");
    if (st) return st;
    return dabgpu_check_hip(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
}

int dabgpu_dabplus_bank_create(dabgpu_ctx* c, size_t n_streams, dabgpu_dabplus_bank** out) {
    if (!c || !out || n_streams == 0 || n_streams > (size_t)(1 << 22)) { dabgpu_set_error("dabplus_bank_create: invalid argument"); return DABGPU_ERR_INVALID_ARG; }
    *out = nullptr;
    DABGPU_BIND(c);
    dabgpu_dabplus_bank* b = new (std::nothrow) dabgpu_dabplus_bank();
    if (!b) return DABGPU_ERR_HIP;
    b->ctx = c; b->n = n_streams;
    const char* what = "hipMalloc(dabplus bank)";
    int st = b->d_states.alloc(n_streams, what);
    if (!st) st = b->d_acc.alloc(n_streams * (size_t)DP_MAX_SF, what);
    if (!st) st = b->d_frame.alloc(DP_MAX_FRAME_BYTES, what);
    if (!st) st = b->d_off.alloc(1, what);
    if (!st) st = b->d_n.alloc(1, what);
    if (!st) st = b->d_sf.alloc(DP_MAX_SF, what);
    if (!st) st = b->d_res.alloc(1, what);
    if (!st) st = b->d_counts.alloc(4, what);
    if (!st) st = dabgpu_check_hip(hipMemsetAsync(b->d_off.get(), 0, sizeof(unsigned long long), c->stream), "hipMemsetAsync");
    if (!st) st = dabgpu_dabplus_bank_reset(b, c->stream);
    if (st) { dabgpu_dabplus_bank_destroy(b); return st; }
    *out = b;
    return DABGPU_OK;
}

int dabgpu_dabplus_bank_process(dabgpu_dabplus_bank* b, const uint8_t* d_frames, const uint64_t* d_stream_offsets, size_t frame_stride_bytes,
                                const uint32_t* d_frame_bytes, int n_frames, uint8_t* d_superframes, size_t superframe_stride_bytes,
                                dabgpu_superframe_result* d_results, int max_superframes, int32_t* d_counts, void* stream) {
    return dabgpu_dabplus_bank_process_masked(b, d_frames, d_stream_offsets, frame_stride_bytes, d_frame_bytes, n_frames, d_superframes,
                                              superframe_stride_bytes, d_results, max_superframes, d_counts, nullptr, 1, stream);
}

int dabgpu_dabplus_bank_process_masked(dabgpu_dabplus_bank* b, const uint8_t* d_frames, const uint64_t* d_stream_offsets, size_t frame_stride_bytes,
                                       const uint32_t* d_frame_bytes, int n_frames, uint8_t* d_superframes, size_t superframe_stride_bytes,
                                       dabgpu_superframe_result* d_results, int max_superframes, int32_t* d_counts,
                                       const int32_t* d_active, int streams_per_flag, void* stream) {
    if (!b || !d_frames || !d_stream_offsets || !d_frame_bytes || !d_superframes || !d_results || !d_counts) {
        dabgpu_set_error("dabplus_bank_process: null argument"); return DABGPU_ERR_INVALID_ARG;
    }
    if (streams_per_flag < 1) { dabgpu_set_error("dabplus_bank_process_masked: streams_per_flag must be positive"); return DABGPU_ERR_INVALID_ARG; }
    if (n_frames <= 0) return DABGPU_OK;
    if (max_superframes < (n_frames + 4) / 5 || superframe_stride_bytes == 0) {
        dabgpu_set_error("dabplus_bank_process: max_superframes must be at least ceil(n_frames / 5)"); return DABGPU_ERR_INVALID_ARG;
    }
    DABGPU_BIND(b->ctx);
    hipLaunchKernelGGL(dabplus_kernel, dim3((unsigned)b->n), dim3(64), 0, (hipStream_t)stream, b->d_states.get(), d_frames,
                       reinterpret_cast<const unsigned long long*>(d_stream_offsets), frame_stride_bytes, d_frame_bytes, n_frames, b->d_acc.get(),
                       d_superframes, superframe_stride_bytes, d_results, max_superframes, d_counts, (int)b->n, d_active, streams_per_flag);
    return dabgpu_check_hip(hipGetLastError(), "dabplus_kernel launch");
}

int dabgpu_dabplus_process_frame_host_sync(dabgpu_dabplus_bank* b, const uint8_t* h_frame, uint32_t n_bytes, int* superframe_done,
                                           int* firecode_wait_failed, uint32_t* firecode_wait_rx_calc, dabgpu_superframe_result* h_result,
                                           uint8_t* h_superframe) {
    if (!b || !h_frame || !superframe_done || !firecode_wait_failed || !h_result || !h_superframe) {
        dabgpu_set_error("dabplus_process_frame_host_sync: null argument"); return DABGPU_ERR_INVALID_ARG;
    }
    if (b->n != 1) { dabgpu_set_error("dabplus_process_frame_host_sync: needs a bank of one stream"); return DABGPU_ERR_INVALID_ARG; }
    *superframe_done = 0; *firecode_wait_failed = 0;
    if (n_bytes > (uint32_t)DP_MAX_FRAME_BYTES) {
        dabgpu_set_error("dabplus_process_frame_host_sync: logical frames of %u bytes are not supported (<= %d)", n_bytes, DP_MAX_FRAME_BYTES);
        return DABGPU_ERR_UNSUPPORTED;
    }
    dabgpu_ctx* c = b->ctx;
    DABGPU_BIND(c);
    DABGPU_HOST_LOCK(b->ctx);
    hipStream_t s = c->stream;
    int st;
    DABGPU_CK(hipMemcpyAsync(b->d_frame.get(), h_frame, n_bytes, hipMemcpyHostToDevice, s));
    DABGPU_CK(hipMemcpyAsync(b->d_n.get(), &n_bytes, sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if ((st = dabgpu_dabplus_bank_process(b, b->d_frame.get(), reinterpret_cast<const uint64_t*>(b->d_off.get()), 0, b->d_n.get(), 1, b->d_sf.get(), DP_MAX_SF, b->d_res.get(), 1,
                                          b->d_counts.get(), s))) return st;
    int32_t counts[4];
    DABGPU_CK(hipMemcpyAsync(counts, b->d_counts.get(), sizeof(counts), hipMemcpyDeviceToHost, s));
    DABGPU_CK(hipStreamSynchronize(s));
    *superframe_done = counts[0];
    *firecode_wait_failed = counts[1];
    if (firecode_wait_rx_calc) *firecode_wait_rx_calc = (uint32_t)counts[2];
    if (counts[0]) {
        DABGPU_CK(hipMemcpyAsync(h_result, b->d_res.get(), sizeof(dabgpu_superframe_result), hipMemcpyDeviceToHost, s));
        DABGPU_CK(hipMemcpyAsync(h_superframe, b->d_sf.get(), 5 * (size_t)n_bytes, hipMemcpyDeviceToHost, s));
        DABGPU_CK(hipStreamSynchronize(s));
    }
    return DABGPU_OK;
}

}  // extern "C"
