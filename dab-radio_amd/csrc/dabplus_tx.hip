// dabplus_tx.hip -- the DAB+ super-frame encoder on the device (include/dabgpu.h, "DAB+ super-frame encoder"): access units -> the bytes of a
// DAB+ sub-channel, ETSI TS 102 563 clauses 5.2 and 6 in the transmit direction.  The inverse of dabplus.hip's clean path; what it writes is
// what AAC_Frame_Processor (src/dab/audio/aac_frame_processor.cpp:201-320) takes apart again.
//
// One wavefront (a 64-thread workgroup) per super frame, the super frame in LDS:
//   1. layout: every lane evaluates dabgpu_dabplus_layout (dabgpu_host_logic.h, the host entry point's body) on wave-uniform inputs;
//   2. fill: header bytes 2.., then the access units copied from global memory, 64 consecutive bytes per load;
//   3. access-unit CRCs: 32 / 16 / 8 lanes per unit for 2 / 3-4 / 6 units, each lane a chunk, the chunks joined by crc_mulmod
//      (au_crc_lanes, which dabplus.hip's check calls too), here writing the two bytes instead of comparing them;
//   4. fire code of bytes 2..10 (firecode_wave);
//   5. RS parity.  The ten parity bytes are linear in the data bytes: data byte j of a code word contributes d_j x^(119 - j) mod g(x), ten
//      bytes whose logarithms are a row of a constant table (rs_core.h makes it, for packet_fec.hip's code too).  A code word is dealt to
//      `per` lanes, lane (i, q) adds the contributions of symbols q, q + per, ... of code word i (1 + 1 + 10 LDS look-ups per symbol: the
//      byte, its logarithm and the table row in one 16-byte read, ten antilogarithms), and the shares are folded by XOR into three LDS
//      words per code word.  n_rs x per work items are walked 64 at a time: per = 64 / n_rs up to 32 code words (one pass, at least 33
//      lanes busy), 128 / n_rs from 33 on (two passes of at most 55 symbols instead of one of 110 with half the wavefront idle);
//   6. the 120 n_rs bytes leave LDS as dwords, frame by frame (frame sizes, offsets and the stride are multiples of 4).
// A super frame the layout refuses writes zeros and its code.  Integer / byte work, bit-exact by construction.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "dabplus_common.h"

namespace dabgpu {

// the parity map of RS(120,110) (rs_core.h).  No coefficient is zero, so no row needs its "no contribution" mark
constexpr rs::ParityTab<RS_DATA, RS_ROOTS> RS_PARITY_TAB_HOST = rs::make_parity_tab<RS_DATA, RS_ROOTS>();
static_assert(RS_PARITY_TAB_HOST.all_nonzero, "a zero coefficient would need its mark read");
static __constant__ rs::ParityTab<RS_DATA, RS_ROOTS> RS_PARITY_TAB = rs::make_parity_tab<RS_DATA, RS_ROOTS>();

struct TxLds {
    alignas(16) uint8_t par_log[RS_DATA][16];
    alignas(16) uint8_t sf[DP_MAX_SF];
    uint8_t exp[512];
    uint8_t log[256];
    uint16_t crc_tab[256];
    uint32_t par[64][3];             // parity of code word i: bytes 0-3 | 4-7 | 8-9, byte r in bits 8 (r % 4) ..
    int au[8];                       // access-unit starts
};

__global__ __launch_bounds__(64)
void dabplus_tx_kernel(const uint8_t* __restrict__ au_bytes, const unsigned long long* __restrict__ au_offsets, const uint16_t* __restrict__ au_len,
                       const uint8_t* __restrict__ descriptors, const uint32_t* __restrict__ frame_bytes, uint8_t* __restrict__ frames,
                       const unsigned long long* __restrict__ stream_offsets, size_t frame_stride, int32_t* __restrict__ status, int n_superframes)
{
    __shared__ TxLds L;
    const int lane = threadIdx.x;
    const size_t item = blockIdx.x;                         // (stream, super frame)
    const size_t s = item / (size_t)n_superframes, k = item % (size_t)n_superframes;
    const uint32_t n = frame_bytes[s];
    const uint32_t descriptor = descriptors[item];
    uint16_t len[6];
#pragma unroll
    for (int a = 0; a < 6; a++) len[a] = au_len[item * 6 + a];
    uint32_t start[7], n_rs;
    int num_aus;
    const int st = dabgpu_dabplus_layout(n, descriptor, len, start, &num_aus, &n_rs);
    uint8_t* out = frames + stream_offsets[s] + 5 * k * frame_stride;
    if (lane == 0) status[item] = st;
    if (st != 0) {
        const uint32_t nz = (n < (uint32_t)DP_MAX_FRAME_BYTES) ? n : (uint32_t)DP_MAX_FRAME_BYTES;
        for (int j = 0; j < 5; j++)
            for (uint32_t b = lane; b < nz; b += 64) out[(size_t)j * frame_stride + b] = 0;
        return;
    }
    // tables
    load_gf_crc_tables(L, lane);
    for (int i = lane; i < RS_DATA; i += 64)
        *reinterpret_cast<uint4*>(L.par_log[i]) = *reinterpret_cast<const uint4*>(RS_PARITY_TAB.log_coef[i]);
    for (int i = lane; i < 64 * 3; i += 64) (&L.par[0][0])[i] = 0;
    if (lane < 7) {
        int v = 0;
#pragma unroll
        for (int a = 0; a < 7; a++) if (lane == a) v = (int)start[a];
        L.au[lane] = v;
    }
    // header: descriptor, then the 12-bit starts of units 1 .. num_aus - 1, MSB first, zero padded to whole bytes (at most 60 bits)
    if (lane >= 2 && lane < (int)start[0]) {
        unsigned long long w = 0;
#pragma unroll
        for (int a = 1; a < 6; a++) if (a < num_aus) w |= (unsigned long long)start[a] << (64 - 12 * a);
        L.sf[lane] = (lane == 2) ? (uint8_t)descriptor : (uint8_t)(w >> (8 * (10 - lane)));          // lane <= 10: start[0] <= 11
    }
    // access units
    const uint8_t* src = au_bytes + au_offsets[item];
#pragma unroll
    for (int a = 0; a < 6; a++) {
        if (a < num_aus) {
            for (uint32_t b = lane; b < (uint32_t)len[a]; b += 64) L.sf[start[a] + b] = src[b];
            src += len[a];
        }
    }
    __syncthreads();
    // CRCs behind the units
    {
        const int lg = (num_aus <= 2) ? 5 : (num_aus <= 4) ? 4 : 3, per = 1 << lg;
        const int a = lane >> lg, q = lane & (per - 1);
        const bool mine = a < num_aus;
        const int a0 = mine ? L.au[a] : 0, nb_data = mine ? (L.au[a + 1] - a0 - 2) : 0;
        const uint16_t crc = au_crc_lanes([&](int k) { return (uint32_t)L.sf[a0 + k]; }, nb_data, L.crc_tab, lg, q);
        if (mine && q == per - 1) { L.sf[a0 + nb_data] = (uint8_t)(crc >> 8); L.sf[a0 + nb_data + 1] = (uint8_t)(crc & 0xFFu); }
    }
    __syncthreads();
    {
        const uint16_t fire = firecode_wave(L.sf + 2, lane);
        if (lane < 2) L.sf[lane] = (uint8_t)(lane ? (fire & 0xFFu) : (fire >> 8));
    }
    __syncthreads();
    // parity
    {
        uint32_t per = ((n_rs <= 32u) ? 64u : 128u) / n_rs;
        if (per > (uint32_t)RS_DATA) per = RS_DATA;
        const uint32_t items = n_rs * per;
        for (uint32_t w = lane; w < items; w += 64) {
            const uint32_t q = w / n_rs, i = w - q * n_rs;
            uint32_t pw[3] = {0, 0, 0};
            for (uint32_t j = q; j < (uint32_t)RS_DATA; j += per) {
                const uint32_t d = L.sf[i + j * n_rs];
                if (d) {
                    const uint32_t ld = L.log[d];
                    const uint4 row = *reinterpret_cast<const uint4*>(L.par_log[j]);
                    const uint32_t rw[4] = {row.x, row.y, row.z, row.w};
                    rs::parity_add<RS_ROOTS>(L, ld, rw, 0u, pw);
                }
            }
#pragma unroll
            for (int k = 0; k < 3; k++) atomicXor(&L.par[i][k], pw[k]);
        }
    }
    __syncthreads();
    for (uint32_t w = lane; w < n_rs * RS_ROOTS; w += 64) {                 // parity byte r of code word i sits at i + (110 + r) n_rs
        const uint32_t r = w / n_rs, i = w - r * n_rs;
        L.sf[RS_DATA * n_rs + w] = (uint8_t)(L.par[i][r >> 2] >> (8 * (r & 3)));
    }
    __syncthreads();
    if (((uintptr_t)out & 3) == 0) {
        const uint32_t fw = n / 4;                                          // dwords per logical frame
        for (uint32_t j = 0; j < 5; j++)
            for (uint32_t p = lane; p < fw; p += 64)
                reinterpret_cast<uint32_t*>(out + (size_t)j * frame_stride)[p] = reinterpret_cast<const uint32_t*>(L.sf)[j * fw + p];
    } else {
        // a stream offset that is no multiple of 4 breaks the documented precondition; it lives on the device, so the host cannot refuse
        // it: the same bytes, stored one by one
        for (uint32_t j = 0; j < 5; j++)
            for (uint32_t p = lane; p < n; p += 64) out[(size_t)j * frame_stride + p] = L.sf[j * n + p];
    }
}

}  // namespace dabgpu

using namespace dabgpu;

static int dabplus_tx_check(const char* who, const dabgpu_ctx* c, size_t n_streams, int n_superframes, bool pointers_ok, const void* frames,
                            size_t frame_stride) {
    if (!c) { dabgpu_set_error("%s: null context", who); return DABGPU_ERR_INVALID_ARG; }
    if (n_superframes < 0) { dabgpu_set_error("%s: n_superframes = %d", who, n_superframes); return DABGPU_ERR_INVALID_ARG; }
    if ((frame_stride & 3) || ((uintptr_t)frames & 3)) {
        dabgpu_set_error("%s: the frames and their stride must be multiples of 4 bytes", who); return DABGPU_ERR_INVALID_ARG;
    }
    if (n_streams == 0 || n_superframes == 0) return DABGPU_OK;
    if (n_streams > ((size_t)1 << 30) / (size_t)n_superframes) {
        dabgpu_set_error("%s: too many super frames (streams x super frames <= 2^30)", who); return DABGPU_ERR_INVALID_ARG;
    }
    if (!pointers_ok) { dabgpu_set_error("%s: null argument", who); return DABGPU_ERR_INVALID_ARG; }
    return DABGPU_OK;
}

extern "C" {

int dabgpu_dabplus_tx_encode(dabgpu_ctx* c, size_t n_streams, int n_superframes, const uint8_t* d_au_bytes, const uint64_t* d_au_offsets,
                             const uint16_t* d_au_len, const uint8_t* d_descriptor, const uint32_t* d_frame_bytes, uint8_t* d_frames,
                             const uint64_t* d_stream_offsets, size_t frame_stride_bytes, int32_t* d_status, void* stream) {
    const bool ptrs = d_au_bytes && d_au_offsets && d_au_len && d_descriptor && d_frame_bytes && d_frames && d_stream_offsets && d_status;
    const int st = dabplus_tx_check("dabplus_tx_encode", c, n_streams, n_superframes, ptrs, d_frames, frame_stride_bytes);
    if (st || n_streams == 0 || n_superframes == 0) return st;
    DABGPU_BIND(c);
    hipLaunchKernelGGL(dabplus_tx_kernel, dim3((unsigned)(n_streams * (size_t)n_superframes)), dim3(64), 0, (hipStream_t)stream, d_au_bytes,
                       reinterpret_cast<const unsigned long long*>(d_au_offsets), d_au_len, d_descriptor, d_frame_bytes, d_frames,
                       reinterpret_cast<const unsigned long long*>(d_stream_offsets), frame_stride_bytes, d_status, n_superframes);
    return dabgpu_check_hip(hipGetLastError(), "dabplus_tx_kernel launch");
}

int dabgpu_dabplus_tx_encode_host_sync(dabgpu_ctx* c, int n_superframes, const uint8_t* h_au_bytes, const uint64_t* h_au_offsets,
                                       const uint16_t* h_au_len, const uint8_t* h_descriptor, uint32_t frame_bytes, uint8_t* h_frames,
                                       int32_t* h_status) {
    const bool ptrs = h_au_bytes && h_au_offsets && h_au_len && h_descriptor && h_frames && h_status;
    int st = dabplus_tx_check("dabplus_tx_encode_host_sync", c, 1, n_superframes, ptrs, nullptr, 0);
    if (st || n_superframes == 0) return st;
    const size_t K = (size_t)n_superframes;
    // a frame size the layout refuses is known here: the device form's answer for it, without a device buffer of that size
    if (frame_bytes < 24u || frame_bytes > (uint32_t)DP_MAX_FRAME_BYTES || frame_bytes % 24u) {
        for (size_t k = 0; k < K; k++) h_status[k] = DABGPU_DABPLUS_TX_BAD_FRAME_SIZE;
        for (size_t f = 0; f < 5 * K; f++) memset(h_frames + f * (size_t)frame_bytes, 0, std::min<size_t>(frame_bytes, DP_MAX_FRAME_BYTES));
        return DABGPU_OK;
    }
    // bytes of h_au_bytes the call reads: the units the descriptors announce (a length beyond num_aus is not looked at)
    size_t au_total = 0;
    for (size_t k = 0; k < K; k++) {
        const int dac_rate = (h_descriptor[k] >> 6) & 1, sbr = (h_descriptor[k] >> 5) & 1, na = dac_rate ? (sbr ? 3 : 6) : (sbr ? 2 : 4);
        size_t end = (size_t)h_au_offsets[k];
        for (int a = 0; a < na; a++) end += h_au_len[6 * k + a];
        // a super frame whose lengths do not fill it is refused on the device and its bytes are never read
        uint32_t start[7], n_rs; int num_aus;
        if (dabgpu_dabplus_layout(frame_bytes, h_descriptor[k], h_au_len + 6 * k, start, &num_aus, &n_rs) == 0) au_total = std::max(au_total, end);
    }
    DABGPU_BIND(c);
    DABGPU_HOST_LOCK(c);
    hipStream_t s = c->stream;
    // one block up: offsets [K] | stream offset | frame bytes, pad | lengths [K][6] | descriptors [K], pad to 16 | access units
    const size_t off_len = 8 * K + 16, off_desc = off_len + 12 * K, off_au = (off_desc + K + 15) & ~(size_t)15;
    const size_t frames_bytes = 5 * K * (size_t)frame_bytes, up_bytes = off_au + au_total + 16, down_bytes = frames_bytes + 4 * K;
    std::vector<uint8_t> up(up_bytes, 0), down(down_bytes);         // one copy each way: the inputs; frames | status
    memcpy(up.data(), h_au_offsets, 8 * K);
    memcpy(up.data() + 8 * K + 8, &frame_bytes, 4);
    memcpy(up.data() + off_len, h_au_len, 12 * K);
    memcpy(up.data() + off_desc, h_descriptor, K);
    if (au_total) memcpy(up.data() + off_au, h_au_bytes, au_total);
    void *d_in, *d_out;
    if ((st = dabgpu_scratch(c, SCR_CONVERT_IN, up_bytes, &d_in))) return st;
    if ((st = dabgpu_scratch(c, SCR_CONVERT_OUT, down_bytes, &d_out))) return st;
    uint8_t* di = static_cast<uint8_t*>(d_in);
    uint8_t* dout = static_cast<uint8_t*>(d_out);
    DABGPU_CK(hipMemcpyAsync(d_in, up.data(), up_bytes, hipMemcpyHostToDevice, s));       // (`up` outlives the synchronise below)
    st = dabgpu_dabplus_tx_encode(c, 1, n_superframes, di + off_au, reinterpret_cast<const uint64_t*>(di), reinterpret_cast<const uint16_t*>(di + off_len),
                                  di + off_desc, reinterpret_cast<const uint32_t*>(di + 8 * K + 8), dout, reinterpret_cast<const uint64_t*>(di + 8 * K),
                                  frame_bytes, reinterpret_cast<int32_t*>(dout + frames_bytes), s);
    if (st) return st;
    DABGPU_CK(hipMemcpyAsync(down.data(), dout, down_bytes, hipMemcpyDeviceToHost, s));
    DABGPU_CK(hipStreamSynchronize(s));
    memcpy(h_frames, down.data(), frames_bytes);
    memcpy(h_status, down.data() + frames_bytes, 4 * K);
    return DABGPU_OK;
}

}  // extern "C"
