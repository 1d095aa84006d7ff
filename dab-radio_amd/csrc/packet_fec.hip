// packet_fec.hip -- MSC packet mode and its FEC scheme on the device, both directions (include/dabgpu.h, "MSC packet mode"; EN 300 401
// clauses 5.3.2 and 5.3.5).  The packet and ring arithmetic both kernels share with the host is in packet_fec_core.h.
//
// Receive (packet_kernel): what MSC_Reed_Solomon_Data_Packet_Processor does (src/dab/msc/msc_reed_solomon_data_packet_processor.cpp), one
// wavefront per stream.  The stream's ring lives in HBM between calls and in LDS during one; logical frames are staged through an LDS
// window so that the walk's dependent header reads cost an LDS access.  The walk is wave-uniform: every lane takes the same branch, the
// copies are dealt over the lanes.  At the ninth FEC packet of a full ring the 12 rows of RS(204,188) are decoded in place:
//   syndromes   lane = share * 16 + row: rows 0..11 of each group of 16 lanes, four shares of 51 symbols each, all sixteen roots per
//               symbol as independent table look-ups (no Horner chain), the roots packed in four words and folded by XOR shuffles over
//               16 and 32; a frame whose 192 syndromes are zero skips everything below
//   locator     Berlekamp-Massey, one lane per row with a non-zero syndrome, its polynomials in LDS
//   roots       Chien search and Forney's formula dealt over 60 lanes: five per row, 51 candidates each; the roots of a row are only
//               applied once their number is known to equal the locator's degree (reed_solomon_decoder.cpp:412-419), to positions
//               0..187 alone (msc_reed_solomon_data_packet_processor.cpp:232-247)
// Packets handed out are copied from the ring by all lanes; their CRCs are computed eight packets at a time, eight lanes per packet, each
// lane a chunk joined by crc_mulmod (crc_lanes, as for DAB+'s access units).  Field, syndromes and parity map: rs_core.h, as for DAB+.
//
// Transmit (packet_tx_kernel): one wavefront per (stream, FEC frame): the frame's packets are built in LDS from the planner's table
// (headers, data, zero padding, CRC), the 12 x 16 parity bytes are linear maps of the 188 row symbols through a constant 188 x 16 table of
// the logarithms of x^(203 - j) mod g(x) (five lanes per row, folded by LDS XOR), the nine FEC packets follow, and the 2472 bytes leave
// through the logical-frame mapping.  Integer / byte work, bit-exact by construction.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <vector>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "packet_fec_core.h"
#include "rs_device.h"

namespace dabgpu {
using namespace pkt;

constexpr int PK_ROOTS = RS_PARITY_BYTES;
constexpr int PK_WINDOW = 1536;                          // bytes of a logical frame staged at once (any frame size is walked through it)
static_assert(PK_WINDOW >= 96 && RING_BYTES % 4 == 0, "the window holds a whole packet; the ring moves as dwords");

struct PkState {                     // per stream, persistent (the ring itself beside it)
    int read, write, size, last_counter, discarded_packets, discarded_bytes, reserved[2];
};

struct PkLds {
    alignas(16) uint8_t ring[RING_BYTES];
    alignas(16) uint8_t win[PK_WINDOW];
    uint8_t exp[512];
    uint8_t log[256];
    uint16_t crc_tab[256];
    uint16_t pk_off[MAX_RING_PACKETS + 1];               // packets of one hand-out: byte offsets behind the read head
    uint8_t syn[RS_ROWS * PK_ROOTS];
    uint8_t lam[RS_ROWS][PK_ROOTS + 4];                  // error locator C_0..C_16
    uint8_t bm_b[RS_ROWS][PK_ROOTS + 4], bm_t[RS_ROWS][PK_ROOTS + 4];
    uint8_t omega[RS_ROWS][PK_ROOTS];
    int rec[RS_ROWS];                                    // degree | roots found << 8
    uint16_t fix[RS_ROWS][PK_ROOTS];                     // per root found: location | error value << 8 (0 where none is applied)
    int8_t rs_count[RS_ROWS];
};

// Berlekamp-Massey for row i, then omega = S C mod x^16: rs::locator's algorithm with run-time trip counts over polynomials in LDS (the
// shared body, unrolled for register arrays, costs this kernel its occupancy).  No host build runs this copy: tests/test_gpu_rs_structured.py holds it to the reference's records.
__device__ void pk_locator(PkLds& L, int i) {
    const uint8_t* S = &L.syn[i * PK_ROOTS];
    uint8_t *C = L.lam[i], *B = L.bm_b[i], *T = L.bm_t[i];
    for (int k = 0; k <= PK_ROOTS; k++) { C[k] = (k == 0); B[k] = (k == 0); }
    int len = 0;
    for (int r = 1; r <= PK_ROOTS; r++) {
        uint8_t d = 0;
        for (int k = 0; k < r; k++) d ^= rs::mul(L, C[k], S[r - 1 - k]);
        if (d == 0) {
            for (int k = PK_ROOTS; k > 0; k--) B[k] = B[k - 1];
            B[0] = 0;
        } else {
            T[0] = C[0];
            for (int k = 0; k < PK_ROOTS; k++) T[k + 1] = (uint8_t)(C[k + 1] ^ rs::mul(L, d, B[k]));
            if (2 * len <= r - 1) {
                len = r - len;
                for (int k = 0; k <= PK_ROOTS; k++) B[k] = rs::div(L, C[k], d);
            } else {
                for (int k = PK_ROOTS; k > 0; k--) B[k] = B[k - 1];
                B[0] = 0;
            }
            for (int k = 0; k <= PK_ROOTS; k++) C[k] = T[k];
        }
    }
    int deg = 0;
    for (int k = 0; k <= PK_ROOTS; k++) if (C[k]) deg = k;
    for (int a = 0; a < PK_ROOTS; a++) {
        uint8_t t = 0;
        for (int b = 0; b <= a; b++) t ^= rs::mul(L, S[a - b], C[b]);
        L.omega[i][a] = t;
    }
    L.rec[i] = deg;
}

// Chien search over candidates x0..x1 of row i and Forney's value of every root found, with run-time trip counts likewise
__device__ void pk_search(PkLds& L, int i, int x0, int x1) {
    const int deg = L.rec[i] & 0xFF;
    if (deg == 0) return;
    const uint8_t* C = L.lam[i];
    const uint8_t* omega = L.omega[i];
    for (int x = x0; x <= x1; x++) {
        uint8_t v = 1;
        for (int k = 1; k <= deg; k++) if (C[k]) v ^= L.exp[(L.log[C[k]] + k * x) % 255];
        if (v) continue;
        const int slot = (atomicAdd(&L.rec[i], 0x100) >> 8) & (PK_ROOTS - 1);     // a locator of degree <= 16 has at most 16 roots
        const int loc = x - 1;
        uint8_t num1 = 0, den = 0;
        for (int a = 0; a < deg; a++) num1 ^= rs::mul(L, omega[a], rs::pow(L, a * x));
        const uint8_t num2 = rs::pow(L, -x);                                        // first root alpha^0
        const int top = ((deg < PK_ROOTS - 1) ? deg : (PK_ROOTS - 1)) & ~1;
        for (int a = 0; a <= top; a += 2) den ^= rs::mul(L, C[a + 1], rs::pow(L, a * x));
        const uint8_t val = (num1 != 0 && loc >= RS_PADDING) ? rs::div(L, rs::mul(L, num1, num2), den) : (uint8_t)0;
        L.fix[i][slot] = (uint16_t)(loc | (val << 8));
    }
}

// PerformReedSolomonCorrection's rows (:186-248) on the full ring whose read head is rd; leaves Decode's return values in L.rs_count
__device__ void pk_correct_rows(PkLds& L, int rd, int lane) {
    {
        const int row = lane & 15, share = lane >> 4;
        uint32_t w[4] = {0, 0, 0, 0};
        if (row < RS_ROWS) {
            for (int j = share * 51; j < share * 51 + 51; j++)
                rs::syndrome_add<RS_MESSAGE_BYTES, PK_ROOTS>(L, L.ring[ring_at(rd, row_symbol_offset(row, j))], j, w);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            w[k] ^= (uint32_t)__shfl_xor((int)w[k], 16);
            w[k] ^= (uint32_t)__shfl_xor((int)w[k], 32);
        }
        if (share == 0 && row < RS_ROWS) {
#pragma unroll
            for (int r = 0; r < PK_ROOTS; r++) L.syn[row * PK_ROOTS + r] = rs::packed_byte<PK_ROOTS>(w, r);
        }
    }
    __syncthreads();
    int any = 0;
    if (lane < RS_ROWS) {
        for (int r = 0; r < PK_ROOTS; r++) any |= L.syn[lane * PK_ROOTS + r];
        L.rs_count[lane] = 0;
    }
    if (!__any(any != 0)) { __syncthreads(); return; }
    if (lane < RS_ROWS) {
        if (any) pk_locator(L, lane);
        else L.rec[lane] = 0;
    }
    __syncthreads();
    if (lane < 5 * RS_ROWS) {
        const int i = lane % RS_ROWS, q = lane / RS_ROWS;
        pk_search(L, i, 1 + 51 * q, 51 + 51 * q);
    }
    __syncthreads();
    if (lane < RS_ROWS) {
        const int w = L.rec[lane], deg = w & 0xFF, found = w >> 8;
        L.rs_count[lane] = (int8_t)((found == deg) ? deg : -1);
    }
    for (int idx = lane; idx < RS_ROWS * PK_ROOTS; idx += 64) {
        const int i = idx / PK_ROOTS, slot = idx % PK_ROOTS;
        const int w = L.rec[i], deg = w & 0xFF, found = w >> 8;
        if (found == deg && slot < found) {
            const int fx = L.fix[i][slot], x = (fx & 0xFF) - RS_PADDING, val = fx >> 8;
            if (val && x >= 0 && x < RS_DATA_BYTES) L.ring[ring_at(rd, x * RS_ROWS + i)] ^= (uint8_t)val;
        }
    }
    __syncthreads();
}

struct PkOut {
    uint8_t* packets; size_t capacity;
    dabgpu_packet_record* records; int max_records;
    int n_packets, n_bytes;
};

// PopRingBuffer + callback (:123-130, :161-176, :250-256): packets leave the head of the ring while it holds any and fewer than `limit`
// bytes have left.  Wave-uniform.
__device__ void pk_hand_out(PkLds& L, PkState& st, int limit, int corrected, PkOut& o, int lane) {
    int np = 0, total = 0;
    while (total < st.size && total < limit && np < MAX_RING_PACKETS) {
        const int len = packet_length(L.ring[ring_at(st.read, total)] >> 6);
        if (lane == 0) L.pk_off[np] = (uint16_t)total;
        np++;
        total += len;
    }
    if (total > RING_BYTES) total = RING_BYTES;              // (cannot happen with a ring this kernel filled)
    if (lane == 0) L.pk_off[np] = (uint16_t)total;
    __syncthreads();
    const int rd = st.read;
    for (int k = lane; k < total; k += 64)
        if ((size_t)(o.n_bytes + k) < o.capacity) o.packets[o.n_bytes + k] = L.ring[ring_at(rd, k)];
    for (int base = 0; base < np; base += 8) {
        const int p = base + (lane >> 3), q = lane & 7;
        const bool mine = p < np;
        const int off = mine ? L.pk_off[p] : 0, len = mine ? (L.pk_off[p + 1] - off) : 0;
        const uint16_t crc = crc_lanes([&](int k) { return (uint32_t)L.ring[ring_at(rd, off + k)]; }, len - 2, L.crc_tab, 3, q);
        if (mine && q == 7 && o.n_packets + p < o.max_records) {
            const uint8_t b0 = L.ring[ring_at(rd, off)], b1 = L.ring[ring_at(rd, off + 1)], b2 = L.ring[ring_at(rd, off + 2)];
            const uint16_t rx = (uint16_t)((L.ring[ring_at(rd, off + len - 2)] << 8) | L.ring[ring_at(rd, off + len - 1)]);
            dabgpu_packet_record r;
            r.offset = (uint32_t)(o.n_bytes + off);
            r.length = (uint16_t)len;
            r.address = (uint16_t)(((b0 & 3) << 8) | b1);
            r.continuity_index = (b0 >> 4) & 3;
            r.first_last = (b0 >> 2) & 3;
            r.command = b2 >> 7;
            r.useful_length = b2 & 0x7F;
            r.is_corrected = (uint8_t)corrected;
            r.crc_ok = (rx == crc);
            r.reserved[0] = 0; r.reserved[1] = 0;
            o.records[o.n_packets + p] = r;
        }
    }
    st.read = ring_at(st.read, total == RING_BYTES ? 0 : total);
    st.size -= total;
    o.n_packets += np;
    o.n_bytes += total;
    __syncthreads();
}

// ~7 KB of LDS per single-wave workgroup
__global__ __launch_bounds__(64)
void packet_kernel(PkState* __restrict__ states, uint32_t* __restrict__ rings, const uint8_t* __restrict__ frames,
                   const unsigned long long* __restrict__ stream_offsets, size_t frame_stride, const uint32_t* __restrict__ frame_bytes, int n_frames,
                   uint8_t* __restrict__ packets, size_t packet_stride, dabgpu_packet_record* __restrict__ records, int max_records,
                   dabgpu_packet_fec_frame* __restrict__ fec_frames, int max_fec_frames, int32_t* __restrict__ counts, int n_streams,
                   const int32_t* __restrict__ active, int active_divisor)
{
    __shared__ PkLds L;
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= n_streams) return;
    if (active != nullptr && active[s / active_divisor] < 0) {           // nothing new for this stream in this call
        if (lane < 4) counts[4 * s + lane] = 0;
        return;
    }
    const uint32_t n = frame_bytes[s];
    // what this call cannot hold is reported, not skipped in silence
    if ((unsigned long long)RING_BYTES + (unsigned long long)n_frames * n > (unsigned long long)packet_stride) {
        if (lane < 4) counts[4 * s + lane] = (lane == 1) ? -2 : 0;
        return;
    }
    load_gf_crc_tables(L, lane);
    PkState st = states[s];
    uint32_t* ring_hbm = rings + (size_t)s * (RING_BYTES / 4);
    for (int k = lane; k < RING_BYTES / 4; k += 64) reinterpret_cast<uint32_t*>(L.ring)[k] = ring_hbm[k];
    PkOut o{packets + (size_t)s * packet_stride, packet_stride, records + (size_t)s * max_records, max_records, 0, 0};
    const uint8_t* base = frames + stream_offsets[s];
    int n_fec = 0, n_discarded = 0;
    __syncthreads();

    for (int f = 0; f < n_frames; f++) {
        const uint8_t* frame = base + (size_t)f * frame_stride;
        uint32_t pos = 0, win_start = 0, win_len = 0;
        while (pos < n) {
            const uint32_t remain = n - pos, need = (remain < 96u) ? remain : 96u;
            if (pos + need > win_start + win_len) {                        // stage the next part of the frame
                __syncthreads();
                win_start = pos;
                win_len = (remain < (uint32_t)PK_WINDOW) ? remain : (uint32_t)PK_WINDOW;
                for (uint32_t k = lane; k < win_len; k += 64) L.win[k] = frame[pos + k];
                __syncthreads();
            }
            const uint8_t* w = L.win + (pos - win_start);
            Header h;
            bool stored;
            const int used = walk_step((int)need, w[0], (need >= 2u) ? w[1] : (uint8_t)0, &h, &stored);
            if (!stored) { pos = n; break; }                               // (:58-61, :78-81: the rest of the buffer is consumed)
            pos += (uint32_t)used;
            // PushIntoRingBuffer (:132-159)
            while (ring_free(st.size) < h.length) {
                const int other = packet_length(L.ring[st.read] >> 6);
                st.size -= other;
                st.read = ring_at(st.read, other);
                st.discarded_bytes += other;
                st.discarded_packets++;
                n_discarded++;
            }
            for (int k = lane; k < h.length; k += 64) L.ring[ring_at(st.write, k)] = (k == 0) ? stored_header(w[0], h.length_id) : w[k];
            st.size += h.length;
            st.write = ring_at(st.write, h.length);
            __syncthreads();
            if (!h.is_fec) continue;
            if (fec_counter_invalid(st.last_counter, h.counter)) {          // (:89-105)
                st.last_counter = -1;
                pk_hand_out(L, st, 0x7FFFFFFF, 0, o, lane);
                continue;
            }
            st.last_counter = h.counter;
            if (h.counter != FEC_PACKETS - 1) continue;
            if (st.size != RING_BYTES) {                                    // (:112-120)
                pk_hand_out(L, st, 0x7FFFFFFF, 0, o, lane);
            } else {
                pk_correct_rows(L, st.read, lane);
                if (n_fec < max_fec_frames) {
                    dabgpu_packet_fec_frame* rec = fec_frames + (size_t)s * max_fec_frames + n_fec;
                    if (lane == 0) { rec->frame_index = f; rec->first_record = o.n_packets; }
                    if (lane < RS_ROWS) rec->rs_count[lane] = L.rs_count[lane];
                }
                n_fec++;
                pk_hand_out(L, st, APP_TABLE_BYTES, 1, o, lane);
            }
            st.last_counter = -1;
            st.read = 0; st.write = 0; st.size = 0; st.discarded_bytes = 0; st.discarded_packets = 0;     // ResetRingBuffer (:178-184)
        }
    }
    __syncthreads();
    for (int k = lane; k < RING_BYTES / 4; k += 64) ring_hbm[k] = reinterpret_cast<const uint32_t*>(L.ring)[k];
    if (lane == 0) {
        states[s] = st;
        counts[4 * s] = o.n_packets;
        counts[4 * s + 1] = o.n_bytes;
        counts[4 * s + 2] = n_fec;
        counts[4 * s + 3] = n_discarded;
    }
}

// ---- transmit ----
// the parity map of RS(204,188) (rs_core.h); some of its coefficients are zero, so the rows' marks are read
static __constant__ rs::ParityTab<RS_DATA_BYTES, PK_ROOTS> PK_PARITY_TAB = rs::make_parity_tab<RS_DATA_BYTES, PK_ROOTS>();

struct PkTxLds {
    alignas(16) uint8_t par_log[RS_DATA_BYTES][PK_ROOTS];
    alignas(16) uint8_t frame[RING_BYTES];
    alignas(16) dabgpu_packet_tx_entry ent[MAX_FRAME_PACKETS];
    uint16_t par_zero[RS_DATA_BYTES];
    uint8_t cell[MAX_FRAME_PACKETS];                         // 24-byte cell -> the entry that covers it
    uint8_t exp[512];
    uint8_t log[256];
    uint16_t crc_tab[256];
    uint32_t par[RS_ROWS][4];                                // parity of row i: byte r in bits 8 (r % 4) .. of word r / 4
    int bad;
};

__global__ __launch_bounds__(64)
void packet_tx_kernel(const uint8_t* __restrict__ data, const unsigned long long* __restrict__ group_offsets, const uint32_t* __restrict__ group_base,
                      const dabgpu_packet_tx_entry* __restrict__ table, size_t table_stride, const uint32_t* __restrict__ frame_first,
                      const uint16_t* __restrict__ address, const uint32_t* __restrict__ frame_bytes, const unsigned long long* __restrict__ start_byte,
                      uint8_t* __restrict__ frames, const unsigned long long* __restrict__ stream_offsets, size_t frame_stride,
                      int32_t* __restrict__ status, int n_fec_frames)
{
    __shared__ PkTxLds L;
    const int lane = threadIdx.x;
    const size_t item = blockIdx.x;
    const size_t s = item / (size_t)n_fec_frames, t = item % (size_t)n_fec_frames;
    const uint32_t fb = frame_bytes[s], addr = address[s];
    const unsigned long long start = start_byte[s];
    const uint32_t pos0 = (uint32_t)t * (uint32_t)RING_BYTES;
    const uint32_t first = frame_first[s * ((size_t)n_fec_frames + 1) + t], end = frame_first[s * ((size_t)n_fec_frames + 1) + t + 1];
    const uint32_t g0 = group_base[s], n_groups = group_base[s + 1] - g0;
    int st = 0;
    if (addr < 1u || addr > (uint32_t)MAX_ADDRESS) st = DABGPU_PACKET_TX_BAD_ADDRESS;
    else if (fb == 0u || fb % 24u) st = DABGPU_PACKET_TX_BAD_FRAME_BYTES;
    else if (start % 24u) st = DABGPU_PACKET_TX_BAD_START;
    else if (end <= first || end - first > (uint32_t)MAX_FRAME_PACKETS || (size_t)end > table_stride) st = DABGPU_PACKET_TX_BAD_TABLE;
    if (fb == 0u) { if (lane == 0) status[item] = st; return; }
    load_gf_crc_tables(L, lane);
    for (int i = lane; i < RS_DATA_BYTES; i += 64) {
        *reinterpret_cast<uint4*>(L.par_log[i]) = *reinterpret_cast<const uint4*>(PK_PARITY_TAB.log_coef[i]);
        L.par_zero[i] = PK_PARITY_TAB.zero[i];
    }
    for (int i = lane; i < RS_ROWS * 4; i += 64) (&L.par[0][0])[i] = 0;
    if (lane == 0) L.bad = 0;
    int cnt = (st == 0) ? (int)(end - first) : 0;
    const dabgpu_packet_tx_entry* tab = table + s * table_stride + first;
    for (int i = lane; i < cnt; i += 64) L.ent[i] = tab[i];
    __syncthreads();
    if (st == 0) {
        // the entries tile the 2256 bytes with valid packets that stay inside their logical frames and inside their groups
        int bad = 0;
        for (int i = lane; i < cnt; i += 64) {
            const dabgpu_packet_tx_entry e = L.ent[i];
            const uint32_t next = (i + 1 < cnt) ? L.ent[i + 1].position : pos0 + (uint32_t)APP_TABLE_BYTES;
            if (!length_valid(e.length) || e.useful + 5 > e.length || e.continuity_index > 3 || e.flags > 3) bad = 1;
            else if ((i == 0 && e.position != pos0) || e.position + e.length != next || e.position < pos0 || (e.position - pos0) % 24u) bad = 1;
            else if ((start + e.position) % fb + e.length > fb) bad = 1;
            else if (e.group < -1 || (e.group >= 0 && (uint32_t)e.group >= n_groups)) bad = 1;
            else if (e.group < 0 && e.useful != 0) bad = 1;
            else if (e.group >= 0) {
                const unsigned long long glen = group_offsets[g0 + e.group + 1] - group_offsets[g0 + e.group];
                if ((unsigned long long)e.offset + e.useful > glen) bad = 1;
            }
        }
        if (bad) L.bad = 1;
        __syncthreads();
        if (L.bad) st = DABGPU_PACKET_TX_BAD_TABLE;
    }
    if (lane == 0) status[item] = st;
    if (st != 0) {                                          // a refused frame: 94 padding packets
        __syncthreads();
        cnt = MAX_FRAME_PACKETS;
        for (int i = lane; i < cnt; i += 64) L.ent[i] = dabgpu_packet_tx_entry{-1, 0u, pos0 + 24u * (uint32_t)i, 24, 0, 0, 0};
        __syncthreads();
    }
    for (int i = lane; i < cnt; i += 64) {
        const uint32_t c0 = (L.ent[i].position - pos0) / 24u;
        for (uint32_t c = 0; c < L.ent[i].length / 24u; c++) L.cell[c0 + c] = (uint8_t)i;
    }
    __syncthreads();
    // packets: header, useful bytes, zero padding (the CRC's two bytes follow below)
    for (int b = lane; b < APP_TABLE_BYTES; b += 64) {
        const dabgpu_packet_tx_entry e = L.ent[L.cell[b / 24]];
        const uint32_t k = (uint32_t)b - (e.position - pos0), a = (e.group < 0) ? 0u : addr;
        uint8_t v = 0;
        if (k == 0) v = data_header0(length_id_of(e.length), e.continuity_index, (e.flags >> 1) & 1, e.flags & 1, (int)a);
        else if (k == 1) v = (uint8_t)(a & 0xFFu);
        else if (k == 2) v = e.useful;
        else if (k < 3u + e.useful) v = data[group_offsets[g0 + e.group] + e.offset + (k - 3u)];
        L.frame[b] = v;
    }
    __syncthreads();
    for (int base = 0; base < cnt; base += 8) {
        const int p = base + (lane >> 3), q = lane & 7;
        const bool mine = p < cnt;
        const int off = mine ? (int)(L.ent[p].position - pos0) : 0, len = mine ? (int)L.ent[p].length : 0;
        const uint16_t crc = crc_lanes([&](int k) { return (uint32_t)L.frame[off + k]; }, len - 2, L.crc_tab, 3, q);
        if (mine && q == 7) { L.frame[off + len - 2] = (uint8_t)(crc >> 8); L.frame[off + len - 1] = (uint8_t)(crc & 0xFFu); }
    }
    __syncthreads();
    // parity: five lanes per row
    if (lane < 5 * RS_ROWS) {
        const int i = lane % RS_ROWS, q = lane / RS_ROWS;
        uint32_t w[4] = {0, 0, 0, 0};
        for (int j = q; j < RS_DATA_BYTES; j += 5) {
            const uint32_t d = L.frame[j * RS_ROWS + i];
            if (d) {
                const uint32_t ld = L.log[d], zero = L.par_zero[j];
                const uint4 row = *reinterpret_cast<const uint4*>(L.par_log[j]);
                const uint32_t rw[4] = {row.x, row.y, row.z, row.w};
                rs::parity_add<PK_ROOTS>(L, ld, rw, zero, w);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) atomicXor(&L.par[i][k], w[k]);
    }
    __syncthreads();
    // the nine FEC packets (:190-206 read them back): counter m, address 0x3FE, 22 bytes of the RS data table, 6 zero bytes at the end
    for (int b = lane; b < FEC_PACKETS * FEC_PACKET_BYTES; b += 64) {
        const int m = b / FEC_PACKET_BYTES, k = b % FEC_PACKET_BYTES;
        uint8_t v = 0;
        if (k == 0) v = fec_packet_header0(m);
        else if (k == 1) v = fec_packet_header1();
        else {
            const int ti = fec_packet_table_index(m, k);
            if (ti >= 0) { const int r = ti / RS_ROWS, i = ti % RS_ROWS; v = (uint8_t)(L.par[i][r >> 2] >> (8 * (r & 3))); }
        }
        L.frame[APP_TABLE_BYTES + b] = v;
    }
    __syncthreads();
    uint8_t* out = frames + stream_offsets[s];
    const unsigned long long f0 = start / fb;
    if (((uintptr_t)out & 3) == 0 && (frame_stride & 3) == 0 && (fb & 3u) == 0 && (start & 3ull) == 0) {
        for (int w = lane; w < RING_BYTES / 4; w += 64) {                   // a dword never straddles two logical frames here
            const unsigned long long k = start + pos0 + 4ull * (unsigned long long)w;
            *reinterpret_cast<uint32_t*>(out + (size_t)(k / fb - f0) * frame_stride + (size_t)(k % fb)) = reinterpret_cast<const uint32_t*>(L.frame)[w];
        }
    } else {
        for (int b = lane; b < RING_BYTES; b += 64) {
            const unsigned long long k = start + pos0 + (unsigned long long)b;
            out[(size_t)(k / fb - f0) * frame_stride + (size_t)(k % fb)] = L.frame[b];
        }
    }
}

}  // namespace dabgpu

using namespace dabgpu;

struct dabgpu_packet_bank {
    dabgpu_ctx* ctx = nullptr;
    size_t n = 0;
    DeviceBuffer<PkState> d_states;
    DeviceBuffer<uint32_t> d_rings;
    DeviceBuffer<unsigned long long> d_off; DeviceBuffer<uint32_t> d_n; DeviceBuffer<int32_t> d_counts;    // single-stream host-buffer path
};

extern "C" {

void dabgpu_packet_bank_destroy(dabgpu_packet_bank* b) {
    if (!dabgpu_destroy_begin(b, b ? b->ctx : nullptr)) return;
    delete b;
}

int dabgpu_packet_bank_reset(dabgpu_packet_bank* b, void* stream) {
    if (!b) { dabgpu_set_error("packet_bank_reset: null bank"); return DABGPU_ERR_INVALID_ARG; }
    DABGPU_BIND(b->ctx);
    // the constructor's state: empty ring, no FEC counter remembered
    std::vector<PkState> init(b->n, PkState{0, 0, 0, -1, 0, 0, {0, 0}});
    int st = dabgpu_check_hip(hipMemcpyAsync(b->d_states.get(), init.data(), b->n * sizeof(PkState), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync");
    if (st) return st;
    st = dabgpu_check_hip(hipMemsetAsync(b->d_rings.get(), 0, b->n * (size_t)RING_BYTES, (hipStream_t)stream), "hipMemsetAsync");
    if (st) return st;
    return dabgpu_check_hip(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
}

int dabgpu_packet_bank_create(dabgpu_ctx* c, size_t n_streams, dabgpu_packet_bank** out) {
    if (!c || !out || n_streams > (size_t)(1 << 22)) { dabgpu_set_error("packet_bank_create: invalid argument"); return DABGPU_ERR_INVALID_ARG; }
    *out = nullptr;
    DABGPU_BIND(c);
    dabgpu_packet_bank* b = new (std::nothrow) dabgpu_packet_bank();
    if (!b) return DABGPU_ERR_HIP;
    b->ctx = c; b->n = n_streams;
    const char* what = "hipMalloc(packet bank)";
    const size_t n1 = std::max<size_t>(n_streams, 1);       // (a bank of no streams is legal and does nothing)
    int st = b->d_states.alloc(n1, what);
    if (!st) st = b->d_rings.alloc(n1 * (size_t)RING_BYTES / sizeof(uint32_t), what);
    if (!st) st = b->d_off.alloc(1, what);
    if (!st) st = b->d_n.alloc(1, what);
    if (!st) st = b->d_counts.alloc(4, what);
    if (!st) st = dabgpu_check_hip(hipMemsetAsync(b->d_off.get(), 0, sizeof(unsigned long long), c->stream), "hipMemsetAsync");
    if (!st) st = dabgpu_packet_bank_reset(b, c->stream);
    if (st) { dabgpu_packet_bank_destroy(b); return st; }
    *out = b;
    return DABGPU_OK;
}

int dabgpu_packet_bank_process(dabgpu_packet_bank* b, const uint8_t* d_frames, const uint64_t* d_stream_offsets, size_t frame_stride_bytes,
                               const uint32_t* d_frame_bytes, int n_frames, uint8_t* d_packets, size_t packet_stride_bytes,
                               dabgpu_packet_record* d_records, int max_records, dabgpu_packet_fec_frame* d_fec_frames, int max_fec_frames,
                               int32_t* d_counts, void* stream) {
    return dabgpu_packet_bank_process_masked(b, d_frames, d_stream_offsets, frame_stride_bytes, d_frame_bytes, n_frames, d_packets,
                                             packet_stride_bytes, d_records, max_records, d_fec_frames, max_fec_frames, d_counts, nullptr, 1, stream);
}

int dabgpu_packet_bank_process_masked(dabgpu_packet_bank* b, const uint8_t* d_frames, const uint64_t* d_stream_offsets, size_t frame_stride_bytes,
                                      const uint32_t* d_frame_bytes, int n_frames, uint8_t* d_packets, size_t packet_stride_bytes,
                                      dabgpu_packet_record* d_records, int max_records, dabgpu_packet_fec_frame* d_fec_frames,
                                      int max_fec_frames, int32_t* d_counts, const int32_t* d_active, int streams_per_flag, void* stream) {
    if (!b) { dabgpu_set_error("packet_bank_process: null bank"); return DABGPU_ERR_INVALID_ARG; }
    if (n_frames < 0 || max_records < 0 || max_fec_frames < 0) {
        dabgpu_set_error("packet_bank_process: n_frames, max_records and max_fec_frames must not be negative"); return DABGPU_ERR_INVALID_ARG;
    }
    if (streams_per_flag < 1) { dabgpu_set_error("packet_bank_process_masked: streams_per_flag must be positive"); return DABGPU_ERR_INVALID_ARG; }
    if (b->n == 0 || n_frames == 0) return DABGPU_OK;
    if (!d_frames || !d_stream_offsets || !d_frame_bytes || !d_packets || !d_counts || (!d_records && max_records > 0) ||
        (!d_fec_frames && max_fec_frames > 0)) {
        dabgpu_set_error("packet_bank_process: null argument"); return DABGPU_ERR_INVALID_ARG;
    }
    DABGPU_BIND(b->ctx);
    hipLaunchKernelGGL(packet_kernel, dim3((unsigned)b->n), dim3(64), 0, (hipStream_t)stream, b->d_states.get(), b->d_rings.get(), d_frames,
                       reinterpret_cast<const unsigned long long*>(d_stream_offsets), frame_stride_bytes, d_frame_bytes, n_frames, d_packets,
                       packet_stride_bytes, d_records, max_records, d_fec_frames, max_fec_frames, d_counts, (int)b->n, d_active, streams_per_flag);
    return dabgpu_check_hip(hipGetLastError(), "packet_kernel launch");
}

int dabgpu_packet_fec_read_host_sync(dabgpu_packet_bank* b, const uint8_t* h_buf, uint32_t n_bytes, uint8_t* h_packets,
                                     dabgpu_packet_record* h_records, int max_records, dabgpu_packet_fec_frame* h_fec_frames,
                                     int max_fec_frames, int32_t* h_counts) {
    if (!b || !h_counts || (!h_buf && n_bytes) || !h_packets || (!h_records && max_records > 0) || (!h_fec_frames && max_fec_frames > 0) ||
        max_records < 0 || max_fec_frames < 0) {
        dabgpu_set_error("packet_fec_read_host_sync: invalid argument"); return DABGPU_ERR_INVALID_ARG;
    }
    if (b->n != 1) { dabgpu_set_error("packet_fec_read_host_sync: needs a bank of one stream"); return DABGPU_ERR_INVALID_ARG; }
    if (n_bytes > (1u << 24)) { dabgpu_set_error("packet_fec_read_host_sync: buffers above 16 MiB are not supported"); return DABGPU_ERR_UNSUPPORTED; }
    for (int k = 0; k < 4; k++) h_counts[k] = 0;
    if (n_bytes == 0) return DABGPU_OK;
    dabgpu_ctx* c = b->ctx;
    DABGPU_BIND(c);
    DABGPU_HOST_LOCK(c);
    hipStream_t s = c->stream;
    int st;
    // in: the buffer; out: packets | records | FEC frame records
    const size_t cap = (size_t)RING_BYTES + n_bytes, off_rec = (cap + 15) & ~(size_t)15;
    const size_t off_fec = off_rec + (size_t)max_records * sizeof(dabgpu_packet_record);
    const size_t out_bytes = off_fec + (size_t)max_fec_frames * sizeof(dabgpu_packet_fec_frame) + 16;
    void *d_in, *d_out;
    if ((st = dabgpu_scratch(c, SCR_CONVERT_IN, (size_t)n_bytes + 16, &d_in))) return st;
    if ((st = dabgpu_scratch(c, SCR_CONVERT_OUT, out_bytes, &d_out))) return st;
    uint8_t* dout = static_cast<uint8_t*>(d_out);
    DABGPU_CK(hipMemcpyAsync(d_in, h_buf, n_bytes, hipMemcpyHostToDevice, s));
    DABGPU_CK(hipMemcpyAsync(b->d_n.get(), &n_bytes, sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if ((st = dabgpu_packet_bank_process(b, static_cast<const uint8_t*>(d_in), reinterpret_cast<const uint64_t*>(b->d_off.get()), 0, b->d_n.get(), 1, dout, cap,
                                         reinterpret_cast<dabgpu_packet_record*>(dout + off_rec), max_records,
                                         reinterpret_cast<dabgpu_packet_fec_frame*>(dout + off_fec), max_fec_frames, b->d_counts.get(), s))) return st;
    DABGPU_CK(hipMemcpyAsync(h_counts, b->d_counts.get(), 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DABGPU_CK(hipStreamSynchronize(s));
    const size_t np = (size_t)std::min(std::max(h_counts[0], 0), max_records), nf = (size_t)std::min(std::max(h_counts[2], 0), max_fec_frames);
    if (h_counts[1] > 0) DABGPU_CK(hipMemcpyAsync(h_packets, dout, (size_t)h_counts[1], hipMemcpyDeviceToHost, s));
    if (np) DABGPU_CK(hipMemcpyAsync(h_records, dout + off_rec, np * sizeof(dabgpu_packet_record), hipMemcpyDeviceToHost, s));
    if (nf) DABGPU_CK(hipMemcpyAsync(h_fec_frames, dout + off_fec, nf * sizeof(dabgpu_packet_fec_frame), hipMemcpyDeviceToHost, s));
    DABGPU_CK(hipStreamSynchronize(s));
    return DABGPU_OK;
}

int dabgpu_packet_tx_encode(dabgpu_ctx* c, size_t n_streams, int n_fec_frames, const uint8_t* d_data, const uint64_t* d_group_offsets,
                            const uint32_t* d_group_base, const dabgpu_packet_tx_entry* d_table, size_t table_stride,
                            const uint32_t* d_frame_first, const uint16_t* d_address, const uint32_t* d_frame_bytes,
                            const uint64_t* d_start_byte, uint8_t* d_frames, const uint64_t* d_stream_offsets, size_t frame_stride_bytes,
                            int32_t* d_status, void* stream) {
    if (!c) { dabgpu_set_error("packet_tx_encode: null context"); return DABGPU_ERR_INVALID_ARG; }
    if (n_fec_frames < 0) { dabgpu_set_error("packet_tx_encode: n_fec_frames = %d", n_fec_frames); return DABGPU_ERR_INVALID_ARG; }
    if (n_streams == 0 || n_fec_frames == 0) return DABGPU_OK;
    if (n_fec_frames > (1 << 20) || n_streams > ((size_t)1 << 30) / (size_t)n_fec_frames) {
        dabgpu_set_error("packet_tx_encode: too many FEC frames (at most 2^20 per stream, streams x frames <= 2^30)"); return DABGPU_ERR_INVALID_ARG;
    }
    if (table_stride < (size_t)MAX_FRAME_PACKETS * (size_t)n_fec_frames) {
        dabgpu_set_error("packet_tx_encode: table_stride must be at least 94 n_fec_frames"); return DABGPU_ERR_INVALID_ARG;
    }
    if (!d_data || !d_group_offsets || !d_group_base || !d_table || !d_frame_first || !d_address || !d_frame_bytes || !d_start_byte || !d_frames ||
        !d_stream_offsets || !d_status) {
        dabgpu_set_error("packet_tx_encode: null argument"); return DABGPU_ERR_INVALID_ARG;
    }
    DABGPU_BIND(c);
    hipLaunchKernelGGL(packet_tx_kernel, dim3((unsigned)(n_streams * (size_t)n_fec_frames)), dim3(64), 0, (hipStream_t)stream, d_data,
                       reinterpret_cast<const unsigned long long*>(d_group_offsets), d_group_base, d_table, table_stride, d_frame_first, d_address,
                       d_frame_bytes, reinterpret_cast<const unsigned long long*>(d_start_byte), d_frames,
                       reinterpret_cast<const unsigned long long*>(d_stream_offsets), frame_stride_bytes, d_status, n_fec_frames);
    return dabgpu_check_hip(hipGetLastError(), "packet_tx_kernel launch");
}

int dabgpu_packet_tx_encode_host_sync(dabgpu_ctx* c, int n_fec_frames, const uint8_t* h_data, size_t n_data_bytes, const uint64_t* h_group_offsets,
                                      size_t n_groups, const dabgpu_packet_tx_entry* h_table, const uint32_t* h_frame_first, uint32_t address,
                                      uint32_t frame_bytes, uint64_t start_byte, uint8_t* h_frames, int32_t* h_status) {
    if (!c) { dabgpu_set_error("packet_tx_encode_host_sync: null context"); return DABGPU_ERR_INVALID_ARG; }
    if (n_fec_frames < 0 || n_fec_frames > (1 << 20)) { dabgpu_set_error("packet_tx_encode_host_sync: n_fec_frames = %d", n_fec_frames); return DABGPU_ERR_INVALID_ARG; }
    if (n_fec_frames == 0) return DABGPU_OK;
    if (!h_table || !h_frame_first || !h_frames || !h_status || (n_groups && !h_group_offsets) || (n_data_bytes && !h_data) || n_groups > (1u << 30)) {
        dabgpu_set_error("packet_tx_encode_host_sync: null argument"); return DABGPU_ERR_INVALID_ARG;
    }
    const size_t K = (size_t)n_fec_frames;
    if (frame_bytes == 0) {                                  // the device form's answer, without a division by it
        for (size_t k = 0; k < K; k++) h_status[k] = (address < 1u || address > (uint32_t)MAX_ADDRESS) ? DABGPU_PACKET_TX_BAD_ADDRESS : DABGPU_PACKET_TX_BAD_FRAME_BYTES;
        return DABGPU_OK;
    }
    const size_t n_entries = std::min<size_t>(h_frame_first[K], K * MAX_FRAME_PACKETS);
    const size_t n_logical = (size_t)((start_byte % frame_bytes + K * RING_BYTES + frame_bytes - 1) / frame_bytes);
    const size_t frames_bytes = n_logical * frame_bytes;
    // one block up: group offsets [n_groups + 1] | group base [2], frame bytes, address | start byte, stream offset | frame_first [K + 1], pad |
    // table [94 K] | data
    const size_t off_base = 8 * (n_groups + 1), off_start = off_base + 16, off_first = off_start + 16;
    const size_t off_table = (off_first + 4 * (K + 1) + 15) & ~(size_t)15, off_data = off_table + 16 * K * MAX_FRAME_PACKETS;
    const size_t up_bytes = off_data + n_data_bytes + 16, down_bytes = ((frames_bytes + 3) & ~(size_t)3) + 4 * K;
    std::vector<uint8_t> up(up_bytes, 0), down(down_bytes);
    for (size_t g = 0; g < n_groups; g++) memcpy(up.data() + 8 * g, &h_group_offsets[g], 8);
    const uint64_t total = n_data_bytes;
    memcpy(up.data() + 8 * n_groups, &total, 8);
    const uint32_t base2[2] = {0u, (uint32_t)n_groups};
    const uint16_t addr16 = (uint16_t)std::min<uint32_t>(address, 0xFFFFu);
    memcpy(up.data() + off_base, base2, 8);
    memcpy(up.data() + off_base + 8, &frame_bytes, 4);
    memcpy(up.data() + off_base + 12, &addr16, 2);
    memcpy(up.data() + off_start, &start_byte, 8);
    memcpy(up.data() + off_first, h_frame_first, 4 * (K + 1));
    memcpy(up.data() + off_table, h_table, n_entries * sizeof(dabgpu_packet_tx_entry));
    if (n_data_bytes) memcpy(up.data() + off_data, h_data, n_data_bytes);
    memcpy(down.data(), h_frames, frames_bytes);             // bytes the call does not write stay as they are
    DABGPU_BIND(c);
    DABGPU_HOST_LOCK(c);
    hipStream_t s = c->stream;
    int st;
    void *d_in, *d_out;
    if ((st = dabgpu_scratch(c, SCR_CONVERT_IN, up_bytes, &d_in))) return st;
    if ((st = dabgpu_scratch(c, SCR_CONVERT_OUT, down_bytes + 16, &d_out))) return st;
    uint8_t* di = static_cast<uint8_t*>(d_in);
    uint8_t* dout = static_cast<uint8_t*>(d_out);
    DABGPU_CK(hipMemcpyAsync(d_in, up.data(), up_bytes, hipMemcpyHostToDevice, s));
    DABGPU_CK(hipMemcpyAsync(d_out, down.data(), frames_bytes, hipMemcpyHostToDevice, s));
    st = dabgpu_packet_tx_encode(c, 1, n_fec_frames, di + off_data, reinterpret_cast<const uint64_t*>(di), reinterpret_cast<const uint32_t*>(di + off_base),
                                 reinterpret_cast<const dabgpu_packet_tx_entry*>(di + off_table), K * MAX_FRAME_PACKETS,
                                 reinterpret_cast<const uint32_t*>(di + off_first), reinterpret_cast<const uint16_t*>(di + off_base + 12),
                                 reinterpret_cast<const uint32_t*>(di + off_base + 8), reinterpret_cast<const uint64_t*>(di + off_start), dout,
                                 reinterpret_cast<const uint64_t*>(di + off_start + 8), frame_bytes,
                                 reinterpret_cast<int32_t*>(dout + ((frames_bytes + 3) & ~(size_t)3)), s);
    if (st) return st;
    DABGPU_CK(hipMemcpyAsync(down.data(), dout, ((frames_bytes + 3) & ~(size_t)3) + 4 * K, hipMemcpyDeviceToHost, s));
    DABGPU_CK(hipStreamSynchronize(s));
    memcpy(h_frames, down.data(), frames_bytes);
    memcpy(h_status, down.data() + ((frames_bytes + 3) & ~(size_t)3), 4 * K);
    return DABGPU_OK;
}

}  // extern "C"
