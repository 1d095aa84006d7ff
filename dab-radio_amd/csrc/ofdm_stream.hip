// ofdm_stream.hip -- device-side unsynchronised front end: a BANK of independent OFDM receivers,
// each with the state OFDM_Demod keeps between Process() calls (src/ofdm/ofdm_demodulator.h:131-176) resident in
// HBM, advanced by device kernels.  One dabgpu_stream_bank_process() = one OFDM_Demod::Process(block) for every
// stream of the bank (src/ofdm/ofdm_demodulator.cpp:235-275):
//
//   stream_l1_kernel        the L1 windows of UpdateSignalAverage (:934-950) for the whole block, one thread per window
//   stream_advance_kernel   one workgroup per stream: the level IIR, FindNullPowerDip (:291-347), ReadNullPRS (:349-358),
//                           ReadSymbols' bookkeeping (:550-562), Reset (:277-289) and the bookkeeping after a sync / a
//                           demodulated frame.  Runs until the stream needs the PRS synchroniser or the frame
//                           demodulator, or has consumed its block.  A frame that completes inside the block is NOT
//                           assembled: the demodulator reads its head from the stream's frame buffer and the rest
//                           straight from the caller's block (dabgpu_frame_desc); only the unfinished frame at the end
//                           of a block is carried over, by
//   stream_copy_kernel      many workgroups per stream, once per call after the last round
//   ofdm_sync_kernel        (ofdm_sync.hip) for the streams whose correlation window just filled
//   ofdm_demod_kernel + ofdm_phase_kernel  (ofdm_demod.hip) for the streams whose frame buffer just filled
//
// repeated ("rounds") until every stream has consumed its block; the host only reads one counter back per round
// after the rounds every stream needs in steady state.  Every float is produced by the same operations in the same
// order as the host mirror class (host/ofdm/ofdm_demodulator.cpp) and the oracle composition tests/stream_model.py.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <new>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "iq_decode.h"
#include "iq_sample.h"
#include "ofdm_device.h"

namespace dabgpu {

// geometry of the bank's transmission mode (src/ofdm/dab_ofdm_params_ref.cpp:11-60); mode I: 2656 / 2552 / 76 / 196608 / 5208
struct BankGeom { int mode, null_period, period, n_sym, n_fft, frame_samples, n_corr, frame_bits; };
enum { ST_FINDING_NULL = 0, ST_READING_NULL_PRS = 1, ST_RUNNING_COARSE = 2, ST_RUNNING_FINE = 3, ST_READING_SYMBOLS = 4 };
enum { PEND_NONE = 0, PEND_SYNC = 1, PEND_DEMOD = 2 };

struct StreamState {
    int state;
    float signal_avg;
    int null_start, null_end;
    int ring_index, ring_length;
    int corr_length, frame_length;
    int pending;
    int n_out;                       // frames completed in the current process() call
    int fine_time_offset;
    int total_frames_read, total_frames_desync;
    int avg_done;                    // UpdateSignalAverage already applied to the current block
    long long pos;                   // samples of the current block consumed
    // retained blocks (dabgpu_stream_bank_process_retained): frame samples [carry_dst, carry_end) of the frame under collection were
    // NOT copied into the frame buffer at the end of the previous call -- they still sit in the previous block, frame sample n at block
    // sample carry_src + (n - carry_dst).  Both bounds are even (the loaders fetch sample pairs); 0, 0 = nothing carried
    int carry_dst, carry_end;
    long long carry_src;
};

struct BankView {
    BankGeom g;
    StreamState* st;
    dabgpu_sync_state* sync;
    f2* ring;                        // [n][null_period]
    f2* corr;                        // [n][null_period + period]
    f2* frame;                       // [n][frame_samples]
    float* freq;                     // [n] coarse + fine handed to the PLL
    int* sync_active;                // [n]
    dabgpu_frame_desc* desc;         // [n] demodulation request of the round
    long long* copy_src;             // [n] carry-over copy of the call: block sample offset ...
    int* copy_dst;                   // [n] ... frame buffer offset ...
    int* copy_cnt;                   // [n] ... samples (0 = none)
    float* win;                      // [n][win_cap] L1 windows of the current block
    long long win_cap;
    int* not_done;                   // [2 lanes][8 rounds]: streams of the lane that need another round; round r counts in [r % 8] and
                                     // clears [(r + 1) % 8] (no memset between the rounds)
    dabgpu_sync_state* records;      // the caller's, by bits slot (dabgpu_stream_bank_set_products); null = the bank stores no products
};


template <int SRC>
__device__ __forceinline__ float l1_window(const uint8_t* base, long long first, int k) {           // CalculateL1Average :922-932
    float acc = 0.0f;
    for (int i = 0; i < k; i++) { const f2 v = sample_at<SRC>(base, first + i); acc += __builtin_fabsf(v.x) + __builtin_fabsf(v.y); }
    return acc / (float)k;
}

template <int SRC>
__device__ __forceinline__ void copy_block_samples(f2* __restrict__ dst, const uint8_t* __restrict__ base, long long first, long long n, int t) {
    for (long long i = t; i < n; i += 256) dst[i] = sample_at<SRC>(base, first + i);
}

__device__ __forceinline__ void copy_samples(f2* __restrict__ dst, const f2* __restrict__ src, long long n, int t) {
    long long i = t;
    for (; i + 768 < n; i += 1024) {                     // four independent loads in flight
        const f2 a = src[i], b = src[i + 256], c = src[i + 512], d = src[i + 768];
        dst[i] = a; dst[i + 256] = b; dst[i + 512] = c; dst[i + 768] = d;
    }
    for (; i < n; i += 256) dst[i] = src[i];
}

template <int SRC>
__global__ __launch_bounds__(256)
void stream_advance_kernel(BankView B, int s0, int n_streams, const uint8_t* __restrict__ iq, size_t stream_stride, long long n_samples,
                           dabgpu_stream_cfg cfg, int max_frames, int first_round, int ring_mode, int* __restrict__ not_done, int* __restrict__ next_not_done,
                           const uint8_t* __restrict__ prev_iq, int retain)
{
    __shared__ StreamState S;
    __shared__ float win[256];
    __shared__ int sh_i[2];
    __shared__ long long sh_w;
    const int s = s0 + blockIdx.x, t = threadIdx.x;       // streams s0 .. s0 + n_streams - 1 (a lane of the bank, see bank_process_impl)
    if (s >= s0 + n_streams) return;
    if (blockIdx.x == 0 && t == 0) *next_not_done = 0;    // the next round's counter (nobody counts in it during this round)
    if (t == 0) S = B.st[s];
    __syncthreads();
    const uint8_t* block = iq + (size_t)s * stream_stride * src_sample_bytes<SRC>::value;
    // the previous call's block, still valid (retained mode), or null: then nothing is carried
    const uint8_t* prev_block = prev_iq ? prev_iq + (size_t)s * stream_stride * src_sample_bytes<SRC>::value : nullptr;
    const int NB_NULL_PERIOD = B.g.null_period, NB_CORR = B.g.n_corr, NB_FRAME_SAMPLES = B.g.frame_samples;
    f2* ring = B.ring + (size_t)s * NB_NULL_PERIOD;
    f2* corr = B.corr + (size_t)s * NB_CORR;
    f2* frame = B.frame + (size_t)s * NB_FRAME_SAMPLES;
    const int k = cfg.signal_l1_nb_samples;

    if (first_round) {
        if (t == 0) {
            S.pos = 0; S.n_out = 0; S.avg_done = 0;
            // what the previous call left in its block instead of copying it (retained mode) is this call's carry -- unless the frame
            // cannot complete inside this block (it began in the last samples of the previous block and this block is shorter than a
            // frame: the ring form's blocks are): a frame may lie in the frame buffer, the previous block and this block, not in a
            // third block, so those few samples are copied into the frame buffer now
            const int left = B.copy_cnt[s];
            sh_i[0] = 0;
            if (prev_block != nullptr && left > 0) {
                S.carry_dst = B.copy_dst[s]; S.carry_end = B.copy_dst[s] + left; S.carry_src = B.copy_src[s];
                if ((long long)NB_FRAME_SAMPLES - (long long)S.frame_length > n_samples) sh_i[0] = 1;
            } else { S.carry_dst = 0; S.carry_end = 0; S.carry_src = 0; }
            B.copy_cnt[s] = 0;
        }
        __syncthreads();
        if (sh_i[0]) {
            copy_block_samples<SRC>(frame + S.carry_dst, prev_block, S.carry_src, (long long)(S.carry_end - S.carry_dst), t);
            __syncthreads();
            if (t == 0) { S.carry_dst = 0; S.carry_end = 0; S.carry_src = 0; }
            __syncthreads();
        }
    }

    // ---- what the previous round's sync / demod kernels produced ----
    if (S.pending == PEND_SYNC) {
        const dabgpu_sync_state y = B.sync[s];
        if (!y.sync_valid) {                                               // Reset() :277-289, :529-532
            __syncthreads();
            if (t == 0) {
                S.state = ST_FINDING_NULL; S.corr_length = 0; S.total_frames_desync++; S.fine_time_offset = 0;
                dabgpu_sync_state z = y; z.is_found_coarse = 0; z.freq_coarse = 0.0f; z.freq_fine = 0.0f; z.fine_time_offset = 0;
                B.sync[s] = z;
            }
        } else {                                                           // :536-546
            const int start = NB_NULL_PERIOD + y.fine_time_offset;
            const int count = NB_CORR - start;
            copy_samples(frame, corr + start, count, t);
            __syncthreads();
            if (t == 0) { S.frame_length = count; S.corr_length = 0; S.fine_time_offset = y.fine_time_offset; S.state = ST_READING_SYMBOLS; }
        }
        if (t == 0) { S.pending = PEND_NONE; B.sync_active[s] = 0; }
        __syncthreads();
    }
    // (a demodulation request never stays pending: the frame's bookkeeping is done where the request is made, see ReadSymbols below)
    if (t == 0) B.desc[s].slot = -1;
    __syncthreads();

    // ---- UpdateSignalAverage over the whole block, once per process() (:934-950); windows from stream_l1_kernel ----
    if (!S.avg_done) {
        if (n_samples >= k) {
            const long long stride = (long long)k * cfg.signal_l1_nb_decimate;
            const long long n_win = (n_samples - k + stride - 1) / stride;         // i = 0, stride, ... < n - k
            const float* wsrc = B.win + (size_t)s * B.win_cap;
            for (long long w0 = 0; w0 < n_win; w0 += 256) {
                if (w0 + t < n_win) win[t] = wsrc[w0 + t];
                __syncthreads();
                if (t == 0) {
                    const int m = (int)((n_win - w0 < 256) ? (n_win - w0) : 256);
                    float a = S.signal_avg;
                    const float beta = cfg.signal_l1_update_beta;
                    for (int j = 0; j < m; j++) a = beta * a + (1.0f - beta) * win[j];
                    S.signal_avg = a;
                }
                __syncthreads();
            }
        }
        if (t == 0) S.avg_done = 1;
        __syncthreads();
    }
    // ---- the Process() loop (:241-274) up to the next device-kernel request ----
    while (S.pos < n_samples && S.pending == PEND_NONE) {
        const long long bpos = S.pos;                                               // buf[i] of the reference = block sample bpos + i
        const long long rest = n_samples - S.pos;
        if (S.state == ST_FINDING_NULL) {
            // FindNullPowerDip :291-347
            const float start_thresh = S.signal_avg * cfg.thresh_null_start;
            const float end_thresh = S.signal_avg * cfg.thresh_null_end;
            const long long n_win = (rest > k) ? (rest - 1) / k : 0;                // i = 0, k, ... while i < rest - k
            if (t == 0) { sh_i[0] = S.null_start; sh_i[1] = 0; }                    // [1] = null end found
            long long nb_read = rest;
            __syncthreads();
            for (long long w0 = 0; w0 < n_win; w0 += 256) {
                const long long w = w0 + t;
                if (w < n_win) win[t] = l1_window<SRC>(block, bpos + w * k, k);
                __syncthreads();
                if (t == 0) {
                    const int m = (int)((n_win - w0 < 256) ? (n_win - w0) : 256);
                    int started = sh_i[0];
                    for (int j = 0; j < m; j++) {
                        const float l1 = win[j];
                        if (started) {
                            if (l1 > end_thresh) { sh_i[1] = 1; sh_w = w0 + j; break; }
                        } else if (l1 < start_thresh) {
                            started = 1;
                        }
                    }
                    sh_i[0] = started;
                }
                __syncthreads();
                if (sh_i[1]) break;
            }
            const int null_end = sh_i[1];
            if (null_end) nb_read = sh_w * k + k;
            // circular buffer of the last nb_null_period samples (:325, circular_buffer.h:18-37)
            const int cap = NB_NULL_PERIOD;
            const long long keep = (nb_read < cap) ? nb_read : cap;
            const long long first = nb_read - keep;
            const int ring_index = S.ring_index;
            for (long long j = t; j < keep; j += 256) ring[(int)((ring_index + first + j) % cap)] = sample_at<SRC>(block, bpos + first + j);
            __syncthreads();
            const int new_index = (int)((ring_index + nb_read) % cap);
            const int new_length = (int)(((long long)S.ring_length + nb_read < cap) ? (S.ring_length + nb_read) : cap);
            if (null_end) {                                                         // :333-338
                for (int j = t; j < new_length; j += 256) corr[j] = ring[(j + new_index) % cap];
            }
            __syncthreads();
            if (t == 0) {
                S.ring_index = new_index; S.ring_length = new_length; S.null_start = sh_i[0];
                if (null_end) { S.corr_length = new_length; S.null_start = 0; S.null_end = 0; S.ring_length = 0; S.state = ST_READING_NULL_PRS; }
                S.pos += nb_read;
            }
            __syncthreads();
        } else if (S.state == ST_READING_NULL_PRS) {
            // ReadNullPRS :349-358
            const long long want = NB_CORR - S.corr_length;
            const long long take = (want < rest) ? want : rest;
            copy_block_samples<SRC>(corr + S.corr_length, block, bpos, take, t);
            __syncthreads();
            if (t == 0) {
                S.corr_length += (int)take; S.pos += take;
                // like the reference, a window that fills with the last sample of a block is synchronised by the NEXT Process()
                if (S.corr_length == NB_CORR) {
                    S.state = ST_RUNNING_COARSE;
                    if (S.pos < n_samples) { S.pending = PEND_SYNC; B.sync_active[s] = 1; }
                }
            }
            __syncthreads();
        } else if (S.state == ST_READING_SYMBOLS) {
            // ReadSymbols :550-577
            const int have = S.frame_length;
            const long long want = NB_FRAME_SAMPLES - have;
            const bool full = (want <= rest);
            const long long take = full ? want : rest;
            const int cd = S.carry_dst, ce = S.carry_end;                       // (retained mode) part of [0, have) still in the previous block
            const long long csrc = S.carry_src;
            if (full) {
                // the frame completes inside this block: no assembly, the demodulator reads [0, split) from the frame
                // buffer (or, retained mode, the previous block) and the rest from the block; one sample is moved over when the boundary
                // would split a pair
                if ((have & 1) && t == 0) frame[have] = sample_at<SRC>(block, bpos);
                // the NULL symbol at the end of this frame heads the next correlation window (:558-562)
                const int null_at = B.g.n_sym * B.g.period;
                for (int j = t; j < NB_NULL_PERIOD; j += 256) {
                    const int idx = null_at + j;
                    corr[j] = (idx < have) ? ((idx >= cd && idx < ce) ? sample_at<SRC>(prev_block, csrc + (idx - cd)) : frame[idx])
                                           : sample_at<SRC>(block, bpos + (idx - have));
                }
            } else if (t == 0) {
                // the block ends inside this frame: its samples so far are carried over into the stream's frame buffer by
                // stream_copy_kernel, ONCE per call after the last round -- a stream that asks for it has consumed its block and takes
                // no further part in the rounds (a copy launch per round, empty in all rounds but the last, cost 67 us each).
                // Retained mode: no copy at all -- the record becomes the next call's carry; its bounds are made even here (the
                // demodulator loads sample pairs), the odd samples at either end go to the frame buffer now.
                int a = have, e = have + (int)take;
                long long src = S.pos;
                if (retain) {
                    if ((a & 1) && a < e) { frame[a] = sample_at<SRC>(block, src); a++; src++; }
                    if ((e & 1) && a < e) { frame[e - 1] = sample_at<SRC>(block, S.pos + take - 1); e--; }
                }
                B.copy_src[s] = src; B.copy_dst[s] = a; B.copy_cnt[s] = e - a;
            }
            __syncthreads();
            if (t == 0) {
                const long long pos0 = S.pos;
                S.frame_length += (int)take; S.pos += take;
                if (full) {
                    S.corr_length = NB_NULL_PERIOD;
                    const dabgpu_sync_state y = B.sync[s];
                    B.freq[s] = y.freq_coarse + y.freq_fine;
                    // a frame beyond the caller's capacity is demodulated into the last slot (and reported through n_frames)
                    // (ring mode: slot of the stream's frame-history ring = frames demodulated so far mod ring length)
                    const int slot = ring_mode ? (S.total_frames_read % max_frames) : ((S.n_out < max_frames) ? S.n_out : (max_frames - 1));
                    dabgpu_frame_desc d;
                    d.slot = s * max_frames + slot;
                    d.split = have + (have & 1);
                    d.tail_off = pos0 + (have & 1);
                    d.carry_dst = cd; d.carry_end = ce; d.carry_off = csrc - cd;
                    B.desc[s] = d;
                    // the frame's record beside its products (dabgpu_stream_bank_set_products): the words the demodulator is handed, the
                    // fine word before this frame's phase update
                    if (B.records != nullptr) {
                        dabgpu_sync_state r;
                        r.freq_coarse = y.freq_coarse; r.freq_fine = y.freq_fine; r.is_found_coarse = y.is_found_coarse;
                        r.fine_time_offset = S.fine_time_offset; r.sync_valid = 1; r.reserved = 0;
                        B.records[d.slot] = r;
                    }
                    S.carry_dst = 0; S.carry_end = 0; S.carry_src = 0;
                    // The demodulation of this frame runs in THIS round (the round's kernel order is advance, copy, demod, phase, sync),
                    // so the state machine does the frame's bookkeeping now (:563-576) and reads on into the next NULL + PRS window: one
                    // round per frame instead of two.  The reference's order is kept -- the fine-frequency update of frame k - 1 (phase
                    // kernel) precedes the synchronisation of frame k (sync kernel) inside the round.
                    S.total_frames_read++; S.n_out++; S.frame_length = 0; S.state = ST_READING_NULL_PRS;
                }
            }
            __syncthreads();
        } else {
            // RUNNING_*: the correlation window filled at the very end of the previous block (:247-262)
            __syncthreads();
            if (t == 0) { S.pending = PEND_SYNC; B.sync_active[s] = 1; }
            __syncthreads();
        }
    }
    if (t == 0) {
        B.st[s] = S;
        if (S.pos < n_samples || S.pending != PEND_NONE) atomicAdd(not_done, 1);
    }
}

// L1 windows of UpdateSignalAverage for every stream's block: window w covers samples [w*stride, w*stride + k).
// 64 windows per workgroup: the samples are fetched coalesced (consecutive lanes = consecutive samples of a window) and
// reduced to |re| + |im| into LDS; one lane per window then adds its k terms in the reference's sequential order.
constexpr int L1_WINDOWS = 64;
constexpr int L1_MAX_K = 128;
template <int SRC>
__global__ __launch_bounds__(256)
void stream_l1_kernel(BankView B, const uint8_t* __restrict__ iq, size_t stream_stride, long long n_win, int k, long long stride) {
    __shared__ float term[L1_WINDOWS * (L1_MAX_K + 1)];
    const long long w0 = (long long)blockIdx.x * L1_WINDOWS;
    const int s = blockIdx.y, t = threadIdx.x;
    const uint8_t* base = iq + (size_t)s * stream_stride * src_sample_bytes<SRC>::value;
    const int m = (int)((n_win - w0 < L1_WINDOWS) ? (n_win - w0) : L1_WINDOWS);
    if (k <= L1_MAX_K) {
        for (int e = t; e < m * k; e += 256) {
            const int w = e / k, i = e - w * k;
            const f2 v = sample_at<SRC>(base, (w0 + w) * stride + i);
            term[w * (k + 1) + i] = __builtin_fabsf(v.x) + __builtin_fabsf(v.y);
        }
        __syncthreads();
        if (t < m) {
            float acc = 0.0f;
            for (int i = 0; i < k; i++) acc += term[t * (k + 1) + i];
            B.win[(size_t)s * B.win_cap + w0 + t] = acc / (float)k;
        }
    } else if (t < m) {
        B.win[(size_t)s * B.win_cap + w0 + t] = l1_window<SRC>(base, (w0 + t) * stride, k);
    }
}

// the carry-over copy block -> frame buffer (the unfinished frame at the end of a block), COPY_WGS workgroups per stream, once per call
constexpr int COPY_WGS = 16;
template <int SRC>
__global__ __launch_bounds__(256)
void stream_copy_kernel(BankView B, int s0, const uint8_t* __restrict__ iq, size_t stream_stride) {
    const int s = s0 + blockIdx.y;
    const int cnt = B.copy_cnt[s];
    if (cnt == 0) return;
    const uint8_t* src = iq + (size_t)s * stream_stride * src_sample_bytes<SRC>::value;
    const long long first = B.copy_src[s];
    f2* dst = B.frame + (size_t)s * B.g.frame_samples + B.copy_dst[s];
    const int per = (((cnt + COPY_WGS - 1) / COPY_WGS) + 255) & ~255;
    const int a = blockIdx.x * per;
    const int b = (a + per < cnt) ? (a + per) : cnt;
    int i = a + threadIdx.x;
    for (; i + 3 * 256 < b; i += 4 * 256) {                   // four independent loads in flight
        const f2 v0 = sample_at<SRC>(src, first + i), v1 = sample_at<SRC>(src, first + i + 256), v2 = sample_at<SRC>(src, first + i + 512),
                 v3 = sample_at<SRC>(src, first + i + 768);
        dst[i] = v0; dst[i + 256] = v1; dst[i + 512] = v2; dst[i + 768] = v3;
    }
    for (; i < b; i += 256) dst[i] = sample_at<SRC>(src, first + i);
}

__global__ void stream_report_kernel(BankView B, int n_streams, int* __restrict__ n_frames, dabgpu_stream_status* __restrict__ status,
                                     int ring_frames) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams) return;
    const StreamState S = B.st[s];
    if (n_frames) n_frames[s] = (ring_frames > 0) ? ((S.n_out > 0) ? ((S.total_frames_read - 1) % ring_frames) : -1) : S.n_out;
    if (status) {
        const dabgpu_sync_state y = B.sync[s];
        dabgpu_stream_status o;
        o.state = S.state; o.signal_l1_average = S.signal_avg; o.freq_coarse = y.freq_coarse; o.freq_fine = y.freq_fine;
        o.is_found_coarse = y.is_found_coarse; o.fine_time_offset = S.fine_time_offset;
        o.total_frames_read = S.total_frames_read; o.total_frames_desync = S.total_frames_desync;
        status[s] = o;
    }
}

}  // namespace dabgpu

using namespace dabgpu;

struct dabgpu_stream_bank {
    dabgpu_ctx* ctx = nullptr;
    size_t n = 0;
    dabgpu_stream_cfg cfg{};
    BankView view{};                   // its pointers, d_corr_out and d_status point at the allocations of `mem` and `win`
    float* d_corr_out = nullptr;       // [n][n_sym][2] cyclic-prefix correlations of the last demodulated frames
    dabgpu_stream_status* d_status = nullptr;
    DeviceBuffer<> mem[14];            // in the order dabgpu_stream_bank_create_mode makes them
    DeviceBuffer<float> win;           // view.win: L1 windows (grow-only)
    DeviceBuffer<float> raw_scratch;   // converted block of dabgpu_stream_bank_process_raw (grow-only)
    Stream side;                       // second lane of a call (mode I banks of >= 1024 streams): half of the streams run their rounds here
    Event ev_fork, ev_join;
    // retained blocks: the last call left the unfinished frames' samples in ITS block (no carry-over copy); the next call must be handed
    // that block again (dabgpu_stream_bank_process_retained), or dabgpu_stream_bank_release must copy them out of it first
    bool carry_pending = false;
    int carry_src = 0;                 // loader kind (SRC) and stream stride of that block
    size_t carry_stride = 0;
    // soft-decision policy of the frames demodulated from the next process call on (dabgpu_stream_bank_set_soft); survives a reset
    dabgpu_soft_cfg soft = {DABGPU_SOFT_NORMALISED, 64.0f};
    float* d_soft_scale = nullptr;     // the caller's: scale of the frame in bits slot k at [k], soft_scale_cap floats
    size_t soft_scale_cap = 0;
    // DQPSK products and sync records of the frames of the frames forms, by bits slot (dabgpu_stream_bank_set_products); survives a reset.
    // The records' address is view.records: the state machine writes them
    float* d_products = nullptr;       // the caller's: [products_cap][75][1536] complex float
    size_t products_cap = 0;           // frames
};

// DABGPU_SOFT_CSI with a scale buffer: every bits slot of the call has its word (checked before a call launches anything)
static int bank_soft_scale_fits(const dabgpu_stream_bank* b, size_t slots_per_stream) {
    if (b->soft.policy != DABGPU_SOFT_CSI || b->d_soft_scale == nullptr || slots_per_stream <= b->soft_scale_cap / b->n) return DABGPU_OK;
    dabgpu_set_error("stream_bank_process: %zu streams x %zu bits slots need more scale words than the %zu dabgpu_stream_bank_set_soft was given", b->n,
                     slots_per_stream, b->soft_scale_cap);
    return DABGPU_ERR_INVALID_ARG;
}

// products set (dabgpu_stream_bank_set_products): the call is a frames form under the weighted policy with a scale buffer, and every bits
// slot of the call has its products and its record (checked before a call launches or converts anything)
static int bank_products_fit(const dabgpu_stream_bank* b, size_t slots_per_stream, int ring_mode) {
    if (b->d_products == nullptr) return DABGPU_OK;
    if (ring_mode) {
        dabgpu_set_error("stream_bank_process_ring: the ring forms store no DQPSK products (dabgpu_stream_bank_set_products is set: use a frames form, "
                         "or switch the products off)");
        return DABGPU_ERR_UNSUPPORTED;
    }
    if (b->soft.policy != DABGPU_SOFT_CSI) {
        dabgpu_set_error("stream_bank_process: DQPSK products are set, their consumers need the frame's scale: the policy must be DABGPU_SOFT_CSI "
                         "(dabgpu_stream_bank_set_soft), it is the normalised one");
        return DABGPU_ERR_INVALID_ARG;
    }
    if (b->d_soft_scale == nullptr) {
        dabgpu_set_error("stream_bank_process: DQPSK products are set, their consumers need the frame's scale: dabgpu_stream_bank_set_soft was given no scale buffer");
        return DABGPU_ERR_INVALID_ARG;
    }
    if (slots_per_stream > b->products_cap / b->n) {
        dabgpu_set_error("stream_bank_process: %zu streams x %zu bits slots need more product frames than the %zu dabgpu_stream_bank_set_products was given",
                         b->n, slots_per_stream, b->products_cap);
        return DABGPU_ERR_INVALID_ARG;
    }
    return DABGPU_OK;
}

// n elements for *p, owned by `owner`
template <class T> static int bank_alloc(DeviceBuffer<>& owner, T** p, size_t n) {
    const int st = owner.alloc(n * sizeof(T), "hipMalloc(stream bank)");
    *p = static_cast<T*>(owner.get());
    return st;
}

extern "C" {

void dabgpu_stream_bank_destroy(dabgpu_stream_bank* b) {
    if (!dabgpu_destroy_begin(b, b ? b->ctx : nullptr)) return;
    delete b;
}

int dabgpu_stream_bank_reset(dabgpu_stream_bank* b, void* stream) {
    if (!b) { dabgpu_set_error("stream_bank_reset: null bank"); return DABGPU_ERR_INVALID_ARG; }
    DABGPU_BIND(b->ctx);
    hipStream_t s = (hipStream_t)stream;
    int st;
    DABGPU_CK(hipMemsetAsync(b->view.st, 0, b->n * sizeof(StreamState), s));
    DABGPU_CK(hipMemsetAsync(b->view.sync, 0, b->n * sizeof(dabgpu_sync_state), s));
    DABGPU_CK(hipMemsetAsync(b->view.sync_active, 0, b->n * sizeof(int), s));
    DABGPU_CK(hipMemsetAsync(b->view.desc, 0xFF, b->n * sizeof(dabgpu_frame_desc), s));
    DABGPU_CK(hipMemsetAsync(b->view.ring, 0, b->n * (size_t)b->view.g.null_period * sizeof(f2), s));
    DABGPU_CK(hipMemsetAsync(b->view.corr, 0, b->n * (size_t)b->view.g.n_corr * sizeof(f2), s));
    DABGPU_CK(hipMemsetAsync(b->view.copy_cnt, 0, b->n * sizeof(int), s));
    DABGPU_CK(hipMemsetAsync(b->view.not_done, 0, 16 * sizeof(int), s));
    b->carry_pending = false;
    return DABGPU_OK;
}

int dabgpu_stream_bank_create(dabgpu_ctx* c, size_t n_streams, const dabgpu_stream_cfg* cfg, dabgpu_stream_bank** out) {
    return dabgpu_stream_bank_create_mode(c, 1, n_streams, cfg, out);
}

int dabgpu_stream_bank_create_mode(dabgpu_ctx* c, int mode, size_t n_streams, const dabgpu_stream_cfg* cfg, dabgpu_stream_bank** out) {
    if (!c || !out || n_streams == 0 || n_streams > (size_t)(1 << 20)) { dabgpu_set_error("stream_bank_create: invalid argument"); return DABGPU_ERR_INVALID_ARG; }
    *out = nullptr;
    ModeGeom mg;
    if (!mode_geometry(mode, mg)) { dabgpu_set_error("stream_bank_create: invalid transmission mode %d", mode); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_stream_cfg k;
    if (cfg) k = *cfg; else dabgpu_stream_cfg_default(&k);
    if (k.signal_l1_nb_samples <= 0 || k.signal_l1_nb_decimate <= 0) { dabgpu_set_error("stream_bank_create: invalid L1 window"); return DABGPU_ERR_INVALID_ARG; }
    DABGPU_BIND(c);
    dabgpu_stream_bank* b = new (std::nothrow) dabgpu_stream_bank();
    if (!b) return DABGPU_ERR_HIP;
    b->ctx = c; b->n = n_streams; b->cfg = k;
    BankGeom& G = b->view.g;
    G.mode = mode; G.null_period = mg.null_period; G.period = mg.period; G.n_sym = mg.n_sym; G.n_fft = mg.n_fft;
    G.frame_samples = mg.frame_samples; G.n_corr = mg.null_period + mg.period; G.frame_bits = mg.frame_bits;
    int st = DABGPU_OK;
    DeviceBuffer<>* m = b->mem;
    if (!st) st = bank_alloc(*m++, &b->view.st, n_streams);
    if (!st) st = bank_alloc(*m++, &b->view.sync, n_streams);
    if (!st) st = bank_alloc(*m++, &b->view.ring, n_streams * (size_t)G.null_period);
    if (!st) st = bank_alloc(*m++, &b->view.corr, n_streams * (size_t)G.n_corr);
    if (!st) st = bank_alloc(*m++, &b->view.frame, n_streams * (size_t)G.frame_samples);
    if (!st) st = bank_alloc(*m++, &b->view.freq, n_streams);
    if (!st) st = bank_alloc(*m++, &b->view.sync_active, n_streams);
    if (!st) st = bank_alloc(*m++, &b->view.desc, n_streams);
    if (!st) st = bank_alloc(*m++, &b->view.copy_src, n_streams);
    if (!st) st = bank_alloc(*m++, &b->view.copy_dst, n_streams);
    if (!st) st = bank_alloc(*m++, &b->view.copy_cnt, n_streams);
    if (!st) st = bank_alloc(*m++, &b->view.not_done, 16);
    if (!st) st = bank_alloc(*m++, &b->d_corr_out, n_streams * (size_t)G.n_sym * 2);
    if (!st) st = bank_alloc(*m++, &b->d_status, n_streams);
    if (!st) st = b->side.create(hipStreamNonBlocking, "hipStreamCreate(stream bank)");
    if (!st) st = b->ev_fork.create(hipEventDisableTiming, "hipEventCreate");
    if (!st) st = b->ev_join.create(hipEventDisableTiming, "hipEventCreate");
    if (!st) st = dabgpu_stream_bank_reset(b, c->stream);
    if (!st) st = dabgpu_check_hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    if (st) { dabgpu_stream_bank_destroy(b); return st; }
    *out = b;
    return DABGPU_OK;
}

}  // extern "C"

// ring_mode: d_bits = [n_streams][max_frames_per_stream = ring length][230400], a completed frame goes to slot
// (frames demodulated so far) mod ring length, d_n_frames receives the slot written in this call or -1
template <int SRC>
static int bank_process_impl(dabgpu_stream_bank* b, const void* d_iq, size_t stream_stride_samples, size_t n_samples,
                             int8_t* d_bits, size_t max_frames_per_stream, int32_t* d_n_frames, void* stream, int ring_mode = 0,
                             int classed = 0, const void* d_prev = nullptr, int retain = 0) {
    if (!b || !d_iq || !d_bits) { dabgpu_set_error("stream_bank_process: null argument"); return DABGPU_ERR_INVALID_ARG; }
    if (n_samples == 0) return DABGPU_OK;
    if (b->carry_pending && (!d_prev || b->carry_src != SRC || b->carry_stride != stream_stride_samples)) {
        dabgpu_set_error("stream_bank_process: the previous call retained its block -- pass that block (same format and stride) to "
                         "dabgpu_stream_bank_process_retained, or call dabgpu_stream_bank_release first");
        return DABGPU_ERR_INVALID_ARG;
    }
    const BankGeom& G = b->view.g;
    const int NB_FRAME_SAMPLES = G.frame_samples, NB_CORR = G.n_corr, NB_NULL_PERIOD = G.null_period;
    // a frame needs at least n_sym symbols + a NULL minus the sync's pull-back of new samples
    const size_t need = ring_mode ? 1 : (n_samples / (size_t)(NB_FRAME_SAMPLES - NB_CORR) + 2);
    if (ring_mode && n_samples > (size_t)(NB_FRAME_SAMPLES - NB_CORR)) {
        dabgpu_set_error("stream_bank_process_ring: at most %d samples per call (one frame per stream per call)", NB_FRAME_SAMPLES - NB_CORR);
        return DABGPU_ERR_INVALID_ARG;
    }
    if (max_frames_per_stream < need || max_frames_per_stream > (size_t)(1 << 20) || b->n * max_frames_per_stream > (size_t)0x7FFFFFFF) {
        dabgpu_set_error("stream_bank_process: max_frames_per_stream must be at least %zu for %zu samples", need, n_samples);
        return DABGPU_ERR_INVALID_ARG;
    }
    if (((uintptr_t)d_iq & (src_sample_bytes<SRC>::value - 1)) || ((uintptr_t)d_bits & 15)) { dabgpu_set_error("stream_bank_process: misaligned buffer"); return DABGPU_ERR_INVALID_ARG; }
    if (int fits = bank_soft_scale_fits(b, max_frames_per_stream)) return fits;
    if (int fits = bank_products_fit(b, max_frames_per_stream, ring_mode)) return fits;
    dabgpu_ctx* c = b->ctx;
    DABGPU_BIND(c);
    hipStream_t s = (hipStream_t)stream;
    const int n = (int)b->n;
    int st;
    // Retained blocks (mode I): the unfinished frame at the end of a block is not copied into the stream's frame buffer -- the next
    // call reads it where it is.  A frame may then lie in the frame buffer, the previous block and the current block.  With blocks of
    // a frame's length or more every pending frame completes inside the next block; with the ring form's blocks (at most a frame
    // minus a correlation window) the few streams whose frame began in the last samples of the previous block copy those samples
    // themselves at the start of the call (stream_advance_kernel); a shorter block copies all carried samples first, like a release.
    const bool use_retain = retain && G.mode == 1;
    const bool prev_valid = b->carry_pending && n_samples >= (size_t)(NB_FRAME_SAMPLES - NB_CORR);
    if (b->carry_pending && !prev_valid) {
        hipLaunchKernelGGL(stream_copy_kernel<SRC>, dim3(COPY_WGS, (unsigned)n), dim3(256), 0, s, b->view, 0, static_cast<const uint8_t*>(d_prev),
                           stream_stride_samples);
        DABGPU_CK(hipGetLastError());
    }
    b->carry_pending = false;
    const uint8_t* prev_iq = prev_valid ? static_cast<const uint8_t*>(d_prev) : nullptr;
    // L1 windows of the signal-level IIR for every stream (grow-only scratch)
    const int k = b->cfg.signal_l1_nb_samples;
    if (n_samples >= (size_t)k) {
        const long long stride = (long long)k * b->cfg.signal_l1_nb_decimate;
        const long long n_win = ((long long)n_samples - k + stride - 1) / stride;
        if (b->win.needs((size_t)n * (size_t)n_win)) {
            DABGPU_CK(hipStreamSynchronize(s));
            b->view.win = nullptr; b->view.win_cap = 0;
            if ((st = b->win.regrow((size_t)n * (size_t)n_win, "hipMalloc((void**)&b->view.win, (size_t)n * (size_t)n_win * sizeof(float))"))) return st;
            b->view.win = b->win.get(); b->view.win_cap = n_win;
        }
        if (n_win > 0) {
            hipLaunchKernelGGL(stream_l1_kernel<SRC>, dim3((unsigned)((n_win + L1_WINDOWS - 1) / L1_WINDOWS), (unsigned)n), dim3(256), 0, s,
                               b->view, static_cast<const uint8_t*>(d_iq), stream_stride_samples, n_win, k, stride);
            DABGPU_CK(hipGetLastError());
        }
    }
    // rounds every locked stream needs: one per frame that can complete inside this block (the demodulation of frame k - 1 and the
    // synchronisation of frame k share a round) plus one for the partial frame at the end; a stream that needs more (re-acquisition)
    // is caught by the counter read back after these
    const int blind_rounds = (int)((n_samples + NB_FRAME_SAMPLES - 1) / NB_FRAME_SAMPLES) + 1;
    // Two lanes: the rounds of a stream are a serial chain (advance -> copy -> demodulate frame k - 1 -> phase -> synchronise frame k
    // -> advance ...) of one bandwidth-sized kernel and four latency-bound small ones, but streams are independent -- a mode I bank
    // of >= 1024 streams runs the two halves of its streams on two HIP streams, so that one half's small kernels run beside the other
    // half's demodulation.  Same kernels, same per-stream order, same results.
    const int n_lanes = (G.mode == 1 && n >= 1024) ? 2 : 1;      // (each half must still fill the chip: 256 streams lost 10-30 % in two lanes)
    hipStream_t lane_stream[2] = {s, b->side.get()};
    // products: a slot of this call without a frame has a zero record (sync_valid = 0), whatever an earlier call left there
    if (b->view.records != nullptr) DABGPU_CK(hipMemsetAsync(b->view.records, 0, (size_t)n * max_frames_per_stream * sizeof(dabgpu_sync_state), s));
    const int lane_lo[3] = {0, (n_lanes == 2) ? n / 2 : n, n};
    if (n_lanes == 2) {
        DABGPU_CK(hipEventRecord(b->ev_fork.get(), s));
        DABGPU_CK(hipStreamWaitEvent(b->side.get(), b->ev_fork.get(), 0));
    }
    // (an error inside the rounds must not leave work on the side stream unordered with the caller's stream: the caller may free the
    // block and the output buffers as soon as the call has returned)
#define CKS(status) do { st = (status); if (st) { if (n_lanes == 2) (void)hipStreamSynchronize(b->side.get()); return st; } } while (0)
#define CKL(call) CKS(dabgpu_check_hip((call), #call))
    const size_t sb = src_sample_bytes<SRC>::value;
    // run length of the bank's demodulation: four workgroups per frame (19 + 19 + 19 + 18 symbols).  Shorter-lived workgroups hand
    // their slots to the round's small kernels sooner: 256 streams +8 % against three per frame, 1024 streams +1 %; six per frame loses again
    const int bank_spb = 19;
    int h_not_done[2] = {1, 0};
    for (int round = 0; h_not_done[0] + h_not_done[1] != 0; round++) {
        for (int l = 0; l < n_lanes; l++) {
            hipStream_t ls = lane_stream[l];
            const int s0 = lane_lo[l], cnt = lane_lo[l + 1] - lane_lo[l];
            const uint8_t* iq_l = static_cast<const uint8_t*>(d_iq) + (size_t)s0 * stream_stride_samples * sb;
            if (round == 0) CKL(hipMemsetAsync(b->view.not_done + 8 * l, 0, sizeof(int), ls));
            hipLaunchKernelGGL(stream_advance_kernel<SRC>, dim3((unsigned)cnt), dim3(256), 0, ls, b->view, s0, cnt, static_cast<const uint8_t*>(d_iq),
                               stream_stride_samples, (long long)n_samples, b->cfg, (int)max_frames_per_stream, round == 0 ? 1 : 0, ring_mode,
                               b->view.not_done + 8 * l + (round & 7), b->view.not_done + 8 * l + ((round + 1) & 7), prev_iq, use_retain ? 1 : 0);
            CKL(hipGetLastError());
            float* corr_l = b->d_corr_out + (size_t)s0 * G.n_sym * 2;
            // (modes II-IV run in one lane: n_lanes == 1, s0 == 0, cnt == n)
            dabgpu_demod_call call;
            call.d_iq = b->view.frame + (size_t)s0 * G.frame_samples; call.src = SRC; call.d_freq = b->view.freq + s0;
            call.d_bits = d_bits; call.classed = classed; call.d_cp_corr = corr_l;
            call.n_frames = cnt; call.symbols_per_block = bank_spb;
            call.d_desc = b->view.desc + s0; call.d_block = iq_l; call.block_stride = stream_stride_samples;
            call.d_prev_block = prev_iq ? prev_iq + (size_t)s0 * stream_stride_samples * sb : nullptr;
            if (b->soft.policy == DABGPU_SOFT_CSI) {         // (mode I banks only: set_soft refuses the others)
                call.bank_soft = true; call.soft_policy = DABGPU_SOFT_CSI; call.soft_level = b->soft.level; call.d_soft_scale = b->d_soft_scale;
                if (b->d_products != nullptr) { call.bank_products = true; call.d_bank_dqpsk = b->d_products; }      // (both lanes: global slots)
            }
            CKS(dabgpu_launch_demod(c, G.mode, call, ls));
            CKL(dabgpu_launch_ofdm_phase(corr_l, cnt, b->cfg.sync.fine_freq_update_beta, nullptr, &b->view.sync[s0].freq_fine,
                                        (int)(sizeof(dabgpu_sync_state) / sizeof(float)), b->view.desc + s0, G.n_sym, G.n_fft, ls));
            // (after the phase kernel: the synchroniser of frame k sees the fine frequency the phase of frame k - 1 left, as in the reference)
            CKS(dabgpu_launch_sync(c, G.mode, reinterpret_cast<const float*>(b->view.corr + (size_t)s0 * NB_CORR + NB_NULL_PERIOD), NB_CORR, cnt, &b->cfg.sync,
                                   b->view.sync + s0, nullptr, nullptr, b->view.sync_active + s0, ls));
        }
        if (round + 1 >= blind_rounds) {
            for (int l = 0; l < n_lanes; l++) CKL(hipMemcpyAsync(&h_not_done[l], b->view.not_done + 8 * l + (round & 7), sizeof(int), hipMemcpyDeviceToHost, lane_stream[l]));
            for (int l = 0; l < n_lanes; l++) CKL(hipStreamSynchronize(lane_stream[l]));
        }
        if (round > (1 << 22)) { dabgpu_set_error("stream_bank_process: no progress"); if (n_lanes == 2) (void)hipStreamSynchronize(b->side.get()); return DABGPU_ERR_HIP; }
    }
    for (int l = 0; l < n_lanes && !use_retain; l++) {                    // the carry-over copies of the call, every lane its own streams
        hipLaunchKernelGGL(stream_copy_kernel<SRC>, dim3(COPY_WGS, (unsigned)(lane_lo[l + 1] - lane_lo[l])), dim3(256), 0, lane_stream[l], b->view,
                           lane_lo[l], static_cast<const uint8_t*>(d_iq), stream_stride_samples);
        CKL(hipGetLastError());
    }
#undef CKL
#undef CKS
    if (n_lanes == 2) {
        DABGPU_CK(hipEventRecord(b->ev_join.get(), b->side.get()));
        DABGPU_CK(hipStreamWaitEvent(s, b->ev_join.get(), 0));
    }
    if (d_n_frames) {
        hipLaunchKernelGGL(stream_report_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, b->view, n, d_n_frames,
                           (dabgpu_stream_status*)nullptr, ring_mode ? (int)max_frames_per_stream : 0);
        DABGPU_CK(hipGetLastError());
    }
    if (use_retain) { b->carry_pending = true; b->carry_src = SRC; b->carry_stride = stream_stride_samples; }
    return DABGPU_OK;
}

// bank_process_impl for the loader src (0..3, dabgpu_fused_loader) of the block's capture format
template <class... A>
static int bank_process_src(int src, A... a) {
    switch (src) {
    case 0: return bank_process_impl<0>(a...);
    case 1: return bank_process_impl<1>(a...);
    case 2: return bank_process_impl<2>(a...);
    case 3: return bank_process_impl<3>(a...);
    default: dabgpu_set_error("stream_bank_process: no loader %d", src); return DABGPU_ERR_INVALID_ARG;
    }
}

// dabgpu_stream_bank_release: copies what the last retained call left in its block into the frame buffers
static int bank_release_src(dabgpu_stream_bank* b, int src, const void* d_prev, size_t stream_stride_samples, void* stream) {
    if (b->carry_src != src || b->carry_stride != stream_stride_samples) {        // (carry_src: the loader of a bank_process_impl<SRC>)
        dabgpu_set_error("stream_bank_release: not the format / stride of the retained block"); return DABGPU_ERR_INVALID_ARG;
    }
    DABGPU_BIND(b->ctx);
    static void (*const copy[4])(BankView, int, const uint8_t*, size_t) = {stream_copy_kernel<0>, stream_copy_kernel<1>, stream_copy_kernel<2>,
                                                                           stream_copy_kernel<3>};
    hipLaunchKernelGGL(copy[src], dim3(COPY_WGS, (unsigned)b->n), dim3(256), 0, (hipStream_t)stream, b->view, 0,
                       static_cast<const uint8_t*>(d_prev), stream_stride_samples);
    const int st = dabgpu_check_hip(hipGetLastError(), "stream_copy_kernel launch");
    if (st) return st;
    // (the copy records stay set; the next call's first round clears them -- it is handed no previous block, so nothing is carried)
    b->carry_pending = false;
    return DABGPU_OK;
}

extern "C" {

int dabgpu_stream_bank_process_retained(dabgpu_stream_bank* b, const void* d_raw, int format, size_t stream_stride_samples, size_t n_samples,
                                        const void* d_prev_raw, int8_t* d_bits, size_t max_frames_per_stream, int32_t* d_n_frames, void* stream) {
    if (!b || !d_raw) { dabgpu_set_error("stream_bank_process_retained: null argument"); return DABGPU_ERR_INVALID_ARG; }
    if (n_samples == 0) return DABGPU_OK;
    const int src = dabgpu_fused_loader(format);
    if (src < 0) {
        dabgpu_set_error("stream_bank_process_retained: format %d is not read by the bank's kernels directly (raw_f32l, raw_u8, raw_s8, raw_s16l, wav PCM8 / PCM16 / float32)", format);
        return DABGPU_ERR_INVALID_ARG;
    }
    return bank_process_src(src, b, d_raw, stream_stride_samples, n_samples, d_bits, max_frames_per_stream, d_n_frames, stream, 0, 0, d_prev_raw, 1);
}

int dabgpu_stream_bank_release(dabgpu_stream_bank* b, const void* d_prev_raw, int format, size_t stream_stride_samples, void* stream) {
    if (!b) { dabgpu_set_error("stream_bank_release: null bank"); return DABGPU_ERR_INVALID_ARG; }
    if (!b->carry_pending) return DABGPU_OK;
    if (!d_prev_raw) { dabgpu_set_error("stream_bank_release: null block"); return DABGPU_ERR_INVALID_ARG; }
    const int src = dabgpu_fused_loader(format);
    if (src < 0) { dabgpu_set_error("stream_bank_release: not the format of the retained block"); return DABGPU_ERR_INVALID_ARG; }
    return bank_release_src(b, src, d_prev_raw, stream_stride_samples, stream);
}

int dabgpu_stream_bank_process(dabgpu_stream_bank* b, const float* d_iq, size_t stream_stride_samples, size_t n_samples,
                               int8_t* d_bits, size_t max_frames_per_stream, int32_t* d_n_frames, void* stream) {
    return bank_process_impl<0>(b, d_iq, stream_stride_samples, n_samples, d_bits, max_frames_per_stream, d_n_frames, stream);
}

// the same from blocks still in their capture format: dequantised on the device (iq_convert_kernel, reader arithmetic of
// examples/app_helpers/app_iq_readers.h) into bank-owned scratch on `stream`, then processed as above
int dabgpu_stream_bank_process_raw(dabgpu_stream_bank* b, const void* d_raw, int format, size_t stream_stride_samples, size_t n_samples,
                                   int8_t* d_bits, size_t max_frames_per_stream, int32_t* d_n_frames, void* stream) {
    if (!b || !d_raw) { dabgpu_set_error("stream_bank_process_raw: null argument"); return DABGPU_ERR_INVALID_ARG; }
    const size_t sb = dabgpu_iq_format_sample_bytes(format);
    if (sb == 0) { dabgpu_set_error("stream_bank_process_raw: unknown format %d", format); return DABGPU_ERR_INVALID_ARG; }
    if (n_samples == 0) return DABGPU_OK;
    // formats the kernels read by themselves: no conversion pass, 2-4 bytes per sample from HBM instead of 8
    const int src = dabgpu_fused_loader(format);
    if (src >= 0) return bank_process_src(src, b, d_raw, stream_stride_samples, n_samples, d_bits, max_frames_per_stream, d_n_frames, stream);
    if (((stream_stride_samples * sb) & 15) != 0 && b->n > 1) {
        dabgpu_set_error("stream_bank_process_raw: the byte stride between streams must be a multiple of 16"); return DABGPU_ERR_INVALID_ARG;
    }
    if (int fits = bank_soft_scale_fits(b, max_frames_per_stream)) return fits;          // (before the conversion is launched)
    if (int fits = bank_products_fit(b, max_frames_per_stream, 0)) return fits;
    DABGPU_BIND(b->ctx);
    hipStream_t s = (hipStream_t)stream;
    const size_t padded = (n_samples + 1) & ~(size_t)1;                   // keeps every stream's converted block 16-byte aligned
    const size_t need = b->n * padded * 2;                                // floats
    if (b->raw_scratch.needs(need)) {
        int st = dabgpu_check_hip(hipStreamSynchronize(s), "hipStreamSynchronize");
        if (st || (st = b->raw_scratch.regrow(need, "hipMalloc(stream bank raw scratch)"))) return st;
    }
    for (size_t k = 0; k < b->n; k++) {
        const int st = dabgpu_iq_convert(b->ctx, static_cast<const uint8_t*>(d_raw) + k * stream_stride_samples * sb, format, n_samples,
                                         b->raw_scratch.get() + k * padded * 2, stream);
        if (st) return st;
    }
    return dabgpu_stream_bank_process(b, b->raw_scratch.get(), padded, n_samples, d_bits, max_frames_per_stream, d_n_frames, stream);
}

// frames go straight into per-stream frame-history rings (the layout dabgpu_fic_decode_ring / dabgpu_msc_decode_ring read)
static int bank_process_ring_any(dabgpu_stream_bank* b, const void* d_raw, int format, size_t stream_stride_samples, size_t n_samples,
                                 int8_t* d_hist, int hist_frames, int32_t* d_newest_slot, int bits_layout, void* stream, const void* d_prev, int retain) {
    if (!b || !d_raw || !d_hist || !d_newest_slot) { dabgpu_set_error("stream_bank_process_ring: null argument"); return DABGPU_ERR_INVALID_ARG; }
    if (int fits = bank_products_fit(b, (size_t)(hist_frames > 0 ? hist_frames : 0), 1)) return fits;
    if (hist_frames < 5) { dabgpu_set_error("stream_bank_process_ring: the ring needs at least 5 frames"); return DABGPU_ERR_INVALID_ARG; }
    const int st = dabgpu_check_bits_layout("stream_bank_process_ring", bits_layout);
    if (st) return st;
    const int classed = bits_layout == DABGPU_BITS_MSC_CLASSED;
    if (classed && b->view.g.mode != 1) {
        dabgpu_set_error("stream_bank_process_ring: class order is defined for transmission mode I (the DAB layer above the soft bits is mode I only)");
        return DABGPU_ERR_UNSUPPORTED;
    }
    const int src = dabgpu_fused_loader(format);
    if (src < 0) {
        dabgpu_set_error("stream_bank_process_ring: format %d is not read directly (use raw_f32l, raw_u8, raw_s8 or raw_s16l)", format);
        return DABGPU_ERR_UNSUPPORTED;
    }
    return bank_process_src(src, b, d_raw, stream_stride_samples, n_samples, d_hist, (size_t)hist_frames, d_newest_slot, stream, 1, classed, d_prev, retain);
}

int dabgpu_stream_bank_process_ring_layout(dabgpu_stream_bank* b, const void* d_raw, int format, size_t stream_stride_samples, size_t n_samples,
                                           int8_t* d_hist, int hist_frames, int32_t* d_newest_slot, int bits_layout, void* stream) {
    return bank_process_ring_any(b, d_raw, format, stream_stride_samples, n_samples, d_hist, hist_frames, d_newest_slot, bits_layout, stream, nullptr, 0);
}

int dabgpu_stream_bank_process_ring_retained(dabgpu_stream_bank* b, const void* d_raw, int format, size_t stream_stride_samples, size_t n_samples,
                                             const void* d_prev_raw, int8_t* d_hist, int hist_frames, int32_t* d_newest_slot, int bits_layout,
                                             void* stream) {
    return bank_process_ring_any(b, d_raw, format, stream_stride_samples, n_samples, d_hist, hist_frames, d_newest_slot, bits_layout, stream, d_prev_raw, 1);
}

int dabgpu_stream_bank_process_ring(dabgpu_stream_bank* b, const void* d_raw, int format, size_t stream_stride_samples, size_t n_samples,
                                    int8_t* d_hist, int hist_frames, int32_t* d_newest_slot, void* stream) {
    return dabgpu_stream_bank_process_ring_layout(b, d_raw, format, stream_stride_samples, n_samples, d_hist, hist_frames, d_newest_slot,
                                                  DABGPU_BITS_NATURAL, stream);
}

int dabgpu_stream_bank_set_soft(dabgpu_stream_bank* b, const dabgpu_soft_cfg* cfg, float* d_soft_scale, size_t scale_capacity) {
    if (!b) { dabgpu_set_error("stream_bank_set_soft: null bank"); return DABGPU_ERR_INVALID_ARG; }
    const int st = dabgpu_host_check_soft_cfg("stream_bank_set_soft", cfg);
    if (st) return st;
    if (cfg->policy != DABGPU_SOFT_NORMALISED && b->view.g.mode != 1) {
        dabgpu_set_error("stream_bank_set_soft: the weighted soft bits exist for transmission mode I banks only (mode %d)", b->view.g.mode);
        return DABGPU_ERR_UNSUPPORTED;
    }
    if ((uintptr_t)d_soft_scale & 3) { dabgpu_set_error("stream_bank_set_soft: misaligned scale buffer"); return DABGPU_ERR_INVALID_ARG; }
    b->soft = *cfg;
    b->d_soft_scale = d_soft_scale;
    b->soft_scale_cap = d_soft_scale ? scale_capacity : 0;
    return DABGPU_OK;
}

int dabgpu_stream_bank_get_soft(const dabgpu_stream_bank* b, dabgpu_soft_cfg* cfg) {
    if (!b || !cfg) { dabgpu_set_error("stream_bank_get_soft: null argument"); return DABGPU_ERR_INVALID_ARG; }
    *cfg = b->soft;
    return DABGPU_OK;
}

int dabgpu_stream_bank_set_products(dabgpu_stream_bank* b, float* d_dqpsk, dabgpu_sync_state* d_records, size_t capacity_frames) {
    if (!b) { dabgpu_set_error("stream_bank_set_products: null bank"); return DABGPU_ERR_INVALID_ARG; }
    if ((d_dqpsk == nullptr) != (d_records == nullptr)) {
        dabgpu_set_error("stream_bank_set_products: the products and the records go together (both, or both NULL to switch them off)");
        return DABGPU_ERR_INVALID_ARG;
    }
    if (d_dqpsk != nullptr) {
        if (b->view.g.mode != 1) {
            dabgpu_set_error("stream_bank_set_products: the DQPSK products exist for transmission mode I banks only (mode %d)", b->view.g.mode);
            return DABGPU_ERR_UNSUPPORTED;
        }
        if (((uintptr_t)d_dqpsk & 15) || ((uintptr_t)d_records & 3)) { dabgpu_set_error("stream_bank_set_products: misaligned buffer"); return DABGPU_ERR_INVALID_ARG; }
        if (capacity_frames == 0 || capacity_frames > (size_t)0x7FFFFFFF) {
            dabgpu_set_error("stream_bank_set_products: capacity_frames %zu outside 1 .. 2^31 - 1", capacity_frames); return DABGPU_ERR_INVALID_ARG;
        }
    }
    b->d_products = d_dqpsk;
    b->view.records = d_records;
    b->products_cap = d_dqpsk ? capacity_frames : 0;
    return DABGPU_OK;
}

int dabgpu_stream_bank_get_products(const dabgpu_stream_bank* b, float** d_dqpsk, dabgpu_sync_state** d_records, size_t* capacity_frames) {
    if (!b) { dabgpu_set_error("stream_bank_get_products: null bank"); return DABGPU_ERR_INVALID_ARG; }
    if (d_dqpsk) *d_dqpsk = b->d_products;
    if (d_records) *d_records = b->view.records;
    if (capacity_frames) *capacity_frames = b->products_cap;
    return DABGPU_OK;
}

int dabgpu_stream_bank_status(dabgpu_stream_bank* b, dabgpu_stream_status* h_status, void* stream) {
    if (!b || !h_status) { dabgpu_set_error("stream_bank_status: null argument"); return DABGPU_ERR_INVALID_ARG; }
    DABGPU_BIND(b->ctx);
    hipStream_t s = (hipStream_t)stream;
    const int n = (int)b->n;
    int st;
    hipLaunchKernelGGL(stream_report_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, b->view, n, (int*)nullptr, b->d_status, 0);
    if ((st = dabgpu_check_hip(hipGetLastError(), "stream_report_kernel launch"))) return st;
    if ((st = dabgpu_check_hip(hipMemcpyAsync(h_status, b->d_status, b->n * sizeof(dabgpu_stream_status), hipMemcpyDeviceToHost, s), "hipMemcpyAsync"))) return st;
    return dabgpu_check_hip(hipStreamSynchronize(s), "hipStreamSynchronize");
}

}  // extern "C"
