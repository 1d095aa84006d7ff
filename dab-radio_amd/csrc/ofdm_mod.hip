// ofdm_mod.hip -- the OFDM transmitter on the device: OFDM_Modulator::ProcessBlock (src/ofdm/ofdm_modulator.cpp:49-156) for a batch of
// independent frames, optionally followed by the frequency shift and 8-bit quantisation of examples/simulate_transmitter.cpp:167-178.
// Per frame, NULL first (transmission order):
//   NULL period            zeros, or (dabgpu_ofdm_modulate_frames_tii, mode I) the frame's TII symbol: the inverse transform of the comb
//                          spectrum of its transmitters (tii_core.h) behind its last 608 samples
//   PRS symbol             IFFT(PRS spectrum), cyclic prefix = its last nb_cyclic_prefix samples
//   data symbols 1..L-1    X_s = X_{s-1} * z_s per carrier (X_0 = the PRS bin; re = x.re*z.re - x.im*z.im, im = x.re*z.im + x.im*z.re,
//                          no fused operations), IFFT, cyclic prefix
// z_s comes from the payload in one of two layouts (include/dabgpu.h, DABGPU_TX_PAYLOAD_*): the reference's 2 bits per carrier in
// natural carrier order through PHASE_MAP, or the frame's hard bits in the demodulator's de-interleaved layout (bit n = real part of
// carrier mapper[n], bit n + NC = its imaginary part, z = ((1 - 2 b_n) + j (1 - 2 b_{n+NC})) * A) -- the ETSI frequency interleaver.
// The inverse transforms are the ones the PRS synchronisation runs (ofdm_fft_lds.h), bit for bit the oracle's dab_ifft2048 / dab_fft_n.
// Output: complex float, or the u8 pairs of QuantisedIQ<uint8_t>::from_iq(I * scale, Q * scale), scale = (1 / NC * 4) * 127.5
// (examples/app_helpers/app_iq_readers.h:19-63).  freq_norm != 0: apply_pll(frame, freq_norm) first, phase 0 at the frame's first
// (NULL) sample, in the PLL contract of DESIGN.md 3.1.
//
// Mode I: one 256-thread workgroup per (frame, run of symbols); thread t owns carriers t + 256 j (j < 6) and keeps their X in registers.
// A run that starts at symbol s0 > 1 first replays the chain through s0 - 1 (complex multiplies only), so that small batches still
// spread over the chip.  Spectrum -> LDS -> fft2048_lds (inverse, in place) -> the symbol period two samples per store (16 bytes of
// complex float, 4 bytes of u8 pairs): every symbol starts on a 16-byte boundary in both formats (2656 * 8, 2552 * 8, 2656 * 2 and
// 2552 * 2 are multiples of 16).
// Modes II-IV: the same per (frame, run) through fft_lds's Stockham passes, one sample per store (no speed target).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "ofdm_device.h"
#include "ofdm_fft_lds.h"
#include "tii_core.h"

namespace dabgpu {

constexpr int TX_NULL = 2656;                 // mode I NULL period
constexpr int TX_NC = 1536;
constexpr int TX_CPT = TX_NC / 256;           // carriers per thread (mode I)
constexpr int TX_SYM_BYTES = TX_NC / 4;       // payload bytes per data symbol, both layouts
constexpr int TX_FRAME_BYTES = (NB_FRAME_SYMBOLS - 1) * TX_SYM_BYTES;
constexpr float TX_A_REF = 1.0f / 1.41421356237309505f;      // 1.0f / std::sqrt(2.0f) (ofdm_modulator.cpp:101)
constexpr float TX_A_BITS = 0.707106769084930420f;

// the differential step in the oracle's operation order (no FMA: the file is built with -ffp-contract=off)
__device__ __forceinline__ f2 tx_mul(f2 x, f2 z) { return mk2(x.x * z.x - x.y * z.y, x.x * z.y + x.y * z.x); }

// PHASE_MAP = {(-A,-A), (A,-A), (A,A), (-A,A)} (ofdm_modulator.cpp:102)
__device__ __forceinline__ f2 tx_phase_map(uint32_t v) {
    return mk2((v == 1u || v == 2u) ? TX_A_REF : -TX_A_REF, (v >= 2u) ? TX_A_REF : -TX_A_REF);
}
__device__ __forceinline__ f2 tx_bits_map(uint32_t b_re, uint32_t b_im) { return mk2(b_re ? -TX_A_BITS : TX_A_BITS, b_im ? -TX_A_BITS : TX_A_BITS); }

// frequency shift of frame sample m (apply_pll over the whole frame from sample 0: groups of 4 throughout, frames are multiples of 4)
template <bool PLL>
__device__ __forceinline__ f2 tx_shift(f2 v, int m, int frame_samples, float f) {
    if constexpr (PLL) return pll_any(v, m, frame_samples, f, 0.0f);
    else return v;
}

// QuantisedIQ<uint8_t>::from_iq(x * scale, ...): + BIAS, clamp to [0, 255] (NaN -> 0), truncate
__device__ __forceinline__ uint32_t tx_u8(float x, float scale) {
    float v = x * scale;
    v = v + 127.5f;
    v = (v > 0.0f) ? v : 0.0f;
    v = (v > 255.0f) ? 255.0f : v;
    return (uint32_t)v;
}
__device__ __forceinline__ uint32_t tx_u8_pair(f2 v, float scale) { return tx_u8(v.x, scale) | (tx_u8(v.y, scale) << 8); }

typedef float tx_f4 __attribute__((ext_vector_type(4)));

// samples n, n + 1 of a symbol period of mode I from the inverse transform in A (natural order), shifted, converted and stored as one
// 16-byte (F32) or 4-byte (U8) store; m = frame sample of n, o = output sample of n.  (U8 in pairs too: with the shift its cost is the
// per-sample PLL, and 1276 pairs keep every thread of the workgroup busy where 319 groups of 8 left 3/8 of the second pass idle.)
template <int OUT, bool PLL>
__device__ __forceinline__ void tx_store_pair(f2 a, f2 b, int m, size_t o, float f, float scale, void* __restrict__ out) {
    const f2 v0 = tx_shift<PLL>(a, m, NB_FRAME_SAMPLES, f);
    const f2 v1 = tx_shift<PLL>(b, m + 1, NB_FRAME_SAMPLES, f);
    // complex float: non-temporal 16-byte stores (the frames stream out once; tools/bench_tx.py, 4096 frames: 1.44 ms against 1.79 ms plain)
    if constexpr (OUT == DABGPU_IQ_RAW_F32L)
        __builtin_nontemporal_store(tx_f4{v0.x, v0.y, v1.x, v1.y}, reinterpret_cast<tx_f4*>(static_cast<float*>(out) + 2 * o));
    else *reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(out) + 2 * o) = tx_u8_pair(v0, scale) | (tx_u8_pair(v1, scale) << 16);
}

// payload of data symbol s (1-based) for thread t's six carriers, loaded one symbol ahead of its use
template <int LAYOUT>
struct TxRaw { uint32_t b[LAYOUT == DABGPU_TX_PAYLOAD_REFERENCE ? TX_CPT : 2 * TX_CPT]; };

template <int LAYOUT>
__device__ __forceinline__ TxRaw<LAYOUT> tx_load_mode1(const uint8_t* __restrict__ sym, int t, const int (&nbit)[TX_CPT]) {
    TxRaw<LAYOUT> r;
#pragma unroll
    for (int j = 0; j < TX_CPT; j++) {
        if constexpr (LAYOUT == DABGPU_TX_PAYLOAD_REFERENCE) {
            r.b[j] = sym[(t >> 2) + 64 * j];                                // carrier t + 256 j: byte c / 4
        } else {
            r.b[2 * j] = sym[nbit[j] >> 3];                                  // bit n, n = inv_map[c]
            r.b[2 * j + 1] = sym[(nbit[j] + TX_NC) >> 3];                    // bit n + NC
        }
    }
    return r;
}

template <int LAYOUT>
__device__ __forceinline__ void tx_step_mode1(f2 (&X)[TX_CPT], const TxRaw<LAYOUT>& r, int t, const int (&nbit)[TX_CPT]) {
#pragma unroll
    for (int j = 0; j < TX_CPT; j++) {
        f2 z;
        if constexpr (LAYOUT == DABGPU_TX_PAYLOAD_REFERENCE) z = tx_phase_map((r.b[j] >> (2 * (t & 3))) & 3u);
        else z = tx_bits_map((r.b[2 * j] >> (nbit[j] & 7)) & 1u, (r.b[2 * j + 1] >> (nbit[j] & 7)) & 1u);
        X[j] = tx_mul(X[j], z);
    }
}

// the TII symbol of a frame with n_tx > 0 transmitters in the NULL period (include/dabgpu.h, "TII"): the spectra add in list order, one
// carrier per thread and transmitter (a transmitter's 32 carriers are distinct; two transmitters may meet on one, hence the barrier)
template <int OUT, bool PLL>
__device__ __forceinline__ void tx_null_tii(f2* A, const Fft2048Tw& w, const f2* __restrict__ prs, const dabgpu_tii_tx* __restrict__ list, int n_tx,
                                            size_t o_frame, float f, float scale, void* __restrict__ out) {
    const int t = threadIdx.x;
#pragma unroll
    for (int r = 0; r < 8; r++) A[t + 256 * r] = mk2(0.0f, 0.0f);
    __syncthreads();
    for (int i = 0; i < n_tx; i++) {
        const dabgpu_tii_tx tx = list[i];
        if (t < 32 && tx.main_id < TII_NB_MAIN && tx.sub_id < TII_COMBS) {
            int k0;
            const int k = tii_carrier(tx.main_id, tx.sub_id, t, &k0);
            const f2 ph = prs[tii_bin(k0)], z = A[tii_bin(k)];
            A[tii_bin(k)] = mk2(z.x + tx.amp * ph.x, z.y + tx.amp * ph.y);
        }
        __syncthreads();
    }
    fft2048_lds(A, w, true);
    for (int q = t; q < TX_NULL / 2; q += 256) {
        const int n = 2 * q, i = (n < TII_PREFIX) ? n + (NB_FFT - TII_PREFIX) : n - TII_PREFIX;   // prefix = the transform's last 608 samples
        tx_store_pair<OUT, PLL>(A[i], A[i + 1], n, o_frame + n, f, scale, out);
    }
    __syncthreads();                                                   // every sample read before the PRS spectrum goes in
}

// mode I: one 256-thread workgroup per (frame, run of symbols [s0, s1)); symbol 0 is the PRS, the run holding it also writes the NULL
// (TII: tii [n_frames][4] and tii_count [n_frames] say what the NULL carries; !TII: neither is read)
template <int OUT, int LAYOUT, bool PLL, bool TII>
__global__ __launch_bounds__(256)
void ofdm_mod_kernel(const uint8_t* __restrict__ payload, const f2* __restrict__ prs, const f2* __restrict__ tw,
                     const uint16_t* __restrict__ inv_map, int n_frames, int sym_per_run, int runs_per_frame, float f, float scale,
                     void* __restrict__ out, const dabgpu_tii_tx* __restrict__ tii, const uint8_t* __restrict__ tii_count)
{
    __shared__ __attribute__((aligned(16))) f2 A[4 * WAVE_PATCH];
    const int t = threadIdx.x;
    const int frame = blockIdx.x / runs_per_frame, run = blockIdx.x % runs_per_frame;
    if (frame >= n_frames) return;
    const int s0 = run * sym_per_run, s1 = min(s0 + sym_per_run, NB_FRAME_SYMBOLS);
    const Fft2048Tw w = fft2048_twiddles(tw);
    const uint8_t* pl = payload + (size_t)frame * TX_FRAME_BYTES;      // data symbol s (>= 1) at pl + (s - 1) * TX_SYM_BYTES
    const size_t o_frame = (size_t)frame * NB_FRAME_SAMPLES;

    int bin[TX_CPT], nbit[TX_CPT];
    f2 X[TX_CPT];
#pragma unroll
    for (int j = 0; j < TX_CPT; j++) {
        const int c = t + 256 * j;
        bin[j] = (c < TX_NC / 2) ? NB_FFT - TX_NC / 2 + c : c - TX_NC / 2 + 1;
        nbit[j] = (LAYOUT == DABGPU_TX_PAYLOAD_FRAME_BITS) ? (int)inv_map[c] : 0;
        X[j] = prs[bin[j]];
    }
    // replay the carrier chain up to the run's first symbol
    for (int s = 1; s < s0; s++) tx_step_mode1<LAYOUT>(X, tx_load_mode1<LAYOUT>(pl + (size_t)(s - 1) * TX_SYM_BYTES, t, nbit), t, nbit);

    if (s0 == 0) {
        int n_tx = 0;
        if constexpr (TII) n_tx = min((int)tii_count[frame], DABGPU_TII_MAX_TX);
        if (n_tx > 0) tx_null_tii<OUT, PLL>(A, w, prs, tii + (size_t)frame * DABGPU_TII_MAX_TX, n_tx, o_frame, f, scale, out);
        else                                                           // the NULL period: zeros through the same shift and conversion
            for (int q = t; q < TX_NULL / 2; q += 256) tx_store_pair<OUT, PLL>(mk2(0.0f, 0.0f), mk2(0.0f, 0.0f), 2 * q, o_frame + 2 * q, f, scale, out);
    }

    TxRaw<LAYOUT> raw = {};
    if (s0 >= 1) raw = tx_load_mode1<LAYOUT>(pl + (size_t)(s0 - 1) * TX_SYM_BYTES, t, nbit);
    for (int s = s0; s < s1; s++) {
        if (s == 0) {                                                  // PRS symbol: the whole spectrum as given (guard bins included)
#pragma unroll
            for (int r = 0; r < 8; r++) A[t + 256 * r] = prs[t + 256 * r];
        } else {
            tx_step_mode1<LAYOUT>(X, raw, t, nbit);
#pragma unroll
            for (int j = 0; j < TX_CPT; j++) A[bin[j]] = X[j];
#pragma unroll
            for (int k = t; k < NB_FFT - TX_NC; k += 256) A[k == 0 ? 0 : TX_NC / 2 + k] = mk2(0.0f, 0.0f);   // DC and the guard band
        }
        if (s + 1 < s1) raw = tx_load_mode1<LAYOUT>(pl + (size_t)s * TX_SYM_BYTES, t, nbit);   // (in flight during the transform)
        __syncthreads();
        fft2048_lds(A, w, true);
        const int m0 = TX_NULL + s * NB_SYMBOL_PERIOD;                  // frame sample of the period's first sample
        for (int q = t; q < NB_SYMBOL_PERIOD / 2; q += 256) {
            const int n = 2 * q, i = (n < NB_CP) ? n + (NB_FFT - NB_CP) : n - NB_CP;    // cyclic prefix = the transform's last NB_CP samples
            tx_store_pair<OUT, PLL>(A[i], A[i + 1], m0 + n, o_frame + m0 + n, f, scale, out);
        }
        __syncthreads();                                               // every period sample read before the next spectrum goes in
    }
}

// modes II-IV (any mode but I): one 256-thread workgroup per (frame, run of symbols), fft_lds's Stockham passes (x -> y), one sample per store
constexpr int TXG_CPT = 3;                     // carriers per thread: up to 768 (mode IV)
template <int OUT, int LAYOUT, bool PLL>
__global__ __launch_bounds__(256)
void ofdm_mod_mode_kernel(int mode, const uint8_t* __restrict__ payload, const f2* __restrict__ prs, const f2* __restrict__ tw,
                          const int* __restrict__ inv_map, int n_frames, int sym_per_run, int runs_per_frame, float f, float scale,
                          void* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) f2 B[3 * 1024];
    ModeGeom g;
    mode_geometry(mode, g);
    const int N = g.n_fft, NC = g.n_carriers, M = NC / 2, sym_bytes = NC / 4;
    f2* x = B;
    f2* y = B + N;
    f2* tmp = B + 2 * N;
    const int t = threadIdx.x;
    const int frame = blockIdx.x / runs_per_frame, run = blockIdx.x % runs_per_frame;
    if (frame >= n_frames) return;
    const int s0 = run * sym_per_run, s1 = min(s0 + sym_per_run, g.n_sym);
    const Fft2048Tw w2048 = {};                                        // (unused: N < 2048)
    const uint8_t* pl = payload + (size_t)frame * (size_t)((g.n_sym - 1) * sym_bytes);    // data symbol s at pl + (s - 1) * sym_bytes
    const size_t o_frame = (size_t)frame * g.frame_samples;

    int bin[TXG_CPT], nbit[TXG_CPT];
    f2 X[TXG_CPT];
#pragma unroll
    for (int j = 0; j < TXG_CPT; j++) {
        const int c = t + 256 * j;
        const bool on = c < NC;
        bin[j] = !on ? 0 : (c < M ? N - M + c : c - M + 1);
        nbit[j] = (on && LAYOUT == DABGPU_TX_PAYLOAD_FRAME_BITS) ? inv_map[c] : 0;
        X[j] = on ? prs[bin[j]] : mk2(0.0f, 0.0f);
    }
    auto step = [&](int s) {
        const uint8_t* sym = pl + (size_t)(s - 1) * sym_bytes;
#pragma unroll
        for (int j = 0; j < TXG_CPT; j++) {
            const int c = t + 256 * j;
            if (c >= NC) continue;
            f2 z;
            if constexpr (LAYOUT == DABGPU_TX_PAYLOAD_REFERENCE) {
                z = tx_phase_map(((uint32_t)sym[c >> 2] >> (2 * (c & 3))) & 3u);
            } else {
                const int n = nbit[j];
                z = tx_bits_map(((uint32_t)sym[n >> 3] >> (n & 7)) & 1u, ((uint32_t)sym[(n + NC) >> 3] >> ((n + NC) & 7)) & 1u);
            }
            X[j] = tx_mul(X[j], z);
        }
    };
    for (int s = 1; s < s0; s++) step(s);

    auto put = [&](f2 v, int m) {                                      // frame sample m
        v = tx_shift<PLL>(v, m, g.frame_samples, f);
        if constexpr (OUT == DABGPU_IQ_RAW_F32L) reinterpret_cast<f2*>(out)[o_frame + m] = v;
        else reinterpret_cast<uint16_t*>(out)[o_frame + m] = (uint16_t)tx_u8_pair(v, scale);
    };
    if (s0 == 0)
        for (int n = t; n < g.null_period; n += 256) put(mk2(0.0f, 0.0f), n);

    for (int s = s0; s < s1; s++) {
        if (s == 0) {
            for (int i = t; i < N; i += 256) x[i] = prs[i];
        } else {
            step(s);
            for (int i = t; i < N; i += 256)
                if (i == 0 || (i > M && i < N - M)) x[i] = mk2(0.0f, 0.0f);     // DC and the guard band
#pragma unroll
            for (int j = 0; j < TXG_CPT; j++)
                if (t + 256 * j < NC) x[bin[j]] = X[j];
        }
        __syncthreads();
        fft_lds(N, x, y, tmp, tw, w2048, true);                         // (ends behind a barrier; its first pass comes after one)
        const int m0 = g.null_period + s * g.period;
        for (int n = t; n < g.period; n += 256) put(y[n < g.n_cp ? n + N - g.n_cp : n - g.n_cp], m0 + n);
    }
}

}  // namespace dabgpu

using namespace dabgpu;

// runs per frame: enough workgroups for every CU to hold a few, fewer replays for large batches (DABGPU_TX_SPB = symbols per run)
static int tx_sym_per_run(dabgpu_ctx* c, size_t n_frames, int n_sym) {
    static const int forced = [] { const char* e = getenv("DABGPU_TX_SPB"); return e ? atoi(e) : 0; }();
    if (forced > 0) return forced < n_sym ? forced : n_sym;
    if (c->n_cu <= 0) {
        hipDeviceProp_t p;
        c->n_cu = (hipGetDeviceProperties(&p, c->device) == hipSuccess) ? p.multiProcessorCount : 256;
    }
    const size_t want = (size_t)8 * (size_t)c->n_cu;
    size_t runs = (want + n_frames - 1) / n_frames;
    if (runs > (size_t)n_sym) runs = (size_t)n_sym;
    return (int)(((size_t)n_sym + runs - 1) / runs);
}

int dabgpu_launch_ofdm_mod(dabgpu_ctx* c, int mode, const uint8_t* d_payload, int layout, size_t n_frames, const float* d_prs, float freq_norm,
                           void* d_out, int out_format, hipStream_t s, const dabgpu_tii_tx* d_tii, const uint8_t* d_tii_count) {
    ModeGeom g;
    if (!mode_geometry(mode, g)) { dabgpu_set_error("ofdm_modulate_frames: invalid transmission mode %d", mode); return DABGPU_ERR_INVALID_ARG; }
    const bool tii = d_tii && d_tii_count;
    if (tii && mode != 1) { dabgpu_set_error("ofdm_modulate_frames_tii: TII is defined for transmission mode I only (mode %d)", mode); return DABGPU_ERR_INVALID_ARG; }
    // (modes II-IV: their tables are built only by a call that reads them)
    const dabgpu_mode_tables* t = nullptr;
    int st = DABGPU_OK;
    if ((mode == 1 || !d_prs || layout == DABGPU_TX_PAYLOAD_FRAME_BITS) && (st = dabgpu_mode_tables_of(c, mode, &t, "ofdm_modulate_frames"))) return st;
    const int* d_inv = (t && layout == DABGPU_TX_PAYLOAD_FRAME_BITS) ? t->inv_map : nullptr;
    const int spb = tx_sym_per_run(c, n_frames, g.n_sym);
    const int runs = (g.n_sym + spb - 1) / spb;
    const size_t units = n_frames * (size_t)runs;
    if (units > 0x7FFFFFFFull) { dabgpu_set_error("ofdm_modulate_frames: n_frames too large"); return DABGPU_ERR_INVALID_ARG; }
    const float scale = (1.0f / (float)g.n_carriers * 4.0f) * 127.5f;          // simulate_transmitter.cpp:174 x QuantisedIQ<uint8_t>::MAX_AMPLITUDE
    const bool pll = freq_norm != 0.0f;
    const f2* prs = reinterpret_cast<const f2*>(d_prs ? d_prs : t->prs);
    const f2* tw = reinterpret_cast<const f2*>(c->d_tw);
#define TX_GO(OUT, LAYOUT, PLL)                                                                                                       \
    do {                                                                                                                              \
        if (mode == 1 && tii)                                                                                                         \
            hipLaunchKernelGGL((ofdm_mod_kernel<OUT, LAYOUT, PLL, true>), dim3((unsigned)units), dim3(256), 0, s, d_payload, prs, tw, \
                               t->inv_map16, (int)n_frames, spb, runs, freq_norm, scale, d_out, d_tii, d_tii_count);                  \
        else if (mode == 1)                                                                                                           \
            hipLaunchKernelGGL((ofdm_mod_kernel<OUT, LAYOUT, PLL, false>), dim3((unsigned)units), dim3(256), 0, s, d_payload, prs, tw, \
                               t->inv_map16, (int)n_frames, spb, runs, freq_norm, scale, d_out, (const dabgpu_tii_tx*)nullptr,        \
                               (const uint8_t*)nullptr);                                                                              \
        else                                                                                                                          \
            hipLaunchKernelGGL((ofdm_mod_mode_kernel<OUT, LAYOUT, PLL>), dim3((unsigned)units), dim3(256), 0, s, mode, d_payload, prs, \
                               tw, d_inv, (int)n_frames, spb, runs, freq_norm, scale, d_out);                                         \
    } while (0)
#define TX_PLL(OUT, LAYOUT) do { if (pll) TX_GO(OUT, LAYOUT, true); else TX_GO(OUT, LAYOUT, false); } while (0)
#define TX_LAYOUT(OUT)                                                                                                                \
    do { if (layout == DABGPU_TX_PAYLOAD_REFERENCE) TX_PLL(OUT, DABGPU_TX_PAYLOAD_REFERENCE); else TX_PLL(OUT, DABGPU_TX_PAYLOAD_FRAME_BITS); } while (0)
    if (out_format == DABGPU_IQ_RAW_F32L) TX_LAYOUT(DABGPU_IQ_RAW_F32L);
    else TX_LAYOUT(DABGPU_IQ_RAW_U8);
#undef TX_LAYOUT
#undef TX_PLL
#undef TX_GO
    return dabgpu_check_hip(hipGetLastError(), "ofdm_mod_kernel launch");
}

extern "C" {

// argument checks first, no device call before them (tests/test_tx_abi.py runs them without a device)
static int tx_check(dabgpu_ctx* c, int mode, const void* payload, int layout, size_t n_frames, void* out, int out_format, const char* who) {
    ModeGeom g;
    if (!c) { dabgpu_set_error("%s: null context", who); return DABGPU_ERR_INVALID_ARG; }
    if (!mode_geometry(mode, g)) { dabgpu_set_error("%s: invalid transmission mode %d", who, mode); return DABGPU_ERR_INVALID_ARG; }
    if (layout != DABGPU_TX_PAYLOAD_REFERENCE && layout != DABGPU_TX_PAYLOAD_FRAME_BITS) {
        dabgpu_set_error("%s: invalid payload layout %d", who, layout); return DABGPU_ERR_INVALID_ARG;
    }
    if (out_format != DABGPU_IQ_RAW_F32L && out_format != DABGPU_IQ_RAW_U8) {
        dabgpu_set_error("%s: output format %d (DABGPU_IQ_RAW_F32L or DABGPU_IQ_RAW_U8 only)", who, out_format); return DABGPU_ERR_INVALID_ARG;
    }
    if (n_frames > 0 && (!payload || !out)) { dabgpu_set_error("%s: null payload / output", who); return DABGPU_ERR_INVALID_ARG; }
    if (n_frames > (size_t)(1 << 22)) { dabgpu_set_error("%s: n_frames too large", who); return DABGPU_ERR_INVALID_ARG; }
    return DABGPU_OK;
}

// both device forms; d_tii / d_tii_count = nullptr: no TII
static int tx_modulate(dabgpu_ctx* c, int mode, const uint8_t* d_payload, int payload_layout, size_t n_frames, const float* d_prs_fft_ref, float freq_norm,
                       void* d_out, int out_format, void* stream, const dabgpu_tii_tx* d_tii, const uint8_t* d_tii_count, const char* who) {
    int st = tx_check(c, mode, d_payload, payload_layout, n_frames, d_out, out_format, who);
    if (st) return st;
    if (d_tii && d_tii_count && mode != 1) { dabgpu_set_error("%s: TII is defined for transmission mode I only (mode %d)", who, mode); return DABGPU_ERR_INVALID_ARG; }
    if (n_frames == 0) return st;
    if ((uintptr_t)d_out & 15) { dabgpu_set_error("%s: d_out must be 16-byte aligned", who); return DABGPU_ERR_INVALID_ARG; }
    if ((uintptr_t)d_prs_fft_ref & 7) { dabgpu_set_error("%s: d_prs_fft_ref must be 8-byte aligned", who); return DABGPU_ERR_INVALID_ARG; }
    if ((uintptr_t)d_tii & 3) { dabgpu_set_error("%s: d_tii must be 4-byte aligned", who); return DABGPU_ERR_INVALID_ARG; }
    DABGPU_BIND(c);
    return dabgpu_launch_ofdm_mod(c, mode, d_payload, payload_layout, n_frames, d_prs_fft_ref, freq_norm, d_out, out_format, (hipStream_t)stream, d_tii,
                                  d_tii_count);
}

int dabgpu_ofdm_modulate_frames(dabgpu_ctx* c, int mode, const uint8_t* d_payload, int payload_layout, size_t n_frames, const float* d_prs_fft_ref,
                                float freq_norm, void* d_out, int out_format, void* stream) {
    return tx_modulate(c, mode, d_payload, payload_layout, n_frames, d_prs_fft_ref, freq_norm, d_out, out_format, stream, nullptr, nullptr,
                       "ofdm_modulate_frames");
}

int dabgpu_ofdm_modulate_frames_tii(dabgpu_ctx* c, int mode, const uint8_t* d_payload, int payload_layout, size_t n_frames, const float* d_prs_fft_ref,
                                    float freq_norm, void* d_out, int out_format, void* stream, const dabgpu_tii_tx* d_tii, const uint8_t* d_tii_count) {
    return tx_modulate(c, mode, d_payload, payload_layout, n_frames, d_prs_fft_ref, freq_norm, d_out, out_format, stream, d_tii, d_tii_count,
                       "ofdm_modulate_frames_tii");
}

static int tx_modulate_host(dabgpu_ctx* c, int mode, const uint8_t* h_payload, int payload_layout, size_t n_frames, const float* h_prs_fft_ref,
                            float freq_norm, void* h_out, int out_format, const dabgpu_tii_tx* h_tii, const uint8_t* h_tii_count, const char* who) {
    int st = tx_check(c, mode, h_payload, payload_layout, n_frames, h_out, out_format, who);
    if (st) return st;
    const bool tii = h_tii && h_tii_count;
    if (tii && mode != 1) { dabgpu_set_error("%s: TII is defined for transmission mode I only (mode %d)", who, mode); return DABGPU_ERR_INVALID_ARG; }
    if (tii && (st = dabgpu_tii_validate(h_tii, h_tii_count, n_frames))) return st;
    if (n_frames == 0) return st;
    ModeGeom g;
    mode_geometry(mode, g);
    DABGPU_BIND(c);
    DABGPU_HOST_LOCK(c);
    const size_t in_bytes = n_frames * (size_t)(g.frame_bits / 8);
    const size_t out_bytes = n_frames * (size_t)g.frame_samples * (out_format == DABGPU_IQ_RAW_F32L ? 8 : 2);
    const size_t prs_bytes = (size_t)g.n_fft * 2 * sizeof(float);
    uint8_t *d_in, *d_out;
    float* d_prs = nullptr;
    // (the slots of the single-frame host forms, in the roles of a transmitter: a call of one of them never runs inside another)
    if ((st = dabgpu_scratch(c, SCR_HOST_BITS, in_bytes, (void**)&d_in))) return st;
    if ((st = dabgpu_scratch(c, SCR_HOST_IQ, out_bytes, (void**)&d_out))) return st;
    if (h_prs_fft_ref && (st = dabgpu_scratch(c, SCR_HOST_FFT, prs_bytes, (void**)&d_prs))) return st;
    dabgpu_tii_tx* d_tii = nullptr;
    uint8_t* d_cnt = nullptr;
    if (tii && (st = dabgpu_scratch(c, SCR_HOST_TII_LIST, n_frames * DABGPU_TII_MAX_TX * sizeof(dabgpu_tii_tx), (void**)&d_tii))) return st;
    if (tii && (st = dabgpu_scratch(c, SCR_HOST_TII_COUNT, n_frames, (void**)&d_cnt))) return st;
    hipStream_t s = c->stream;
    DABGPU_CK(hipMemcpyAsync(d_in, h_payload, in_bytes, hipMemcpyHostToDevice, s));
    if (h_prs_fft_ref) DABGPU_CK(hipMemcpyAsync(d_prs, h_prs_fft_ref, prs_bytes, hipMemcpyHostToDevice, s));
    if (tii) {
        DABGPU_CK(hipMemcpyAsync(d_tii, h_tii, n_frames * DABGPU_TII_MAX_TX * sizeof(dabgpu_tii_tx), hipMemcpyHostToDevice, s));
        DABGPU_CK(hipMemcpyAsync(d_cnt, h_tii_count, n_frames, hipMemcpyHostToDevice, s));
    }
    if ((st = tx_modulate(c, mode, d_in, payload_layout, n_frames, d_prs, freq_norm, d_out, out_format, s, d_tii, d_cnt, who))) return st;
    DABGPU_CK(hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, s));
    DABGPU_CK(hipStreamSynchronize(s));
    return DABGPU_OK;
}

int dabgpu_ofdm_modulate_frames_host_sync(dabgpu_ctx* c, int mode, const uint8_t* h_payload, int payload_layout, size_t n_frames,
                                          const float* h_prs_fft_ref, float freq_norm, void* h_out, int out_format) {
    return tx_modulate_host(c, mode, h_payload, payload_layout, n_frames, h_prs_fft_ref, freq_norm, h_out, out_format, nullptr, nullptr,
                            "ofdm_modulate_frames_host_sync");
}

int dabgpu_ofdm_modulate_frames_tii_host_sync(dabgpu_ctx* c, int mode, const uint8_t* h_payload, int payload_layout, size_t n_frames,
                                              const float* h_prs_fft_ref, float freq_norm, void* h_out, int out_format, const dabgpu_tii_tx* h_tii,
                                              const uint8_t* h_tii_count) {
    return tx_modulate_host(c, mode, h_payload, payload_layout, n_frames, h_prs_fft_ref, freq_norm, h_out, out_format, h_tii, h_tii_count,
                            "ofdm_modulate_frames_tii_host_sync");
}

}  // extern "C"
