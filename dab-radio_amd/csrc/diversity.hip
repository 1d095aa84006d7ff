// diversity.hip -- receive diversity (include/dabgpu.h, "Receive diversity"): the DQPSK products of up to 8 branches of one ensemble, as
// the demodulator's display view holds them ([75][1536] complex float per frame, carrier order), summed carrier by carrier, scaled by
// the combined factor of the frame and quantised into the decoder's soft bits.  Arithmetic: diversity_core.h (every step; this file adds
// none).  A stage of its own behind the demodulator: the demodulation kernel is untouched.
//
// One workgroup of 256 lanes per (frame, run of symbols).  The branch table travels by value as a kernel argument -- no host-to-device
// copy, so a call is one launch and can be captured.  The workgroup forms the live mask and k once (wave-uniform: the table entries are
// scalar loads, the arithmetic is the same in every lane).  Per symbol a lane reads, for every live branch, three 16-byte pieces of the
// branch's row = two carriers each, lane after lane (coalesced, 12288 bytes per branch and symbol), accumulates the six carriers in
// registers, scales and quantises, and scatters the twelve soft bits to their de-interleaved positions in an LDS row (inv_map16; in
// class order the second position set, bit p of the symbol at (p mod 16) * 192 + p / 16).  192 lanes then store the 3072-byte row with
// 16-byte stores.  Two LDS rows alternate, so a symbol costs one barrier.  HBM-bound: K * 921,600 bytes in, 230,400 out per frame.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>

#include "dabgpu_internal.h"
#include "diversity_core.h"
#include "noise_profile_core.h"
#include "ofdm_device.h"

namespace dabgpu {

typedef float dv_f4 __attribute__((ext_vector_type(4)));
struct dv_table { dabgpu_diversity_branch b[DV_MAX_BRANCHES]; };
// the banded call's argument: the branch table and, per branch, its band weights [n_frames][128] (null: the branch has a scalar weight)
struct dv_table_banded { dabgpu_diversity_branch b[DV_MAX_BRANCHES]; const float* band[DV_MAX_BRANCHES]; };
// the symbol-weighted call's: per branch also its symbol weights [n_frames][75] (null: none)
struct dv_table_symbols { dabgpu_diversity_branch b[DV_MAX_BRANCHES]; const float* band[DV_MAX_BRANCHES]; const float* sym[DV_MAX_BRANCHES]; };
enum dv_mode { DV_SCALAR = 0, DV_BANDED = 1, DV_SYMBOLS = 2 };
template <int MODE> struct dv_table_of { typedef dv_table type; };
template <> struct dv_table_of<DV_BANDED> { typedef dv_table_banded type; };
template <> struct dv_table_of<DV_SYMBOLS> { typedef dv_table_symbols type; };

constexpr int DV_DATA_SYMBOLS = 75, DV_CARRIERS = 1536, DV_SYM_BITS = 3072, DV_FIC_SYMBOLS = 3, DV_CIF_SYMBOLS = 18, DV_CIF_BITS = 55296;
constexpr int DV_ROW_PIECES = DV_CARRIERS / 2;              // 16-byte pieces of a branch's symbol row: 768 = 3 per lane
static_assert(DV_ROW_PIECES == 3 * (int)DABGPU_DIVERSITY_THREADS && DV_SYM_BITS / 16 <= (int)DABGPU_DIVERSITY_THREADS, "three pieces per lane, 192 storing lanes");

// BANDED (include/dabgpu.h, "Banded receive diversity"): a branch with a band table takes the tree mean of the frame's 128 band weights
// for its weight -- lanes 0 .. 127 hold one band each, the two wave sums meet in LDS -- and every lane keeps the band weights of its three
// pieces (carriers 2 (t + 256 j), + 1: band (t + 256 j) / 6) in registers for all symbols of the run.  The first instantiation is the
// kernel as it was.  DV_SYMBOLS (include/dabgpu.h, "Symbol-weighted receive diversity") is the banded instantiation with one more factor:
// a branch with a symbol table multiplies the piece's weight by the clean weight of the row, one uniform load per branch and row, the
// product rounded once.  Symbol weights enter neither the live rule nor the scale.
template <int MODE>
__global__ __launch_bounds__(DABGPU_DIVERSITY_THREADS)
void diversity_combine_kernel(const typename dv_table_of<MODE>::type tab, const int n_branches, const int n_frames, const int sym_per_run, const int runs_per_frame,
                              int8_t* __restrict__ bits, const size_t bits_frame_stride, const int classed, const uint16_t* __restrict__ inv_map,
                              float* __restrict__ soft_scale, uint32_t* __restrict__ live_mask)
{
    __shared__ __attribute__((aligned(16))) int8_t obuf[2][DV_SYM_BITS];
    const int t = threadIdx.x;
    const int frame = blockIdx.x / runs_per_frame, run = blockIdx.x % runs_per_frame;
    if (frame >= n_frames) return;
    constexpr bool BANDED = MODE != DV_SCALAR;
    const int row0 = run * sym_per_run, row1 = min(row0 + sym_per_run, DV_DATA_SYMBOLS);

    // ---- the frame's live branches and its scale (uniform) ----
    float w[DV_MAX_BRANCHES];
    float wl[BANDED ? DV_MAX_BRANCHES : 1][3], wmean[BANDED ? DV_MAX_BRANCHES : 1];
    if constexpr (BANDED) {
        __shared__ float meanS[DV_MAX_BRANCHES][2];
#pragma unroll
        for (int b = 0; b < DV_MAX_BRANCHES; b++) {
            if (b < n_branches && tab.band[b] != nullptr) {                           // (uniform)
                const float* const bw = tab.band[b] + (size_t)frame * NP_BANDS;
                if (t < NP_BANDS) {
                    const float s = wave_tree_sum(np_clean_weight(bw[t]), t & 63);
                    if ((t & 63) == 0) meanS[b][t >> 6] = s;
                }
#pragma unroll
                for (int j = 0; j < 3; j++) wl[b][j] = np_clean_weight(bw[(t + 256 * j) / 6]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < DV_MAX_BRANCHES; b++) wmean[b] = (b < n_branches && tab.band[b] != nullptr) ? np_mean_join(meanS[b][0], meanS[b][1]) : 1.0f;
    }
    dv_scale_state st = dv_scale_begin();
#pragma unroll
    for (int b = 0; b < DV_MAX_BRANCHES; b++) {
        w[b] = 1.0f;
        if (b < n_branches) {
            const dabgpu_diversity_branch B = tab.b[b];
            const bool sync_ok = B.d_sync == nullptr || B.d_sync[frame].sync_valid != 0;
            if (B.d_weight != nullptr) w[b] = B.d_weight[frame];
            if constexpr (BANDED) {
                if (tab.band[b] != nullptr) w[b] = wmean[b];
                else { wl[b][0] = w[b]; wl[b][1] = w[b]; wl[b][2] = w[b]; }
            }
            dv_scale_add(st, b, sync_ok, B.d_scale[frame], w[b]);
        }
    }
    const float k = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(dv_scale_end(st))));
    const uint32_t mask = __builtin_amdgcn_readfirstlane(st.mask);
    if (run == 0 && t == 0) {
        if (soft_scale != nullptr) soft_scale[frame] = k;
        if (live_mask != nullptr) live_mask[frame] = mask;
    }
    // an erased frame is all zeros whatever its products hold (c * 0 is 0 or NaN, and NaN quantises to 0): nothing is read
    const uint32_t read_mask = (k == 0.0f) ? 0u : mask;

    // ---- de-interleave positions of this lane's six carriers: pieces t, t + 256, t + 512 = carriers 2 (t + 256 j), + 1 ----
    int pos[6], posc[6];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        pos[2 * j] = inv_map[2 * (t + 256 * j)];
        pos[2 * j + 1] = inv_map[2 * (t + 256 * j) + 1];
    }
#pragma unroll
    for (int i = 0; i < 6; i++) posc[i] = (pos[i] & 15) * 192 + (pos[i] >> 4);        // class order; the second bit sits 96 further

    int8_t* const out_frame = bits + (size_t)frame * bits_frame_stride;
    for (int row = row0; row < row1; row++) {
        dv_f4 acc[3] = {dv_f4{0.0f, 0.0f, 0.0f, 0.0f}, dv_f4{0.0f, 0.0f, 0.0f, 0.0f}, dv_f4{0.0f, 0.0f, 0.0f, 0.0f}};
        bool first = true;
#pragma unroll
        for (int b = 0; b < DV_MAX_BRANCHES; b++) {
            if ((read_mask >> b) & 1u) {                                              // (uniform)
                const dv_f4* const p = reinterpret_cast<const dv_f4*>(tab.b[b].d_dqpsk) + ((size_t)frame * DV_DATA_SYMBOLS + (size_t)row) * DV_ROW_PIECES + t;
                const dv_f4 v0 = p[0], v1 = p[256], v2 = p[512];
                const dv_f4 v[3] = {v0, v1, v2};
                // the weight of piece j: the branch's, or (BANDED) the one of the piece's band
                float ws = 1.0f;
                if constexpr (MODE == DV_SYMBOLS) {
                    if (tab.sym[b] != nullptr) ws = np_clean_weight(tab.sym[b][(size_t)frame * DV_DATA_SYMBOLS + (size_t)row]);   // (uniform)
                }
                auto wj = [&](int j) __attribute__((always_inline)) {
                    if constexpr (MODE == DV_SYMBOLS) return wl[b][j] * ws;
                    else if constexpr (BANDED) return wl[b][j];
                    else return w[b];
                };
                if (first) {
#pragma unroll
                    for (int j = 0; j < 3; j++)
                        acc[j] = dv_f4{dv_sum_first(wj(j), v[j].x), dv_sum_first(wj(j), v[j].y), dv_sum_first(wj(j), v[j].z), dv_sum_first(wj(j), v[j].w)};
                    first = false;
                } else {
#pragma unroll
                    for (int j = 0; j < 3; j++)
                        acc[j] = dv_f4{dv_sum_next(acc[j].x, wj(j), v[j].x), dv_sum_next(acc[j].y, wj(j), v[j].y), dv_sum_next(acc[j].z, wj(j), v[j].z),
                                       dv_sum_next(acc[j].w, wj(j), v[j].w)};
                }
            }
        }
        // soft bits of the six carriers into this symbol's LDS row
        int8_t* const ob = obuf[(row - row0) & 1];
        const bool class_row = classed && row >= DV_FIC_SYMBOLS;                      // (uniform)
        const int second = class_row ? 96 : DV_CARRIERS;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int p0 = class_row ? posc[2 * j] : pos[2 * j], p1 = class_row ? posc[2 * j + 1] : pos[2 * j + 1];
            ob[p0] = (int8_t)sb_soft_bit(acc[j].x, k);
            ob[p0 + second] = (int8_t)sb_soft_bit(-acc[j].y, k);
            ob[p1] = (int8_t)sb_soft_bit(acc[j].z, k);
            ob[p1 + second] = (int8_t)sb_soft_bit(-acc[j].w, k);
        }
        // the row is complete behind this barrier; the other LDS row takes the next symbol, and the barrier of that symbol orders this
        // row's reads below before the scatter of the symbol after it
        __syncthreads();
        if (t < DV_SYM_BITS / 16) {
            const uint4 o = reinterpret_cast<const uint4*>(ob)[t];
            size_t off;
            if (class_row) {                                                          // class t / 12, bytes 16 (t mod 12) .. + 15 of this symbol's 192
                const int q = (row - DV_FIC_SYMBOLS) / DV_CIF_SYMBOLS, sy = (row - DV_FIC_SYMBOLS) % DV_CIF_SYMBOLS;
                off = (size_t)(DV_FIC_SYMBOLS * DV_SYM_BITS + q * DV_CIF_BITS + (t / 12) * (DV_CIF_BITS / 16) + sy * (DV_SYM_BITS / 16) + 16 * (t % 12));
            } else {
                off = (size_t)(row * DV_SYM_BITS + 16 * t);
            }
            *reinterpret_cast<uint4*>(out_frame + off) = o;
        }
    }
}

}  // namespace dabgpu

using namespace dabgpu;

namespace {

constexpr int K = DABGPU_DIVERSITY_MAX_BRANCHES;
// by dv_mode: the device entry point, its launch label, the host form
const char* const DV_CALL[3] = {"diversity_combine_frames", "diversity_combine_frames_banded", "diversity_combine_frames_symbols"};
const char* const DV_LABEL[3] = {"diversity_combine_kernel launch", "diversity_combine_kernel (banded) launch", "diversity_combine_kernel (symbols) launch"};
const char* const DV_FORM[3] = {"diversity_combine_host_sync", "diversity_combine_banded_host_sync", "diversity_combine_symbols_host_sync"};

const float* dv_entry(const float* const* table, int b) { return table ? table[b] : nullptr; }

// The three device entry points: `who` is the one that was called and names itself in the null-context refusal only.  Everything behind
// the plan goes by the call's EFFECTIVE mode -- symbols where a symbol entry is given, else banded where a band entry is, else scalar
// (dabgpu_host_plan_diversity_mode): a call without a table of its kind is the narrower call, messages, label and instantiation included.
int dv_combine_frames(const char* who, dabgpu_ctx* c, const dabgpu_diversity_branch* h_branches, int n_branches, size_t n_frames, int8_t* d_bits,
                      size_t bits_frame_stride, int bits_layout, int symbols_per_block, float* d_soft_scale, uint32_t* d_live_mask,
                      const float* const* h_band_weight, const float* const* h_symbol_weight, void* stream) {
    if (!c) { dabgpu_set_error("%s: null context", who); return DABGPU_ERR_INVALID_ARG; }
    dabgpu_diversity_geometry g;
    int mode;
    int st = dabgpu_host_plan_diversity_mode(h_branches, n_branches, n_frames, d_bits, bits_frame_stride, bits_layout, symbols_per_block, h_band_weight,
                                             h_symbol_weight, &g, &mode);
    if (st) return st;
    if ((((uintptr_t)d_soft_scale | (uintptr_t)d_live_mask) & 3)) {
        dabgpu_set_error("%s: d_soft_scale and d_live_mask must be 4-byte aligned", DV_CALL[mode]); return DABGPU_ERR_INVALID_ARG;
    }
    if (n_frames == 0) return DABGPU_OK;
    DABGPU_BIND(c);
    const dabgpu_mode_tables* t;
    if ((st = dabgpu_mode_tables_of(c, 1, &t, DV_CALL[mode]))) return st;
    const auto launch = [&](auto m) {
        constexpr int MODE = decltype(m)::value;
        typename dv_table_of<MODE>::type tab;
        memset(&tab, 0, sizeof(tab));
        for (int b = 0; b < n_branches; b++) {
            tab.b[b] = h_branches[b];
            if constexpr (MODE != DV_SCALAR) tab.band[b] = dv_entry(h_band_weight, b);
            if constexpr (MODE == DV_SYMBOLS) tab.sym[b] = dv_entry(h_symbol_weight, b);
        }
        hipLaunchKernelGGL(diversity_combine_kernel<MODE>, dim3(g.grid), dim3(g.threads), 0, (hipStream_t)stream, tab, n_branches, (int)n_frames,
                           (int)g.symbols_per_block, (int)g.runs_per_frame, d_bits, bits_frame_stride ? bits_frame_stride : (size_t)DABGPU_NB_FRAME_BITS,
                           bits_layout == DABGPU_BITS_MSC_CLASSED ? 1 : 0, t->inv_map16, d_soft_scale, d_live_mask);
    };
    if (mode == DV_SCALAR) launch(std::integral_constant<int, DV_SCALAR>{});
    else if (mode == DV_BANDED) launch(std::integral_constant<int, DV_BANDED>{});
    else launch(std::integral_constant<int, DV_SYMBOLS>{});
    return dabgpu_check_hip(hipGetLastError(), DV_LABEL[mode]);
}

// The three host forms.  The form, and with it the name in its own refusals and the device call it makes, follows the ARRAYS given: without
// h_symbol_weight it is the banded form, without h_band_weight either the scalar one (an array of null entries keeps its form).  The block of
// small words: K scales, K weights, k and the mask, K band tables, K symbol tables.
int dv_combine_host(dabgpu_ctx* c, const float* const* h_dqpsk, const float* h_scale, const float* h_weight, const int* h_valid, int n_branches,
                    int bits_layout, int8_t* h_bits, float* h_soft_scale, uint32_t* h_live_mask, const float* const* h_band_weight,
                    const float* const* h_symbol_weight) {
    const int form = h_symbol_weight ? DV_SYMBOLS : h_band_weight ? DV_BANDED : DV_SCALAR;
    const char* const who = DV_FORM[form];
    if (!c || !h_dqpsk || !h_scale || !h_bits) { dabgpu_set_error("%s: null argument", who); return DABGPU_ERR_INVALID_ARG; }
    if (n_branches < 1 || n_branches > K) { dabgpu_set_error("%s: n_branches %d outside 1 .. %d", who, n_branches, K); return DABGPU_ERR_INVALID_ARG; }
    int st = dabgpu_check_bits_layout(who, bits_layout);
    if (st) return st;
    // what the kernel will find live decides which products are uploaded: a branch the synchroniser refused travels as scale 0 (symbol
    // weights have no say in that)
    float small[2 * K] = {};
    for (int b = 0; b < n_branches; b++) {
        const float* const hb = dv_entry(h_band_weight, b);
        const float w = hb ? np_branch_weight(hb) : (h_weight ? h_weight[b] : 1.0f);
        const bool live = dv_branch_live(!h_valid || h_valid[b] != 0, h_scale[b], w);
        if (live && !h_dqpsk[b]) { dabgpu_set_error("%s: live branch %d has no products", who, b); return DABGPU_ERR_INVALID_ARG; }
        small[b] = live ? h_scale[b] : 0.0f;
        small[K + b] = w;
    }
    DABGPU_BIND(c);
    DABGPU_HOST_LOCK(c);
    const size_t dq_floats = (size_t)DV_DATA_SYMBOLS * DV_CARRIERS * 2, dq_bytes = dq_floats * sizeof(float);
    float *d_dq, *d_small; int8_t* d_bits;
    if ((st = dabgpu_scratch(c, SCR_HOST_DQPSK, dq_bytes * (size_t)n_branches, (void**)&d_dq))) return st;
    if ((st = dabgpu_scratch(c, SCR_HOST_BITS, (size_t)DABGPU_NB_FRAME_BITS, (void**)&d_bits))) return st;
    if ((st = dabgpu_scratch(c, SCR_HOST_FREQ, (2 * K + 2 + K * NP_BANDS + K * DV_DATA_SYMBOLS) * sizeof(float), (void**)&d_small))) return st;
    hipStream_t s = c->stream;
    float* const d_k = d_small + 2 * K;
    uint32_t* const d_mask = reinterpret_cast<uint32_t*>(d_k + 1);
    float* const d_band = d_k + 2;
    float* const d_sym = d_band + (size_t)K * NP_BANDS;
    dabgpu_diversity_branch br[K];
    const float *band[K], *sym[K];
    for (int b = 0; b < n_branches; b++) {
        const float *const hb = dv_entry(h_band_weight, b), *const hs = dv_entry(h_symbol_weight, b);
        br[b].d_dqpsk = d_dq + (size_t)b * dq_floats;
        br[b].d_scale = d_small + b;
        br[b].d_weight = hb ? nullptr : d_small + K + b;
        br[b].d_sync = nullptr;
        band[b] = hb ? d_band + (size_t)b * NP_BANDS : nullptr;
        sym[b] = hs ? d_sym + (size_t)b * DV_DATA_SYMBOLS : nullptr;
        if (hb) DABGPU_CK(hipMemcpyAsync(const_cast<float*>(band[b]), hb, NP_BANDS * sizeof(float), hipMemcpyHostToDevice, s));
        if (hs) DABGPU_CK(hipMemcpyAsync(const_cast<float*>(sym[b]), hs, DV_DATA_SYMBOLS * sizeof(float), hipMemcpyHostToDevice, s));
        if (small[b] != 0.0f) DABGPU_CK(hipMemcpyAsync(const_cast<float*>(br[b].d_dqpsk), h_dqpsk[b], dq_bytes, hipMemcpyHostToDevice, s));
    }
    if ((st = dabgpu_stage_h2d(c, d_small, small, sizeof(small), s))) return st;
    if ((st = dv_combine_frames(DV_CALL[form], c, br, n_branches, 1, d_bits, 0, bits_layout, 0, d_k, d_mask, band, sym, s))) return st;
    uint32_t back[2];
    DABGPU_CK(hipMemcpyAsync(h_bits, d_bits, (size_t)DABGPU_NB_FRAME_BITS, hipMemcpyDeviceToHost, s));
    DABGPU_CK(hipMemcpyAsync(back, d_k, sizeof(back), hipMemcpyDeviceToHost, s));
    DABGPU_CK(hipStreamSynchronize(s));
    if (h_soft_scale) memcpy(h_soft_scale, &back[0], sizeof(float));
    if (h_live_mask) *h_live_mask = back[1];
    return DABGPU_OK;
}

}  // namespace

int dabgpu_diversity_combine_frames(dabgpu_ctx* c, const dabgpu_diversity_branch* h_branches, int n_branches, size_t n_frames, int8_t* d_bits,
                                    size_t bits_frame_stride, int bits_layout, int symbols_per_block, float* d_soft_scale, uint32_t* d_live_mask,
                                    void* stream) {
    return dv_combine_frames(DV_CALL[DV_SCALAR], c, h_branches, n_branches, n_frames, d_bits, bits_frame_stride, bits_layout, symbols_per_block, d_soft_scale,
                             d_live_mask, nullptr, nullptr, stream);
}

int dabgpu_diversity_combine_frames_banded(dabgpu_ctx* c, const dabgpu_diversity_branch* h_branches, int n_branches, size_t n_frames, int8_t* d_bits,
                                           size_t bits_frame_stride, int bits_layout, int symbols_per_block, float* d_soft_scale,
                                           uint32_t* d_live_mask, const float* const* h_band_weight, void* stream) {
    return dv_combine_frames(DV_CALL[DV_BANDED], c, h_branches, n_branches, n_frames, d_bits, bits_frame_stride, bits_layout, symbols_per_block, d_soft_scale,
                             d_live_mask, h_band_weight, nullptr, stream);
}

int dabgpu_diversity_combine_frames_symbols(dabgpu_ctx* c, const dabgpu_diversity_branch* h_branches, int n_branches, size_t n_frames, int8_t* d_bits,
                                            size_t bits_frame_stride, int bits_layout, int symbols_per_block, float* d_soft_scale,
                                            uint32_t* d_live_mask, const float* const* h_band_weight, const float* const* h_symbol_weight,
                                            void* stream) {
    return dv_combine_frames(DV_CALL[DV_SYMBOLS], c, h_branches, n_branches, n_frames, d_bits, bits_frame_stride, bits_layout, symbols_per_block, d_soft_scale,
                             d_live_mask, h_band_weight, h_symbol_weight, stream);
}

int dabgpu_diversity_combine_host_sync(dabgpu_ctx* c, const float* const* h_dqpsk, const float* h_scale, const float* h_weight, const int* h_valid,
                                       int n_branches, int bits_layout, int8_t* h_bits, float* h_soft_scale, uint32_t* h_live_mask) {
    return dv_combine_host(c, h_dqpsk, h_scale, h_weight, h_valid, n_branches, bits_layout, h_bits, h_soft_scale, h_live_mask, nullptr, nullptr);
}

int dabgpu_diversity_combine_banded_host_sync(dabgpu_ctx* c, const float* const* h_dqpsk, const float* h_scale, const float* h_weight,
                                              const int* h_valid, int n_branches, int bits_layout, int8_t* h_bits, float* h_soft_scale,
                                              uint32_t* h_live_mask, const float* const* h_band_weight) {
    return dv_combine_host(c, h_dqpsk, h_scale, h_weight, h_valid, n_branches, bits_layout, h_bits, h_soft_scale, h_live_mask, h_band_weight, nullptr);
}

int dabgpu_diversity_combine_symbols_host_sync(dabgpu_ctx* c, const float* const* h_dqpsk, const float* h_scale, const float* h_weight,
                                               const int* h_valid, int n_branches, int bits_layout, int8_t* h_bits, float* h_soft_scale,
                                               uint32_t* h_live_mask, const float* const* h_band_weight, const float* const* h_symbol_weight) {
    return dv_combine_host(c, h_dqpsk, h_scale, h_weight, h_valid, n_branches, bits_layout, h_bits, h_soft_scale, h_live_mask, h_band_weight, h_symbol_weight);
}
