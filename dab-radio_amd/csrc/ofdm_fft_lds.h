// ofdm_fft_lds.h -- the workgroup-wide transforms through LDS shared by the kernels that run whole transforms in one 256-thread
// workgroup: PRS synchronisation (ofdm_sync.hip) and the transmitter (ofdm_mod.hip).  Same butterflies and twiddle rule as the symbol
// kernel (ofdm_device.h); the inverse is conj(FFT(conj(x))), bit for bit the oracle's dab_ifft2048 / dab_fft_n(inverse = 1).
#pragma once
#include <hip/hip_runtime.h>

#include "ofdm_device.h"

namespace dabgpu {

// ---- 2048-point transform between natural-order LDS arrays (x -> y), same pass structure as ofdm_demod_kernel ----
// conj_io: inverse transform as conj(FFT(conj(x))), unnormalised like FFTW_BACKWARD
// x, bufA and y may all be ONE array (in place): a thread writes bufA at exactly the eight positions it has read x at, and the results
// are written behind a barrier
// the 20 twiddles a thread needs in a 2048-point transform depend on its index only: a kernel that runs several transforms loads them once
struct Fft2048Tw { f2 p1[6], p2[7], p3[7]; };
__device__ __forceinline__ Fft2048Tw fft2048_twiddles(const f2* __restrict__ tw) {
    const int t = threadIdx.x, lane = t & 63, la = lane & 7;
    Fft2048Tw w;
#pragma unroll
    for (int k = 1; k <= 3; k++) { w.p1[k - 1] = tw[(2 * t) * k]; w.p1[2 + k] = tw[(2 * t + 1) * k]; }
#pragma unroll
    for (int k = 1; k < 8; k++) { w.p2[k - 1] = tw[4 * lane * k]; w.p3[k - 1] = tw[32 * la * k]; }
    return w;
}

// x, y and the exchange array are ONE array of 4 x WAVE_PATCH elements (in place): input and output in natural order in its first 2048
// elements; between them the radix-4 outputs sit as four 512-element blocks WAVE_PATCH apart, one per wave's 512-point problem, and a
// wave's transpose patch aliases its own block (the wave has read its 8 inputs per lane before it writes the patch; one wave's LDS
// instructions execute in order) -- the layout of the symbol kernel (ofdm_demod.hip).  Barriers: inputs read / blocks written / results written.
__device__ __forceinline__ void fft2048_lds(f2* A, const Fft2048Tw& w, bool conj_io) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int la = lane & 7, lb = lane >> 3;
    f2* patch = A + wave * WAVE_PATCH;
    f2 a[8];
#pragma unroll
    for (int j = 0; j < 4; j++) { a[j] = A[2 * t + 512 * j]; a[4 + j] = A[2 * t + 1 + 512 * j]; }
    if (conj_io) {
#pragma unroll
        for (int j = 0; j < 8; j++) a[j].y = -a[j].y;
    }
    __syncthreads();                                       // (the blocks below do not sit where the inputs did)
    {
        f2 b0, b1, b2, b3, c0, c1, c2, c3;
        dft4(a[0], a[1], a[2], a[3], b0, b1, b2, b3);
        dft4(a[4], a[5], a[6], a[7], c0, c1, c2, c3);
        b1 = cmul(b1, w.p1[0]); b2 = cmul(b2, w.p1[1]); b3 = cmul(b3, w.p1[2]);
        c1 = cmul(c1, w.p1[3]); c2 = cmul(c2, w.p1[4]); c3 = cmul(c3, w.p1[5]);
        A[2 * t] = b0;                       A[2 * t + 1] = c0;
        A[2 * t + WAVE_PATCH] = b1;          A[2 * t + 1 + WAVE_PATCH] = c1;
        A[2 * t + 2 * WAVE_PATCH] = b2;      A[2 * t + 1 + 2 * WAVE_PATCH] = c2;
        A[2 * t + 3 * WAVE_PATCH] = b3;      A[2 * t + 1 + 3 * WAVE_PATCH] = c3;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; j++) a[j] = patch[lane + 64 * j];
    dft8(a);
    patch[lane] = a[0];
#pragma unroll
    for (int k = 1; k < 8; k++) patch[lane + 72 * k] = cmul(a[k], w.p2[k - 1]);
    wave_lds_fence();
#pragma unroll
    for (int j = 0; j < 8; j++) a[j] = patch[la + 72 * lb + 8 * j];
    wave_lds_fence();
    dft8(a);
    patch[la + 72 * lb] = a[0];
#pragma unroll
    for (int k = 1; k < 8; k++) patch[la + 72 * lb + 9 * k] = cmul(a[k], w.p3[k - 1]);
    wave_lds_fence();
#pragma unroll
    for (int j = 0; j < 8; j++) a[j] = patch[9 * la + 72 * lb + j];
    wave_lds_fence();
    dft8(a);
    const int Kb = wave + 4 * lb + 32 * la;
    __syncthreads();                                       // every wave has taken its block out of the array before anybody writes a result
#pragma unroll
    for (int k = 0; k < 8; k++) {
        f2 v = a[k];
        if (conj_io) v.y = -v.y;
        A[Kb + 256 * k] = v;
    }
    __syncthreads();
}

// transform of any supported length between natural-order LDS arrays: the register-resident 2048-point version above, or
// Stockham passes r1 x 8 x 8 [x 8] alternating between `tmp` and `y` so that the last pass lands in `y`
__device__ __forceinline__ void fft_lds(int N, f2* x, f2* y, f2* tmp, const f2* __restrict__ tw, const Fft2048Tw& w2048, bool conj_io) {
    if (N == NB_FFT) { fft2048_lds(x, w2048, conj_io); return; }      // (x == y == tmp: in place)
    const int t = threadIdx.x;
    if (conj_io) { for (int i = t; i < N; i += 256) x[i].y = -x[i].y; __syncthreads(); }
    const int r1 = (N == 256) ? 4 : (N == 1024 ? 2 : 8);
    const int n_pass = (N == 1024) ? 4 : 3;
    const f2* src = x;
    int cur_n = N, s = 1;
    for (int ps = 0; ps < n_pass; ps++) {
        const int r = (ps == 0) ? r1 : 8;
        const bool last = (ps == n_pass - 1);
        f2* dst = (((n_pass - 1 - ps) & 1) == 0) ? y : tmp;
        if (r == 8) stockham_pass<8>(src, dst, N, cur_n, s, last, tw, t, 256);
        else if (r == 4) stockham_pass<4>(src, dst, N, cur_n, s, last, tw, t, 256);
        else stockham_pass<2>(src, dst, N, cur_n, s, last, tw, t, 256);
        __syncthreads();
        src = dst; cur_n /= r; s *= r;
    }
    if (conj_io) { for (int i = t; i < N; i += 256) y[i].y = -y[i].y; __syncthreads(); }
}

}  // namespace dabgpu
