// null_window.h -- the front half that the TII detector (tii.hip), the noise estimator (noise.hip) and the noise profile
// (noise_profile.hip) share on the device: where a window is and how it is rotated (null_window_place), and steps 1 to 4 of
// include/dabgpu.h, "TII" (null_window_powers).  One 256-thread workgroup per window.  Thread t reads the window samples 2 t + 512 j, 2 t + 1 + 512 j
// (j < 4: the eight inputs of its first butterflies) as four 16-byte loads (8-byte loads when the window starts on an odd sample), rotates
// them in registers and puts them into LDS with 16-byte stores; fft2048_lds in place; 2048 powers into LDS, complete behind the barrier
// this function ends with.
#pragma once
#include "ofdm_device.h"
#include "ofdm_fft_lds.h"
#include "tii_core.h"

namespace dabgpu {

// Where window k begins and how it is rotated (the same for the whole workgroup).  In: *f and *fto hold the call's own (no records); out:
// the record's fine time offset and net frequency offset, and over either a caller's offset (NaN: none for this window).  False: the
// record refuses the window -- no sync, an offset outside the range, with front also a NULL that would begin in front of the stream's
// slice (the TII bank does not ask that) -- and none of its samples may be read
__device__ __forceinline__ bool null_window_place(const dabgpu_sync_state* __restrict__ states, const float* __restrict__ freq, size_t k,
                                                  long long null_offset, bool front, float* f, int* fto) {
    if (states) {
        const dabgpu_sync_state st = states[k];
        if (!st.sync_valid || !tii_time_offset_ok(st.fine_time_offset) || (front && null_offset + st.fine_time_offset < 0)) return false;
        *fto = st.fine_time_offset;
        *f = st.freq_coarse + st.freq_fine;
    }
    if (freq) { const float fc = freq[k]; if (fc == fc) *f = fc; }
    return true;
}

// A: 4 x WAVE_PATCH elements, 16-byte aligned; Pw: TII_FFT floats; f: cycles per sample, phase 0 at the window's first sample
__device__ __forceinline__ void null_window_powers(const f2* __restrict__ win, float f, const Fft2048Tw& w, f2* A, float* Pw, int t) {
    const bool wide = ((uintptr_t)win & 15) == 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int n = 2 * t + 512 * j;
        f2 a, b;
        if (wide) { const f4 v = *reinterpret_cast<const f4*>(win + n); a = mk2(v.x, v.y); b = mk2(v.z, v.w); }
        else { a = win[n]; b = win[n + 1]; }
        a = pll_any(a, n, TII_FFT, f, 0.0f);
        b = pll_any(b, n + 1, TII_FFT, f, 0.0f);
        *reinterpret_cast<f4*>(A + n) = f4{a.x, a.y, b.x, b.y};
    }
    __syncthreads();
    fft2048_lds(A, w, false);
#pragma unroll
    for (int r = 0; r < 8; r++) { const f2 x = A[t + 256 * r]; Pw[t + 256 * r] = tii_power(x.x, x.y); }
    __syncthreads();
}

}  // namespace dabgpu
