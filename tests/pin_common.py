"""What the float64 pins of the transmitter (tests/test_independent_pins.py) and of the demodulator (tests/demod_model.py) share: the
frequency interleaver of ETSI EN 300 401 clause 14.6, the carrier order of clause 14.5, and the two error bounds both stages use (the
float32 transform, the float32 PLL).  Nothing here shares code with the oracle or the kernels."""
import numpy as np

U32 = 2.0 ** -24                                # unit roundoff of binary32


def tx64_interleaver(N, NC):
    """clause 14.6: PI(0) = 0, PI(i) = (13 PI(i-1) + N/4 - 1) mod N; D = the values in [N/2 - NC/2, N/2 + NC/2] without N/2, in order of
    appearance; QPSK symbol n of an OFDM symbol goes onto carrier k = D[n] - N/2  (k in -NC/2 .. NC/2, k != 0)"""
    pi, ks = 0, []
    for _ in range(N):
        if N // 2 - NC // 2 <= pi <= N // 2 + NC // 2 and pi != N // 2:
            ks.append(pi - N // 2)
        pi = (13 * pi + N // 4 - 1) % N
    ks = np.array(ks, dtype=np.int64)
    assert ks.size == NC and np.unique(ks).size == NC
    return ks


def tx64_carriers(NC):
    """carrier numbers in ascending frequency: -NC/2 .. -1, 1 .. NC/2 (clause 14.5: no DC carrier)"""
    return np.concatenate([np.arange(-NC // 2, 0), np.arange(1, NC // 2 + 1)])


def tx64_slot(k, NC):
    """position of carrier number k in tx64_carriers"""
    k = np.asarray(k)
    return np.where(k < 0, k + NC // 2, k + NC // 2 - 1)


def fft_rounding_bound(N):
    """relative L2 error of a float32 transform of N points against exact arithmetic.  Higham, "Accuracy and Stability of Numerical
    Algorithms" (2nd ed.), Theorem 24.2 (Cooley-Tukey radix 2):
    |y^ - y|_2 / |y|_2 <= log2(N) eta / (1 - log2(N) eta), eta = mu + gamma_4 (sqrt(2) + mu), gamma_4 = 4u / (1 - 4u), mu = the error
    of the stored twiddles, here u (each component is a double-precision value rounded once).  A radix-4 / radix-8 pass is two / three
    radix-2 butterfly levels with exact or once-rounded inner factors, so log2(N) levels in all: c = eta / u = 1 + 4 sqrt(2) ~ 6.66."""
    gamma4 = 4 * U32 / (1 - 4 * U32)
    eta = U32 + gamma4 * (np.sqrt(2.0) + U32)
    t = np.log2(N) * eta
    return t / (1 - t)


# chebyshev_sine.h:13-20: sin(2 pi x) ~ P(x) = (a0 + a1 z + ... + a5 z^5) (z - 1/4) x, z = x x, on [-1/2, 1/2]
TX_CHEB = (-25.13274193, 64.83583069, -67.07687378, 38.50016403, -14.07150173, 3.20396066)


def pll_sample_bound(n, f):
    """|y^_n - x_n e^{2 pi j f n}| / |x_n| for the float32 PLL of DESIGN.md 3.1, sample n of a frame (phase 0 at n = 0):
      * the phase: (float)(n & ~3) * f rounds once (<= u n|f| cycles), base + (k f [+ 1/4]) rounds a value of magnitude <= n|f| + 1 once
        more, k f rounds below u |f| x 4 ... in all <= 2u (n|f| + 1) cycles; d - rint(d) is exact.  In radians: 2 pi 2u (n|f| + 1).
      * the polynomial: its distance from sin(2 pi x) on [-1/2, 1/2] (computed below in float64 from the published coefficients) plus
        Horner in float32: 5 steps of one rounding each (fused) on sum |a_k| z^k <= 46.2 at z = 1/4, times |z - 1/4| |x| <= 1/8, plus the
        three roundings of the closing products on |P| <= 1:  (5 x 46.2 / 8 + 3) u < 32 u.  cos and sin each carry it: a factor sqrt(2).
      * the complex product: < 3u (as in tx_symbol_bound)."""
    x = np.linspace(-0.5, 0.5, 200001)
    z = x * x
    p = np.polyval(TX_CHEB[::-1], z) * (z - 0.25) * x
    approx = float(np.abs(p - np.sin(2 * np.pi * x)).max())
    return 2 * np.pi * 2 * U32 * (n * abs(float(f)) + 1.0) + np.sqrt(2.0) * (approx + 32 * U32) + 3 * U32
