"""Test-side model of the OFDM transmitter (dabgpu_ofdm_modulate_frames) for any transmission mode, composed from pinned oracle pieces:
the float32 DQPSK chain in the oracle's operation order (re = x.re*z.re - x.im*z.im, im = x.re*z.im + x.im*z.re, no fused operations),
oracle.fft_n(inverse=True), the cyclic prefix, the NULL period first.  tests/test_tx_model.py holds it to the oracle's own mode I
restatements (modulate_frame_reference_payload, modulate_frame) bit for bit; the GPU tests hold the device to it in modes II-IV."""
import numpy as np

LAYOUT_REFERENCE = 0
LAYOUT_FRAME_BITS = 1
A_REF = np.float32(1.0) / np.float32(1.41421356237309505)      # 1.0f / std::sqrt(2.0f)
A_BITS = np.float32(0.707106769084930420)


def carrier_bins(N, NC):
    """carrier index in natural order -> FFT bin (ofdm_modulator.cpp:106-126)"""
    c = np.arange(NC)
    M = NC // 2
    return np.where(c < M, N - M + c, c - M + 1)


def payload_bytes(oracle, mode):
    g = oracle.geometry(mode)
    return (g.nb_frame_symbols - 1) * g.nb_carriers // 4


def _z_symbol(sym_bytes, layout, NC, mapper):
    """(zr, zi) float32 in natural carrier order for one data symbol's payload bytes"""
    if layout == LAYOUT_REFERENCE:
        c = np.arange(NC)
        v = (sym_bytes[c // 4].astype(np.uint32) >> (2 * (c % 4)).astype(np.uint32)) & 3
        zr = np.where((v == 1) | (v == 2), A_REF, -A_REF).astype(np.float32)
        zi = np.where(v >= 2, A_REF, -A_REF).astype(np.float32)
    else:
        b = np.unpackbits(sym_bytes, bitorder="little")
        zr = np.empty(NC, np.float32)
        zi = np.empty(NC, np.float32)
        zr[mapper] = np.where(b[:NC] != 0, -A_BITS, A_BITS)
        zi[mapper] = np.where(b[NC:] != 0, -A_BITS, A_BITS)
    return zr, zi


def modulate(oracle, mode, payload, layout, prs=None, mapper=None):
    """one frame, NULL first: complex64 [nb_frame_samples]"""
    g = oracle.geometry(mode)
    N, NC, L, P, CP = g.nb_fft, g.nb_carriers, g.nb_frame_symbols, g.nb_symbol_period, g.nb_cp
    prs = (oracle.prs_fft_mode(mode) if prs is None else np.asarray(prs)).astype(np.complex64)
    mapper = oracle.mapper_n(N, NC) if mapper is None else np.asarray(mapper)
    payload = np.ascontiguousarray(payload, dtype=np.uint8).reshape(L - 1, NC // 4)
    bins = carrier_bins(N, NC)
    out = np.zeros(g.nb_frame_samples, np.complex64)

    def put(s, spec):
        t = oracle.fft_n(spec, inverse=True)
        p = g.nb_null_period + s * P
        out[p:p + CP] = t[N - CP:]
        out[p + CP:p + P] = t

    put(0, prs)
    xr = prs.real[bins].astype(np.float32)
    xi = prs.imag[bins].astype(np.float32)
    for s in range(1, L):
        zr, zi = _z_symbol(payload[s - 1], layout, NC, mapper)
        nr = xr * zr - xi * zi
        ni = xr * zi + xi * zr
        xr, xi = nr, ni
        spec = np.zeros(N, np.complex64)
        spec.real[bins] = xr
        spec.imag[bins] = xi
        put(s, spec)
    return out


def quantise_u8(oracle, frame, freq_norm, n_carriers):
    """simulate_transmitter.cpp:167-178 on one frame: optional apply_pll, then QuantisedIQ<uint8_t>::from_iq(I*scale, Q*scale)"""
    frame = np.asarray(frame, np.complex64)
    if np.float32(freq_norm) != 0:
        frame = oracle.apply_pll(frame, np.float32(freq_norm))
    scale = (np.float32(1.0) / np.float32(n_carriers) * np.float32(4.0)) * np.float32(127.5)
    x = np.ascontiguousarray(frame).view(np.float32)
    v = x * scale
    v = v + np.float32(127.5)
    v = np.where(v > 0, v, np.float32(0))
    v = np.where(v > 255, np.float32(255), v)
    return v.astype(np.uint8)


def freq_norm(hz):
    """simulate_transmitter.cpp:169-170: frequency / 2.048e6f in float"""
    return np.float32(np.float32(hz) / np.float32(2.048e6))


SERIES_SHIFT = freq_norm(3000.0)            # the shift of the run-length series (tests/tx_variants_child.py)


def shift_cases():
    """the freq_norm values the transmitter tests use (float32, as the ABI takes them): the CLI's Hz values, the run-length series' shift,
    and the edges -- tiny, a quarter cycle per sample, just under half a cycle, both signs.  tests/test_independent_pins.py holds
    oracle.apply_pll to a float64 rotation at every one of them; tests/test_gpu_ofdm_modulator_variants.py holds the device to
    oracle.apply_pll."""
    hz = [freq_norm(1000.0), freq_norm(-2500.0), SERIES_SHIFT]
    edges = [np.float32(v) for v in (2.0 ** -20, 1e-7, 0.25, -0.25, 0.4999, -0.4999)]
    return hz + edges


def to_frame_buffer(oracle, mode, tx_frame):
    """a NULL-first frame -> the demodulator's frame-buffer layout (PRS first, the following frame's NULL -- zeros -- last)"""
    g = oracle.geometry(mode)
    out = np.zeros(g.nb_frame_samples, np.complex64)
    out[:g.nb_frame_samples - g.nb_null_period] = tx_frame[g.nb_null_period:]
    return out


def scrambler_bytes(n):
    """the DVB scrambler of simulate_transmitter.cpp:26-40, reset to its sync word"""
    reg = 0b0000000010101001
    out = np.empty(n, np.uint8)
    for i in range(n):
        v = (((reg ^ (reg << 1)) & 0xFFFF) >> 8) & 0xFF
        reg = ((reg << 8) | v) & 0xFFFF
        out[i] = v
    return out
