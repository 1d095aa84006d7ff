"""CPU: the test-side transmitter model (tests/tx_model.py) -- the composition the -m gpu tests hold modes II-IV to -- equals the
oracle's own mode I restatements of OFDM_Modulator::ProcessBlock and of the frequency-interleaved transmitter, as uint32 bit patterns."""
import numpy as np

import tx_model as TX


def bits(x):
    return np.ascontiguousarray(x, dtype=np.complex64).view(np.uint32)


def test_model_equals_oracle_reference_payload(oracle):
    rng = np.random.default_rng(1301)
    for _ in range(2):
        payload = rng.integers(0, 256, TX.payload_bytes(oracle, 1), dtype=np.uint8)
        got = TX.modulate(oracle, 1, payload, TX.LAYOUT_REFERENCE)
        exp = oracle.modulate_frame_reference_payload(payload)
        assert np.array_equal(bits(got), bits(exp))


def test_model_equals_oracle_frame_bits(oracle):
    rng = np.random.default_rng(1302)
    payload = rng.integers(0, 256, TX.payload_bytes(oracle, 1), dtype=np.uint8)
    got = TX.modulate(oracle, 1, payload, TX.LAYOUT_FRAME_BITS)
    exp = oracle.modulate_frame(np.unpackbits(payload, bitorder="little"))
    assert np.array_equal(bits(got), bits(exp))


def test_model_shapes_all_modes(oracle):
    for mode in (2, 3, 4):
        g = oracle.geometry(mode)
        payload = np.zeros(TX.payload_bytes(oracle, mode), np.uint8)
        f = TX.modulate(oracle, mode, payload, TX.LAYOUT_REFERENCE)
        assert f.size == g.nb_frame_samples
        assert not f[:g.nb_null_period].any()
        # the cyclic prefix repeats the end of each symbol: every symbol of the frame, and the symbols fill it to its last sample
        assert g.nb_null_period + g.nb_frame_symbols * g.nb_symbol_period == f.size
        for s in range(g.nb_frame_symbols):
            p = g.nb_null_period + s * g.nb_symbol_period
            assert np.array_equal(bits(f[p:p + g.nb_cp]), bits(f[p + g.nb_fft:p + g.nb_symbol_period])), (mode, s)
            assert f[p + g.nb_cp:p + g.nb_symbol_period].any(), (mode, s)


def test_quantise_u8_and_scrambler():
    fr = np.array([0, 1 + 1j, -1e9 + 1e9j, complex(np.nan, 0.0), 0.01 - 0.01j], np.complex64)
    q = TX.quantise_u8(None, fr, 0.0, 1536)
    assert q.tolist() == [127, 127, 127, 127, 0, 255, 0, 127, 127, 127]
    # simulate_transmitter.cpp:26-40 by hand: reg = 0xA9 -> v = ((0xA9 ^ 0x152) >> 8) & 0xFF = 1, reg = 0xA901 -> 0xFB, reg = 0x01FB -> 2
    assert TX.scrambler_bytes(3).tolist() == [1, 0xFB, 2]
