"""CPU: the numpy model of the channel BER (tests/ber_model.py) on frames whose content is known.  Noise-free frames as the oracle
composes them (tests/tx_encode_cases.expected_frames), mapped to +-127 and decoded by the oracle: no errors, every bit counted, weight
127 K.  Then k isolated sign flips and m erasures in one code word: exactly k errors, K - m bits, the flipped magnitudes as error
weight -- with k and the spacing chosen so that the oracle's decoder alone still returns the sent bytes, which is asserted."""
import numpy as np
import pytest

import ber_model as M
import channel_loop as CL
import tx_encode_cases as T

F = 5                                        # 20 CIFs: CIFs 15 .. 19 have their whole logical frame in the ring


@pytest.fixture(scope="module")
def clean(oracle):
    subs = [T.o_sub(oracle, d) for d in CL.SUBS]
    nb = sum(oracle.subchannel_plan(s)[2] for s in subs)
    fib, pay = T.random_input(np.random.default_rng(7700), 1, F, nb)
    frames = T.expected_frames(oracle, CL.SUBS, fib[0], pay[0])
    ring = np.stack([oracle.soft_from_bits(np.unpackbits(f, bitorder="little")) for f in frames])      # [5][230400], slot = frame
    return subs, nb, fib[0], pay[0].reshape(4 * F, nb), ring


def decode_frame(oracle, ring, newest, subs):
    """the oracle's decoders on the ring: FIB bytes [4][96], sub-channel bytes [4][B] of the frame in slot `newest`"""
    fib = np.stack([oracle.fic_decode_group(ring[newest, 2304 * g:2304 * (g + 1)])[0] for g in range(4)])
    rows = []
    for q in range(4):
        row = []
        for sc in subs:
            bits = np.zeros(sc.length * 64, np.int8)
            K = M.kept_bits(oracle, sc)
            bits[:K] = M.consumed(ring, newest, q, sc.start_address, K)
            row.append(oracle.msc_decode_logical(sc, bits)[0])
        rows.append(np.concatenate(row))
    return fib, np.stack(rows)


def test_the_models_code_words_and_index_are_the_oracles(oracle, clean):
    subs, nb, fib, cifs, ring = clean
    for g in range(4):
        body = fib[2, g].reshape(90)
        b96 = oracle.fic_decode_group(oracle.soft_from_bits(oracle.fic_encode_group(body)))[0]
        assert np.array_equal(b96.reshape(3, 32)[:, :30].reshape(90), body)
        assert np.array_equal(M.fic_codeword(oracle, b96), oracle.fic_encode_group(body))
    # the explicit de-interleave index against the oracle's CIF_Deinterleaver, fed CIF by CIF
    sc = subs[1]
    de = oracle.Deinterleaver(sc.length * 8)
    for t in range(4 * F):
        de.consume(ring[t // 4, M.FIC_BITS + M.CIF_BITS * (t % 4) + 64 * sc.start_address:][:64 * sc.length])
        out = de.deinterleave()
        if t >= 15:
            assert np.array_equal(out, M.consumed(ring, t // 4, t % 4, sc.start_address, 64 * sc.length)), t
    assert np.array_equal(M.to_classed(ring)[:, M.FIC_BITS + 3 * M.CIF_BITS + 5 * 3456 + 7], ring[:, M.FIC_BITS + 3 * M.CIF_BITS + 16 * 7 + 5])


def test_noise_free_frames_have_no_errors_and_full_weight(oracle, clean):
    subs, nb, fib, cifs, ring = clean
    for newest in range(F):
        fibb, msc = decode_frame(oracle, ring, newest, subs)
        fic_r, msc_r = M.ber_frames(oracle, ring, newest, subs, fibb, msc)
        for g in range(4):
            assert tuple(fic_r[g]) == (2304, 0, 0, 127 * 2304), (newest, g)
        for q in range(4):
            if 4 * newest + q < 15:
                continue
            assert np.array_equal(msc[q], cifs[4 * newest + q - 15])
            for s, sc in enumerate(subs):
                K = M.kept_bits(oracle, sc)
                assert tuple(msc_r[q, s]) == (K, 0, 0, 127 * K), (newest, q, s)


def perturb(values, code, k, m, spacing):
    """values int8 [K] (noise free): k sign flips `spacing` apart with assorted magnitudes, m zeros between them -> new values, flipped weight"""
    v = values.copy()
    mags = [1, 64, 127, 128, 33]
    flips = 40 + spacing * np.arange(k)
    zeros = 40 + spacing // 2 + spacing * np.arange(m)
    assert flips[-1] < v.size and zeros[-1] < v.size
    weight = 0
    for n, i in enumerate(flips):
        mag = mags[n % len(mags)]
        if code[i] == 0 and mag == 128:            # sent -127: the flipped value is positive, 128 does not exist
            mag = 127
        v[i] = -mag if code[i] else mag
        weight += mag
    v[zeros] = 0
    return v, int(weight), int(np.abs(v.astype(np.int64)).sum())


@pytest.mark.parametrize("which", ["fic", "eep", "uep"])
def test_isolated_flips_and_erasures_are_counted_exactly(oracle, clean, which):
    subs, nb, fib, cifs, ring = clean
    ring = ring.copy()
    newest, q, k, m, spacing = F - 1, 3, 12, 9, 150
    if which == "fic":
        g = 2
        view = ring[newest, 2304 * g:2304 * (g + 1)]
        code = (view > 0).astype(np.uint8)
        new, weight, total = perturb(view, code, k, m, spacing)
        ring[newest, 2304 * g:2304 * (g + 1)] = new
        fibb, msc = decode_frame(oracle, ring, newest, subs)
        for i in range(3):                                           # the oracle's decoder alone still returns what was sent
            assert np.array_equal(fibb[g, 32 * i:32 * i + 30], fib[newest, g, i])
        assert oracle.fic_decode_group(new)[1] == 7
        fic_r, _ = M.ber_frames(oracle, ring, newest, subs, fibb, None)
        assert tuple(fic_r[g]) == (2304 - m, k, weight, total)
        for o in (0, 1, 3):
            assert tuple(fic_r[o]) == (2304, 0, 0, 127 * 2304)
        return
    s = 0 if which == "eep" else 1
    sc = subs[s]
    K = M.kept_bits(oracle, sc)
    i = np.arange(K)
    slot = (4 * newest + q - (15 - M.CIF_DELAY[i % 16])) % (4 * F)
    fr, pos = slot // 4, M.FIC_BITS + M.CIF_BITS * (slot % 4) + 64 * sc.start_address + i
    view = ring[fr, pos]
    code = (view > 0).astype(np.uint8)
    new, weight, total = perturb(view, code, k, m, spacing)
    ring[fr, pos] = new
    fibb, msc = decode_frame(oracle, ring, newest, subs)
    assert np.array_equal(msc[q], cifs[4 * newest + q - 15])       # the oracle's decoder alone still returns what was sent
    _, msc_r = M.ber_frames(oracle, ring, newest, subs, None, msc)
    assert tuple(msc_r[q, s]) == (K - m, k, weight, total)
    o = 1 - s
    Ko = M.kept_bits(oracle, subs[o])
    assert tuple(msc_r[q, o]) == (Ko, 0, 0, 127 * Ko)
    assert tuple(msc_r[q - 1, s]) == (K, 0, 0, 127 * K)
