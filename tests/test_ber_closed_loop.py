"""CPU: the closed-loop identity of tests/ber_loop.py for the MODEL on the oracle's soft bits: oracle transmitter -> host model of the
channel (two paths, offset, 15 dB) -> oracle receive chain; every code word is delivered (asserted first), so the model's n_errors are
the differences between the hard decisions and the transmitted bits, and n_bits is K minus the zeros."""
import numpy as np
import pytest

import ber_loop as BL
import ber_model as M
import channel_loop as CL
import channel_model as CM
import tx_encode_cases as T


def test_model_counts_the_transmitted_bits_on_the_oracle_chain(oracle, tmp_path):
    host = CM.build_host_model(tmp_path)
    fib, pay, nb = CL.inputs(oracle)
    frames = T.expected_frames(oracle, CL.SUBS, fib[0], pay[0])
    sent = np.stack([np.unpackbits(f, bitorder="little") for f in frames])
    iq = np.concatenate([oracle.modulate_frame(b) for b in sent]).astype(np.complex64)
    rx = CM.host_apply(host, [CL.params(iq)], iq, 0, CL.N_OUT, False)[0]
    slices = CL.slices_of(rx)
    subs = [T.o_sub(oracle, d) for d in CL.SUBS]
    exp = oracle.receive_frames(slices, CL.STRIDE, CL.P, CL.N_FRAMES, subs)
    CL.check_delivery(exp, fib, pay, nb, oracle)
    ring, st = BL.oracle_soft_frames(oracle, slices)
    assert st.fine_time_offset == exp["state"].fine_time_offset
    for name in ("freq_coarse", "freq_fine"):                       # the frame-by-frame chain above is the oracle's own
        assert np.float32(getattr(st, name)).view(np.uint32) == np.float32(getattr(exp["state"], name)).view(np.uint32), name
    cifs = pay.reshape(4 * CL.N_FRAMES, nb)
    total = 0
    for j in range(CL.N_FRAMES):
        fibb = np.stack([oracle.fic_decode_group(ring[j, 2304 * g:2304 * (g + 1)])[0] for g in range(4)])
        first = max(0, 15 - 4 * j)
        msc = np.zeros((4, nb), np.uint8)
        for q in range(first, 4):
            off = 0
            for sc in subs:
                bits = np.zeros(64 * sc.length, np.int8)
                K = M.kept_bits(oracle, sc)
                bits[:K] = M.consumed(ring, j, q, sc.start_address, K)
                out = oracle.msc_decode_logical(sc, bits)[0]
                msc[q, off:off + out.size] = out
                off += out.size
            assert np.array_equal(msc[q], cifs[4 * j + q - 15]), (j, q)          # delivered: the decoded bytes are the sent ones
        for g in range(4):
            for i in range(3):
                assert np.array_equal(fibb[g, 32 * i:32 * i + 30], fib[0, j, g, i])
                assert oracle.crc16(fibb[g, 32 * i:32 * i + 30]) == 256 * int(fibb[g, 32 * i + 30]) + int(fibb[g, 32 * i + 31])
        if j == CL.N_FRAMES - 1:
            assert np.array_equal(fibb, exp["fib"]) and np.array_equal(msc, exp["msc"])
        fic_r, msc_r = M.ber_frames(oracle, ring, j, subs, fibb, msc)
        total += BL.check_identity(oracle, sent, ring, j, subs, fic_r, msc_r, min(first, 4))
    print(f"channel bit errors over the delivered code words: {total}")
    assert total > 0                                                # 15 dB with a -6 dB echo: the channel does flip bits
