"""Shared by the closed-loop tests of the channel BER (not a test module): tests/channel_loop.py's loop as it stands -- two paths, carrier
offset, 37 samples late, 15 dB -- with the transmitted frame bits kept.  For a code word whose decoded bytes equal the sent ones the
re-encoded code word IS the transmitted one, so n_errors must equal the number of consumed soft bits whose hard decision differs from the
transmitted bit at the same place of the same frame (the time interleaver's work is already in the transmitted frames) and n_bits must be
K minus the zeros: an exact identity between the receive half and the transmit half, with no tolerance."""
import numpy as np

import ber_model as M
import channel_loop as CL


def oracle_soft_frames(oracle, slices):
    """the oracle's receive chain up to the soft bits, frame by frame as dab_receive_frames runs it (oracle/dab_oracle_chain.c): coarse
    frequency, fine time, demodulation at the summed offset, fine-frequency update -> bits [F][230400], the final state"""
    st = oracle.SyncState(0.0, 0.0, 0, 0, 0, 0)
    conj_ref, time_ref = oracle.sync_refs()
    out = []
    for sl in slices:
        prs = sl[CL.P:]
        oracle.coarse_freq_sync(prs, st, prs_time_ref=time_ref)
        f = np.float32(np.float32(st.freq_coarse) + np.float32(st.freq_fine))
        ok, off, _ = oracle.fine_time_sync(prs, f, prs_fft_conj=conj_ref)
        assert ok
        st.fine_time_offset = off
        d = oracle.demod_frame(sl[CL.P + off:CL.P + off + 196608], f)
        st.freq_fine = float(oracle.update_fine_freq(st.freq_fine, d["total_phase"]))
        out.append(d["bits"])
    return np.stack(out), st


def truth(oracle, sent, ring, newest, subs):
    """(n_bits, n_errors) against the TRANSMITTED bits: sent [H][230400] 0/1 and ring [H][230400] soft bits (natural order), both with
    frame j in slot j -> fic [4][2], msc [4][n_sub][2]"""
    def count(soft, bits):
        nz = soft != 0
        return int(nz.sum()), int((nz & ((soft >= 0) != (bits != 0))).sum())
    fic = np.array([count(ring[newest, 2304 * g:2304 * (g + 1)], sent[newest, 2304 * g:2304 * (g + 1)]) for g in range(4)])
    msc = np.zeros((4, len(subs), 2), np.int64)
    for q in range(4):
        for s, sc in enumerate(subs):
            K = M.kept_bits(oracle, sc)
            msc[q, s] = count(M.consumed(ring, newest, q, sc.start_address, K), M.consumed(sent, newest, q, sc.start_address, K))
    return fic, msc


def check_identity(oracle, sent, ring, newest, subs, fic_rec, msc_rec, first_cif):
    """records (BER_DTYPE: fic [4], msc [4][n_sub]) of the frame in slot `newest` against the transmitted bits; CIFs before `first_cif` of
    the frame have no whole logical frame in the ring yet"""
    fic_t, msc_t = truth(oracle, sent, ring, newest, subs)
    errors = 0
    for g in range(4):
        assert (int(fic_rec[g]["n_bits"]), int(fic_rec[g]["n_errors"])) == tuple(fic_t[g]), (newest, g)
        errors += int(fic_rec[g]["n_errors"])
    for q in range(first_cif, 4):
        for s in range(len(subs)):
            assert (int(msc_rec[q, s]["n_bits"]), int(msc_rec[q, s]["n_errors"])) == tuple(msc_t[q, s]), (newest, q, s)
            errors += int(msc_rec[q, s]["n_errors"])
    return errors
