"""-m gpu: the closed loop of tests/channel_loop.py on the device: TxBank -> channel kernel (two paths, carrier offset, +37 samples, noise
at 15 dB) -> dabgpu_ofdm_sync_demod_frames -> dabgpu_decode_frames_layout.  The channel's output equals the host model's on the same IQ bit
for bit; the receive outputs equal the CPU oracle chain's on that IQ byte for byte (the parity contract); every FIB CRC passes and the
sub-channel bytes are the transmitted ones.  The noise level was chosen on the CPU: tests/test_channel_closed_loop.py delivers every byte
through host model -> oracle chain at this level and 3 dB below it."""
import numpy as np
import pytest

import channel_loop as CL
import channel_model as CM
import tx_encode_cases as T

pytestmark = pytest.mark.gpu


def test_txbank_channel_receiver_closed_loop(oracle, tmp_path):
    import dabgpu
    import torch
    host = CM.build_host_model(tmp_path)
    ctx = dabgpu.Context(0)
    fib, pay, nb = CL.inputs(oracle)
    gsubs = [T.g_sub(dabgpu, d) for d in CL.SUBS]
    osubs = [T.o_sub(oracle, d) for d in CL.SUBS]
    F, S = CL.N_FRAMES, dabgpu.NB_FRAME_SAMPLES
    bank = dabgpu.TxBank(ctx, 1, gsubs)
    assert bank.cif_in_bytes == nb
    d_iq = torch.zeros((F * S, 2), dtype=torch.float32, device="cuda")
    bank.transmit_frames(torch.from_numpy(fib).cuda(), torch.from_numpy(pay).cuda(), F, d_iq)
    torch.cuda.synchronize()
    iq = d_iq.cpu().numpy().view(np.complex64).reshape(-1)
    P = CL.params(iq)
    ch = dabgpu.Channel(ctx, [CM.to_struct(P, dabgpu.ChannelStream)])
    d_rx = torch.zeros((CL.N_OUT, 2), dtype=torch.float32, device="cuda")
    ch.apply(d_iq, F * S, CL.N_OUT, d_rx)
    torch.cuda.synchronize()
    rx = d_rx.cpu().numpy().view(np.complex64).reshape(-1)
    assert np.array_equal(rx.view(np.uint32), CM.host_apply(host, [P], iq, 0, CL.N_OUT, False)[0].view(np.uint32)), "channel output != host model"
    slices = CL.slices_of(rx)
    exp = oracle.receive_frames(slices, CL.STRIDE, CL.P, F, osubs)
    CL.check_delivery(exp, fib, pay, nb, oracle)                            # (the oracle on the device's IQ: what the CPU test showed)
    # the product's receive chain over the same slices
    H = 8
    sdt = np.dtype(dabgpu.SYNC_STATE_DTYPE)
    rdt = np.dtype(dabgpu.RESULT_DTYPE)
    d_st = torch.zeros(sdt.itemsize, dtype=torch.uint8, device="cuda")
    hist = torch.zeros((1, H, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
    d_fib = torch.zeros((1, 4, 96), dtype=torch.uint8, device="cuda"); fres = torch.zeros((4, 16), dtype=torch.uint8, device="cuda")
    msc = torch.zeros((1, 4, nb), dtype=torch.uint8, device="cuda"); mres = torch.zeros((4 * len(gsubs), 16), dtype=torch.uint8, device="cuda")
    n_crc = 0
    cifs = pay.reshape(4 * F, nb)
    for j in range(F):
        d_slice = torch.from_numpy(np.ascontiguousarray(slices[j:j + 1]).view(np.float32)).cuda()
        ctx.ofdm_sync_demod_frames(d_slice, 1, CL.STRIDE, CL.P, d_st, hist[:, j % H], bits_frame_stride=H * dabgpu.NB_FRAME_BITS)
        ctx.decode_frames(hist, 1, H * dabgpu.NB_FRAME_BITS, H, j % H, gsubs, d_fib, fres, msc, 4 * nb, mres)
        torch.cuda.synchronize()
        masks = fres.cpu().numpy().view(rdt)["crc_ok_mask"]
        assert (masks == 7).all(), f"frame {j}: FIB CRCs {masks}"
        n_crc += 12
        got_fib, got_msc = d_fib.cpu().numpy()[0], msc.cpu().numpy()[0]
        # the oracle chain after the same j + 1 frames: its state, FIB bytes and sub-channel bytes of this frame
        ej = oracle.receive_frames(slices[:j + 1], CL.STRIDE, CL.P, j + 1, osubs)
        sj = d_st.cpu().numpy().view(sdt)[0]
        assert sj["fine_time_offset"] == ej["state"].fine_time_offset
        for name in ("freq_coarse", "freq_fine"):
            assert np.float32(sj[name]).view(np.uint32) == np.float32(getattr(ej["state"], name)).view(np.uint32), (j, name)
        assert np.array_equal(got_fib, ej["fib"]), f"frame {j}: FIB bytes differ from the oracle chain"
        for c in range(4):                                                  # (before CIF 15 the time de-interleaver has no whole logical frame)
            if 4 * j + c >= 15:
                assert np.array_equal(got_msc[c], ej["msc"][c]), f"frame {j} CIF {c}: sub-channel bytes differ from the oracle chain"
        for g in range(4):
            for i in range(3):
                assert np.array_equal(got_fib[g, 32 * i:32 * i + 30], fib[0, j, g, i]), (j, g, i)
        for c in range(4):
            if 4 * j + c >= 15:
                assert np.array_equal(got_msc[c], cifs[4 * j + c - 15]), f"frame {j} CIF {c}"
    assert n_crc == exp["fib_crc_ok"] == 12 * F
    st = d_st.cpu().numpy().view(sdt)[0]
    assert st["sync_valid"] == 1 and st["fine_time_offset"] == exp["state"].fine_time_offset == CL.TIMING
    for name in ("freq_coarse", "freq_fine"):
        assert np.float32(st[name]).view(np.uint32) == np.float32(getattr(exp["state"], name)).view(np.uint32), name
    assert np.array_equal(got_fib, exp["fib"]) and np.array_equal(got_msc, exp["msc"])
    ch.close(); bank.close(); ctx.close()
