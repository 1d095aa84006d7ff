"""-m gpu: the closed loop of tests/channelise_loop.py on the device with THREE ensembles: TxBank x 3 -> channel kernel -> combiner
(the wanted block 300 kHz above the centre of an 8.192 MS/s capture, the neighbours 1.712 MHz to either side and ADJACENT_DB above it) ->
channeliser (all three blocks split back out of the one capture) -> dabgpu_ofdm_sync_demod_frames -> dabgpu_decode_frames_layout.
Combiner and channeliser outputs equal the host model's on the same input bit for bit; the wanted block's receive outputs equal the
CPU oracle chain's byte for byte (the parity contract); all three blocks decode to the bytes each was sent, every FIB CRC, fine time
offset 37 in every frame.  The operating point was chosen on the CPU: tests/test_channelise_closed_loop.py delivers every byte through
the host models and the oracle chain at this noise level and 3 dB below it, and at neighbours 10 dB stronger."""
import numpy as np
import pytest

import channel_loop as CL
import channel_model as CHM
import channelise_loop as XL
import channelise_model as CM
import tx_encode_cases as T

pytestmark = pytest.mark.gpu


def receive_on_device(oracle, ctx, out, fib, pay, nb, against_oracle):
    """the product's receive chain over the slices of `out`, frame by frame; against the oracle chain on the same slices where asked"""
    import dabgpu
    import torch
    gsubs = [T.g_sub(dabgpu, s) for s in CL.SUBS]
    osubs = [T.o_sub(oracle, s) for s in CL.SUBS]
    F, H = CL.N_FRAMES, 8
    slices = CL.slices_of(out)
    sdt, rdt = np.dtype(dabgpu.SYNC_STATE_DTYPE), np.dtype(dabgpu.RESULT_DTYPE)
    d_st = torch.zeros(sdt.itemsize, dtype=torch.uint8, device="cuda")
    hist = torch.zeros((1, H, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
    d_fib = torch.zeros((1, 4, 96), dtype=torch.uint8, device="cuda"); fres = torch.zeros((4, 16), dtype=torch.uint8, device="cuda")
    msc = torch.zeros((1, 4, nb), dtype=torch.uint8, device="cuda"); mres = torch.zeros((4 * len(gsubs), 16), dtype=torch.uint8, device="cuda")
    cifs = pay.reshape(4 * F, nb)
    for j in range(F):
        d_slice = torch.from_numpy(np.ascontiguousarray(slices[j:j + 1]).view(np.float32)).cuda()
        ctx.ofdm_sync_demod_frames(d_slice, 1, CL.STRIDE, CL.P, d_st, hist[:, j % H], bits_frame_stride=H * dabgpu.NB_FRAME_BITS)
        ctx.decode_frames(hist, 1, H * dabgpu.NB_FRAME_BITS, H, j % H, gsubs, d_fib, fres, msc, 4 * nb, mres)
        torch.cuda.synchronize()
        masks = fres.cpu().numpy().view(rdt)["crc_ok_mask"]
        assert (masks == 7).all(), f"frame {j}: FIB CRCs {masks}"
        got_fib, got_msc = d_fib.cpu().numpy()[0], msc.cpu().numpy()[0]
        sj = d_st.cpu().numpy().view(sdt)[0]
        assert sj["sync_valid"] == 1 and sj["fine_time_offset"] == CL.TIMING, (j, sj["fine_time_offset"])
        if against_oracle:
            ej = oracle.receive_frames(slices[:j + 1], CL.STRIDE, CL.P, j + 1, osubs)
            assert ej["sync_failed"] == 0 and sj["fine_time_offset"] == ej["state"].fine_time_offset
            for name in ("freq_coarse", "freq_fine"):
                assert np.float32(sj[name]).view(np.uint32) == np.float32(getattr(ej["state"], name)).view(np.uint32), (j, name)
            assert np.array_equal(got_fib, ej["fib"]), f"frame {j}: FIB bytes differ from the oracle chain"
        for g in range(4):
            for i in range(3):
                assert np.array_equal(got_fib[g, 32 * i:32 * i + 30], fib[j, g, i]), (j, g, i)
        for c in range(4):                                                  # (before CIF 15 the time de-interleaver has no whole logical frame)
            if 4 * j + c >= 15:
                if against_oracle:
                    assert np.array_equal(got_msc[c], ej["msc"][c]), f"frame {j} CIF {c}: sub-channel bytes differ from the oracle chain"
                assert np.array_equal(got_msc[c], cifs[4 * j + c - 15]), f"frame {j} CIF {c}"


def test_three_blocks_through_one_capture(oracle, tmp_path):
    import dabgpu
    import torch
    ch_host, cs_host = CHM.build_host_model(tmp_path), CM.build_host_model(tmp_path)
    ctx = dabgpu.Context(0)
    nb = sum(oracle.subchannel_plan(T.o_sub(oracle, d))[2] for d in CL.SUBS)
    fib, pay = T.random_input(np.random.default_rng(CL.SEED + 1), 3, CL.N_FRAMES, nb)        # three ensembles, three contents
    F, S = CL.N_FRAMES, dabgpu.NB_FRAME_SAMPLES
    bank = dabgpu.TxBank(ctx, 3, [T.g_sub(dabgpu, s) for s in CL.SUBS])
    d_iq = torch.zeros((3, F * S, 2), dtype=torch.float32, device="cuda")
    bank.transmit_frames(torch.from_numpy(fib).cuda(), torch.from_numpy(pay).cuda(), F, d_iq)
    torch.cuda.synchronize()
    iq = d_iq.cpu().numpy().view(np.complex64).reshape(3, F * S)
    # every block through the channel loop's channel (two paths, 50 Hz, 37 samples late, noise at SNR_DB of its own power), its own noise seed
    plist = [dict(CL.params(iq[k]), seed=0xDAB + k) for k in range(3)]
    ch = dabgpu.Channel(ctx, [CHM.to_struct(P, dabgpu.ChannelStream) for P in plist])
    n_blk = CL.N_OUT + XL.EXTRA
    d_rx = torch.zeros((3, n_blk, 2), dtype=torch.float32, device="cuda")
    ch.apply(d_iq, F * S, n_blk, d_rx, in_stride_samples=F * S, out_stride_bytes=n_blk * 8)
    torch.cuda.synchronize()
    rx = d_rx.cpu().numpy().view(np.complex64).reshape(3, n_blk)
    assert np.array_equal(rx.view(np.uint32), CHM.host_apply(ch_host, plist, iq, 0, n_blk, False).view(np.uint32)), "channel output != host model"
    # the combiner: one 8.192 MS/s capture
    chs = XL.channels(XL.ADJACENT_DB)
    G = dabgpu.channeliser_design(XL.D)
    Fh = CM.host_design(cs_host, XL.D)
    assert np.array_equal(np.ctypeslib.as_array(G.table), np.ctypeslib.as_array(Fh.table))
    cb = dabgpu.Channeliser(ctx, [CM.to_struct(c, dabgpu.ChanneliserChannel) for c in chs], 1, G)
    d_wide = torch.zeros((XL.N_WIDE, 2), dtype=torch.float32, device="cuda")
    cb.combine(d_rx, n_blk, XL.N_WIDE, d_wide, in_stride_samples=n_blk)
    torch.cuda.synchronize()
    wide = d_wide.cpu().numpy().view(np.complex64).reshape(-1)
    assert np.array_equal(wide.view(np.uint32), CM.host_combine(cs_host, chs, 1, Fh, rx, 0, 0, XL.N_WIDE, False)[0].view(np.uint32)), "combiner output != host model"
    # the channeliser: all three blocks back out of the capture (the same offsets, the levels taken back)
    back_chs = [dict(c, gain=1.0 / float(np.float32(c["gain"]))) for c in chs]
    cb.set_params([CM.to_struct(c, dabgpu.ChanneliserChannel) for c in back_chs], 0)
    cb.seek(0)
    n_out = CL.N_OUT
    d_back = torch.zeros((3, n_out, 2), dtype=torch.float32, device="cuda")
    cb.split(d_wide, XL.N_WIDE, n_out, d_back, out_stride_bytes=n_out * 8)
    torch.cuda.synchronize()
    back = d_back.cpu().numpy().view(np.complex64).reshape(3, n_out)
    assert np.array_equal(back.view(np.uint32), CM.host_split(cs_host, back_chs, Fh, wide, 0, 0, n_out, False).view(np.uint32)), "channeliser output != host model"
    for k in range(3):
        receive_on_device(oracle, ctx, back[k], fib[k], pay[k], nb, against_oracle=(k == 0))
    cb.close(); ch.close(); bank.close(); ctx.close()
