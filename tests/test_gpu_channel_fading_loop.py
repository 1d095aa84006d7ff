"""-m gpu: the fading closed loop of tests/channel_fading_loop.py on the device: TxBank -> fading bank (`tu6`, Rayleigh at 10 Hz, +37
samples, carrier offset, noise at the operating point chosen on the CPU by tests/test_channel_fading_closed_loop.py) ->
dabgpu_ofdm_sync_demod_frames -> dabgpu_decode_frames_layout, one ensemble, five frames.  The channel's output equals the host model's on
the same IQ bit for bit; sync records, FIB bytes and sub-channel bytes equal the oracle chain's on that IQ (computed here, on the host);
every FIB CRC passes and the bytes are the transmitted ones."""
import numpy as np
import pytest

import channel_fading_loop as FL
import channel_fading_model as FM
import channel_loop as CL
import channel_model as CM
import tx_encode_cases as T

pytestmark = pytest.mark.gpu


def test_txbank_fading_channel_receiver_closed_loop(oracle, tmp_path):
    import dabgpu
    import torch
    host = FM.build_host_model(tmp_path)
    ctx = dabgpu.Context(0)
    fib, pay, nb = CL.inputs(oracle)
    gsubs = [T.g_sub(dabgpu, d) for d in CL.SUBS]
    osubs = [T.o_sub(oracle, d) for d in CL.SUBS]
    F, S = CL.N_FRAMES, dabgpu.NB_FRAME_SAMPLES
    bank = dabgpu.TxBank(ctx, 1, gsubs)
    d_iq = torch.zeros((F * S, 2), dtype=torch.float32, device="cuda")
    bank.transmit_frames(torch.from_numpy(fib).cuda(), torch.from_numpy(pay).cuda(), F, d_iq)
    torch.cuda.synchronize()
    iq = d_iq.cpu().numpy().view(np.complex64).reshape(-1)
    P = FL.params(iq)
    prof = dabgpu.channel_profile("tu6")
    assert [t[0] for t in prof["taps"]] == FL.TU6_DELAYS and np.array_equal(np.float32([t[1] for t in prof["taps"]]), np.float32([t[1] for t in P["taps"]]))
    streams = [CM.to_struct(P, dabgpu.ChannelStream)]
    tables = dabgpu.channel_fading_plan(streams, [dabgpu.channel_fading_spec(FL.DOPPLER_CYCLES, FL.FADING_SEED, prof["kinds"], prof["rice_k"], prof["los_cos"])])
    ch = dabgpu.Channel(ctx, streams, fading=tables)
    assert ch.plan["staged"] == 1 and ch.plan["lds_bytes"] == (1024 + ch.plan["halo"] + 2) * 8 + 1152
    d_rx = torch.zeros((CL.N_OUT, 2), dtype=torch.float32, device="cuda")
    ch.apply(d_iq, F * S, CL.N_OUT, d_rx)
    torch.cuda.synchronize()
    rx = d_rx.cpu().numpy().view(np.complex64).reshape(-1)
    model = FM.host_apply(host, [P], [FM.from_struct(tables[0], 6)], iq, 0, CL.N_OUT, False)[0]
    assert np.array_equal(rx.view(np.uint32), model.view(np.uint32)), "channel output != host model"
    slices = CL.slices_of(rx)
    exp = oracle.receive_frames(slices, CL.STRIDE, CL.P, F, osubs)
    assert FL.delivered(exp, fib, pay, nb)                                  # (the oracle on the device's IQ: what the CPU test showed)
    H = 8
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
        ej = oracle.receive_frames(slices[:j + 1], CL.STRIDE, CL.P, j + 1, osubs)   # the oracle chain after the same j + 1 frames
        sj = d_st.cpu().numpy().view(sdt)[0]
        assert sj["sync_valid"] == 1 and sj["fine_time_offset"] == ej["state"].fine_time_offset
        for name in ("freq_coarse", "freq_fine"):
            assert np.float32(sj[name]).view(np.uint32) == np.float32(getattr(ej["state"], name)).view(np.uint32), (j, name)
        assert np.array_equal(got_fib, ej["fib"]), f"frame {j}: FIB bytes differ from the oracle chain"
        for g in range(4):
            for i in range(3):
                assert np.array_equal(got_fib[g, 32 * i:32 * i + 30], fib[0, j, g, i]), (j, g, i)
        for c in range(4):                                                  # (before CIF 15 the time de-interleaver has no whole logical frame)
            if 4 * j + c >= 15:
                assert np.array_equal(got_msc[c], ej["msc"][c]), f"frame {j} CIF {c}: sub-channel bytes differ from the oracle chain"
                assert np.array_equal(got_msc[c], cifs[4 * j + c - 15]), f"frame {j} CIF {c}"
    assert exp["fib_crc_ok"] == 12 * F and np.array_equal(got_fib, exp["fib"]) and np.array_equal(got_msc, exp["msc"])
    ch.close(); bank.close(); ctx.close()
