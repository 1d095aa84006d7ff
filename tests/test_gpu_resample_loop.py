"""-m gpu: the two closed loops of tests/resample_loop.py on the device: TxBank -> channel kernel -> resampler -> dabgpu_ofdm_sync_demod_frames
-> dabgpu_decode_frames_layout.  (a) a clock error of CLOCK_PPM, (b) up to 2.4 MS/s and back down at a fractional offset.  The resampler's
output equals the host model's on the same IQ bit for bit; the product's receive outputs equal the CPU oracle chain's on that IQ byte for
byte (the parity contract); every FIB CRC passes, the bytes are the transmitted ones, and the fine time offset of every frame is where T(m)
puts it, +-1 sample.  The operating points were chosen on the CPU: tests/test_resample_closed_loop.py delivers every byte through the host
models and the oracle chain at this noise level and 3 dB below it."""
import numpy as np
import pytest

import channel_loop as CL
import channel_model as CM
import resample_loop as RL
import resample_model as RM
import tx_encode_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def loop(oracle, tmp_path_factory):
    """the transmission through TxBank and the channel kernel, once for both cases: (ctx, rs_host, d_rx, rx, fib, pay, nb)"""
    import dabgpu
    import torch
    d = tmp_path_factory.mktemp("resample_loop_host_models")
    ch_host, rs_host = CM.build_host_model(d), RM.build_host_model(d)
    ctx = dabgpu.Context(0)
    fib, pay, nb = CL.inputs(oracle)
    F, S = CL.N_FRAMES, dabgpu.NB_FRAME_SAMPLES
    bank = dabgpu.TxBank(ctx, 1, [T.g_sub(dabgpu, s) for s in CL.SUBS])
    d_iq = torch.zeros((F * S, 2), dtype=torch.float32, device="cuda")
    bank.transmit_frames(torch.from_numpy(fib).cuda(), torch.from_numpy(pay).cuda(), F, d_iq)
    torch.cuda.synchronize()
    iq = d_iq.cpu().numpy().view(np.complex64).reshape(-1)
    P = CL.params(iq)
    ch = dabgpu.Channel(ctx, [CM.to_struct(P, dabgpu.ChannelStream)])
    n_rx = CL.N_OUT + 256                                                    # (the resampler reads ahead of its output)
    d_rx = torch.zeros((n_rx, 2), dtype=torch.float32, device="cuda")
    ch.apply(d_iq, F * S, n_rx, d_rx)
    torch.cuda.synchronize()
    rx = d_rx.cpu().numpy().view(np.complex64).reshape(-1)
    assert np.array_equal(rx.view(np.uint32), CM.host_apply(ch_host, [P], iq, 0, n_rx, False)[0].view(np.uint32)), "channel output != host model"
    yield ctx, rs_host, d_rx, rx, fib, pay, nb
    ch.close(); bank.close(); ctx.close()


def resample_on_device(ctx, rs_host, P, d_in, x, n_out):
    """one stream through a bank of its own -> (device tensor, host copy), held bit for bit to the host model on the same input"""
    import dabgpu
    import torch
    max_step = RM.design_max_step(P["step_q62"])
    rs = dabgpu.Resampler(ctx, [RM.to_struct(P, dabgpu.ResampleStream)], dabgpu.resample_design(max_step))
    d_out = torch.zeros((n_out + (n_out & 1), 2), dtype=torch.float32, device="cuda")
    rs.apply(d_in, x.size, n_out, d_out)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.complex64).reshape(-1)[:n_out]
    exp = RM.host_apply(rs_host, [P], RM.host_design(rs_host, max_step), x, 0, n_out, False)[0]
    assert np.array_equal(out.view(np.uint32), exp.view(np.uint32)), "resampler output != host model"
    rs.close()
    return d_out, out


def receive_on_device(oracle, ctx, out, predicted, fib, pay, nb):
    """the product's receive chain over the slices of `out`, frame by frame against the oracle chain on the same slices and the prediction"""
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
    offsets = []
    for j in range(F):
        d_slice = torch.from_numpy(np.ascontiguousarray(slices[j:j + 1]).view(np.float32)).cuda()
        ctx.ofdm_sync_demod_frames(d_slice, 1, CL.STRIDE, CL.P, d_st, hist[:, j % H], bits_frame_stride=H * dabgpu.NB_FRAME_BITS)
        ctx.decode_frames(hist, 1, H * dabgpu.NB_FRAME_BITS, H, j % H, gsubs, d_fib, fres, msc, 4 * nb, mres)
        torch.cuda.synchronize()
        masks = fres.cpu().numpy().view(rdt)["crc_ok_mask"]
        assert (masks == 7).all(), f"frame {j}: FIB CRCs {masks}"
        got_fib, got_msc = d_fib.cpu().numpy()[0], msc.cpu().numpy()[0]
        ej = oracle.receive_frames(slices[:j + 1], CL.STRIDE, CL.P, j + 1, osubs)
        sj = d_st.cpu().numpy().view(sdt)[0]
        assert sj["sync_valid"] == 1 and ej["sync_failed"] == 0
        assert sj["fine_time_offset"] == ej["state"].fine_time_offset
        offsets.append(int(sj["fine_time_offset"]))
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
    assert all(abs(o - p) <= 1.0 for o, p in zip(offsets, predicted)), (offsets, predicted)
    return offsets


def test_clock_error_closed_loop(oracle, loop):
    ctx, rs_host, d_rx, rx, fib, pay, nb = loop
    P = RL.clock_params(RL.CLOCK_PPM)
    _, out = resample_on_device(ctx, rs_host, P, d_rx, rx, CL.N_OUT)
    offsets = receive_on_device(oracle, ctx, out, RL.predicted_offsets([P]), fib, pay, nb)
    assert offsets[0] - offsets[-1] >= 38                                    # the clock drifts: 9.83 samples per frame


def test_up_and_down_closed_loop(oracle, loop):
    ctx, rs_host, d_rx, rx, fib, pay, nb = loop
    up, down = RL.updown_params()
    d_high, high = resample_on_device(ctx, rs_host, up, d_rx, rx, RL.N_UP)
    _, out = resample_on_device(ctx, rs_host, down, d_high, high, CL.N_OUT)
    receive_on_device(oracle, ctx, out, RL.predicted_offsets([up, down]), fib, pay, nb)
