"""-m gpu: the closed loop of tests/channel_loop.py on the device with the channel BER behind it: TxBank.encode_frames (the sent frame bits
are kept) -> OFDM modulator -> channel kernel (two paths, offset, 15 dB) -> dabgpu_ofdm_sync_demod_frames -> dabgpu_decode_frames_layout ->
dabgpu_ber_frames_layout.  Every code word is delivered (asserted first); then its n_errors is the number of consumed soft bits whose
hard decision differs from the TRANSMITTED bit and n_bits is K minus the zeros (tests/ber_loop.py) -- exactly; and the device's records
equal the model's on the device's soft bits."""
import numpy as np
import pytest

import ber_loop as BL
import ber_model as M
import channel_loop as CL
import channel_model as CM
import tx_encode_cases as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layout", [0, 1])
def test_errors_counted_on_the_device_are_the_flipped_transmitted_bits(oracle, layout):
    import dabgpu
    import torch
    ctx = dabgpu.Context(0)
    fib, pay, nb = CL.inputs(oracle)
    gsubs = [T.g_sub(dabgpu, d) for d in CL.SUBS]
    osubs = [T.o_sub(oracle, d) for d in CL.SUBS]
    F, S, H = CL.N_FRAMES, dabgpu.NB_FRAME_SAMPLES, 8
    bank = dabgpu.TxBank(ctx, 1, gsubs)
    d_bits = torch.zeros((F, dabgpu.NB_FRAME_BITS // 8), dtype=torch.uint8, device="cuda")
    bank.encode_frames(torch.from_numpy(fib).cuda(), torch.from_numpy(pay).cuda(), F, d_bits)
    d_iq = torch.zeros((F * S, 2), dtype=torch.float32, device="cuda")
    ctx.ofdm_modulate_frames(1, d_bits, F, d_iq, layout=dabgpu.TX_PAYLOAD_FRAME_BITS)
    torch.cuda.synchronize()
    sent = np.zeros((H, dabgpu.NB_FRAME_BITS), np.uint8)
    sent[:F] = np.unpackbits(d_bits.cpu().numpy(), axis=1, bitorder="little")
    assert np.array_equal(np.packbits(sent[:F], axis=1, bitorder="little"), T.expected_frames(oracle, CL.SUBS, fib[0], pay[0]))
    iq = d_iq.cpu().numpy().view(np.complex64).reshape(-1)
    ch = dabgpu.Channel(ctx, [CM.to_struct(CL.params(iq), dabgpu.ChannelStream)])
    d_rx = torch.zeros((CL.N_OUT, 2), dtype=torch.float32, device="cuda")
    ch.apply(d_iq, F * S, CL.N_OUT, d_rx)
    torch.cuda.synchronize()
    slices = CL.slices_of(d_rx.cpu().numpy().view(np.complex64).reshape(-1))
    sdt, rdt = np.dtype(dabgpu.SYNC_STATE_DTYPE), np.dtype(dabgpu.RESULT_DTYPE)
    d_st = torch.zeros(sdt.itemsize, dtype=torch.uint8, device="cuda")
    hist = torch.zeros((1, H, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
    d_fib = torch.zeros((1, 4, 96), dtype=torch.uint8, device="cuda"); fres = torch.zeros((4, 16), dtype=torch.uint8, device="cuda")
    msc = torch.zeros((1, 4, nb), dtype=torch.uint8, device="cuda"); mres = torch.zeros((4 * len(gsubs), 16), dtype=torch.uint8, device="cuda")
    fic_r = torch.zeros((1, 4, 16), dtype=torch.uint8, device="cuda"); msc_r = torch.zeros((1, 4, len(gsubs), 16), dtype=torch.uint8, device="cuda")
    cifs = pay.reshape(4 * F, nb)
    to_natural = dabgpu.classed_to_natural_index()
    total = 0
    for j in range(F):
        d_slice = torch.from_numpy(np.ascontiguousarray(slices[j:j + 1]).view(np.float32)).cuda()
        ctx.ofdm_sync_demod_frames(d_slice, 1, CL.STRIDE, CL.P, d_st, hist[:, j % H], bits_frame_stride=H * dabgpu.NB_FRAME_BITS, bits_layout=layout)
        ctx.decode_frames(hist, 1, H * dabgpu.NB_FRAME_BITS, H, j % H, gsubs, d_fib, fres, msc, 4 * nb, mres, bits_layout=layout)
        ctx.ber_frames(hist, 1, H * dabgpu.NB_FRAME_BITS, H, j % H, gsubs, d_fib, msc, 4 * nb, fic_r, msc_r, bits_layout=layout)
        torch.cuda.synchronize()
        # delivered: every FIB CRC, the FIB bodies and the sub-channel bytes are the sent ones
        assert (fres.cpu().numpy().view(rdt)["crc_ok_mask"] == 7).all(), j
        got_fib, got_msc = d_fib.cpu().numpy()[0], msc.cpu().numpy()[0]
        first = min(max(0, 15 - 4 * j), 4)
        for g in range(4):
            for i in range(3):
                assert np.array_equal(got_fib[g, 32 * i:32 * i + 30], fib[0, j, g, i]), (j, g, i)
        for q in range(first, 4):
            assert np.array_equal(got_msc[q], cifs[4 * j + q - 15]), (j, q)
        ring = hist.cpu().numpy()[0]
        if layout == dabgpu.BITS_MSC_CLASSED:
            ring = ring[:, to_natural]
        got_f, got_m = fic_r.cpu().numpy().view(M.BER_DTYPE).reshape(4), msc_r.cpu().numpy().view(M.BER_DTYPE).reshape(4, len(gsubs))
        total += BL.check_identity(oracle, sent, ring, j, osubs, got_f, got_m, first)
        # ... and device = model on the device's soft bits, every field (the CIFs without a whole logical frame included)
        exp_f, exp_m = M.ber_frames(oracle, ring, j, osubs, got_fib, got_msc)
        assert np.array_equal(got_f, exp_f) and np.array_equal(got_m, exp_m), j
    assert total > 0
    ch.close(); bank.close(); ctx.close()
