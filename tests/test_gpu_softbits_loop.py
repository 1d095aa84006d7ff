"""-m gpu: the closed loop of tests/softbit_loop.py on the device: TxBank -> fading bank (`tu6`, six Rayleigh taps at 10 Hz, +37 samples,
no carrier offset, noise) -> dabgpu_ofdm_sync_demod_frames / dabgpu_ofdm_sync_demod_frames_soft -> dabgpu_decode_frames_layout, one
ensemble, five frames, at the operating points of tests/test_softbit_closed_loop.py.  The rule is the CPU test's: the reference's soft
bits do not deliver (fewer than 60 FIB CRCs or a wrong byte in the EEP 3-A sub-channel's five delivered logical frames), the weighted
ones (level 64) deliver everything.  Unlike the CPU experiment, which cuts the frame at the known position, this chain runs the real
synchroniser.  Measured on an MI355X over the grid the CPU test tabulates (FIB CRCs of 60 / wrong bytes, normalised -> weighted):

    SNR dB  seed 0        1              2            3            4            5            6            7              totals
       6    34/62->58/2   36/667->36/454 36/212->36/34 36/239->54/43 53/216->60/7 44/118->60/0 47/180->48/77 9/686->20/332  295/2380 -> 372/949
       7    45/25->58/0   36/464->37/266 36/89->37/5  42/84->56/7  59/111->60/0 55/42->60/0  48/89->48/25 19/475->27/101  340/1379 -> 383/404
       8    49/6->60/0    36/277->46/110 36/37->50/0  49/30->58/3  60/44->60/0  58/16->60/0  48/28->48/7  21/292->39/32   357/730  -> 421/152
       9    57/0->60/0    38/139->55/33  39/12->56/0  54/15->60/2  60/18->60/0  59/5->60/0   48/4->48/4   30/122->43/12   385/315  -> 442/51
      10    60/0->60/0    44/26->59/8    48/8->60/0   57/5->60/3   60/1->60/0   60/0->60/0   48/2->49/0   38/64->54/0     415/106  -> 462/11
      11    60/0->60/0    54/7->60/0     55/0->60/0   59/0->60/0   60/1->60/0   60/0->60/0   48/0->52/0   42/19->58/0     438/27   -> 470/0
      12    60/0->60/0    60/0->60/0     59/0->60/0   60/0->60/0   60/0->60/0   60/0->60/0   48/0->59/0   54/5->59/0      461/5    -> 478/0

No frame of the grid was refused by the synchroniser.  Both points of the CPU test carry over: (10 dB, seed 2) 48/8 -> 60/0 and
(8 dB, seed 0) 49/6 -> 60/0."""
import numpy as np
import pytest

import channel_fading_loop as FL
import channel_loop as CL
import channel_model as CM
import softbit_loop as SL
import tx_encode_cases as T

pytestmark = pytest.mark.gpu


class Chain:
    """the transmission on the device, once; a point = (SNR, fading seed, policy) through channel, receiver and decoders"""

    def __init__(self, oracle):
        import dabgpu
        import torch
        self.dabgpu, self.torch = dabgpu, torch
        self.ctx = dabgpu.Context(0)
        self.fib, self.pay, self.nb = CL.inputs(oracle)
        self.gsubs = [T.g_sub(dabgpu, d) for d in CL.SUBS]
        self.n0 = oracle.subchannel_plan(T.o_sub(oracle, CL.SUBS[0]))[2]
        F, S = CL.N_FRAMES, dabgpu.NB_FRAME_SAMPLES
        bank = dabgpu.TxBank(self.ctx, 1, self.gsubs)
        self.d_iq = torch.zeros((F * S, 2), dtype=torch.float32, device="cuda")
        bank.transmit_frames(torch.from_numpy(self.fib).cuda(), torch.from_numpy(self.pay).cuda(), F, self.d_iq)
        torch.cuda.synchronize()
        bank.close()
        self.iq = self.d_iq.cpu().numpy().view(np.complex64).reshape(-1)
        self.prof = dabgpu.channel_profile("tu6")

    def close(self):
        self.ctx.close()

    def point(self, snr_db, seed, policy):
        """-> (FIB CRCs of 60, wrong bytes of sub-channel 0's delivered logical frames, frames the synchroniser refused)"""
        dabgpu, torch, ctx = self.dabgpu, self.torch, self.ctx
        F, nb, H = CL.N_FRAMES, self.nb, 8
        streams = [CM.to_struct(SL.params(self.iq, snr_db), dabgpu.ChannelStream)]
        tables = dabgpu.channel_fading_plan(streams, [dabgpu.channel_fading_spec(FL.DOPPLER_CYCLES, seed, self.prof["kinds"], self.prof["rice_k"],
                                                                                  self.prof["los_cos"])])
        ch = dabgpu.Channel(ctx, streams, fading=tables)
        d_rx = torch.zeros((CL.N_OUT, 2), dtype=torch.float32, device="cuda")
        ch.apply(self.d_iq, F * dabgpu.NB_FRAME_SAMPLES, CL.N_OUT, d_rx)
        torch.cuda.synchronize()
        ch.close()
        slices = CL.slices_of(d_rx.cpu().numpy().view(np.complex64).reshape(-1))
        sdt, rdt = np.dtype(dabgpu.SYNC_STATE_DTYPE), np.dtype(dabgpu.RESULT_DTYPE)
        d_st = torch.zeros(sdt.itemsize, dtype=torch.uint8, device="cuda")
        hist = torch.zeros((1, H, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
        d_fib = torch.zeros((1, 4, 96), dtype=torch.uint8, device="cuda"); fres = torch.zeros((4, 16), dtype=torch.uint8, device="cuda")
        msc = torch.zeros((1, 4, nb), dtype=torch.uint8, device="cuda"); mres = torch.zeros((4 * len(self.gsubs), 16), dtype=torch.uint8, device="cuda")
        cifs = self.pay.reshape(4 * F, nb)[:, :self.n0]
        soft = dabgpu.SoftCfg(policy, SL.LEVEL)
        crc = wrong = lost = 0
        for j in range(F):
            d_slice = torch.from_numpy(np.ascontiguousarray(slices[j:j + 1]).view(np.float32)).cuda()
            if policy == dabgpu.SOFT_NORMALISED:
                ctx.ofdm_sync_demod_frames(d_slice, 1, CL.STRIDE, CL.P, d_st, hist[:, j % H], bits_frame_stride=H * dabgpu.NB_FRAME_BITS)
            else:
                ctx.ofdm_sync_demod_frames_soft(d_slice, 1, CL.STRIDE, CL.P, d_st, hist[:, j % H], soft, bits_frame_stride=H * dabgpu.NB_FRAME_BITS)
            ctx.decode_frames(hist, 1, H * dabgpu.NB_FRAME_BITS, H, j % H, self.gsubs, d_fib, fres, msc, 4 * nb, mres)
            torch.cuda.synchronize()
            lost += int(d_st.cpu().numpy().view(sdt)[0]["sync_valid"] == 0)
            crc += int(sum(bin(int(m)).count("1") for m in fres.cpu().numpy().view(rdt)["crc_ok_mask"].reshape(-1)))
            got = msc.cpu().numpy()[0][:, :self.n0]
            for c in range(4):
                if 4 * j + c >= 15:
                    wrong += int((got[c] != cifs[4 * j + c - 15]).sum())
        return crc, wrong, lost


@pytest.fixture(scope="module")
def chain(oracle):
    c = Chain(oracle)
    yield c
    c.close()


@pytest.mark.parametrize("snr_db,seed", SL.POINTS)
def test_weighted_soft_bits_deliver_on_the_device_where_the_reference_policy_does_not(chain, snr_db, seed):
    dabgpu = chain.dabgpu
    norm = chain.point(snr_db, seed, dabgpu.SOFT_NORMALISED)
    csi = chain.point(snr_db, seed, dabgpu.SOFT_CSI)
    print(f"{snr_db} dB, fading seed {seed}: normalised {norm}, weighted {csi} (FIB CRCs of 60, wrong bytes, frames without sync)")
    assert norm[:2] != (12 * CL.N_FRAMES, 0)
    assert csi == (12 * CL.N_FRAMES, 0, 0)
