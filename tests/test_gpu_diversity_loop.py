"""-m gpu: the closed loop of tests/diversity_loop.py on the device: TxBank -> one fading bank per branch (`tu6`, six Rayleigh
taps at 10 Hz, +37 samples, no carrier offset, a fading seed and a noise seed of its own) -> dabgpu_ofdm_sync_demod_frames_branch per
branch (synchroniser, weighted soft bits at level 64, DQPSK products, scale) -> dabgpu_diversity_combine_frames over the branches'
products, scales and sync records straight into the history ring -> dabgpu_decode_frames_layout; one ensemble, five frames, at the two
points of tests/test_diversity_closed_loop.py.  The rule is the CPU test's: each branch's own soft bits do not deliver (fewer than 60
FIB CRCs or a wrong byte in the EEP 3-A sub-channel's five delivered logical frames), the combination delivers everything, and the
synchroniser refuses no frame of either branch.  Measured on an MI355X (FIB CRCs of 60 / wrong bytes; single branches, then combinations):

    SNR dB  seed 1    seed 7    seed 3    seed 6    1+7     3+6    1+3     7+6    all four
       5    36/667    14/591    40/111    48/167    54/2    60/0   60/0    48/0   60/0
       6    36/454    19/279    49/21     48/54     59/0    60/0   60/0    51/0   60/0
       7    37/266    23/125    56/5      48/16     60/0    60/0   60/0    57/0   60/0

Every cell equals the CPU table of tests/test_diversity_closed_loop.py (the device's synchroniser, demodulator and fading bank equal their
host models bit for bit, and a bank of ONE stream per branch gives a branch the realisation the CPU loop gives it; as stream 1 of a common
bank the same seeds draw another realisation).  No frame of the grid was refused by a synchroniser.  Both points of the CPU test carry over
unchanged: 6 dB with the branches (3, 6): alone 49/21 and 48/54, together 60/0; with (1, 3): alone 36/454 and 49/21, together 60/0."""
import numpy as np
import pytest

import channel_fading_loop as FL
import channel_loop as CL
import channel_model as CM
import diversity_loop as DL
import tx_encode_cases as T

pytestmark = pytest.mark.gpu


class Chain:
    """the transmission on the device, once; a point = (SNR, the branches' fading seeds) through channels, receivers, combiner, decoders"""

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

    def point(self, snr_db, seeds):
        """-> (per branch (FIB CRCs of 60, wrong bytes) of its own soft bits, the same of the combination, frames a synchroniser refused)"""
        dabgpu, torch, ctx = self.dabgpu, self.torch, self.ctx
        F, nb, H, K, NB = CL.N_FRAMES, self.nb, 8, len(seeds), dabgpu.NB_FRAME_BITS
        # a fading bank of one stream per branch: the realisation of a branch is then the one the CPU loop's host model gives it
        d_rx = torch.zeros((K, CL.N_OUT, 2), dtype=torch.float32, device="cuda")
        for b, s in enumerate(seeds):
            streams = [CM.to_struct(DL.params(self.iq, snr_db, s), dabgpu.ChannelStream)]
            tables = dabgpu.channel_fading_plan(streams, [dabgpu.channel_fading_spec(FL.DOPPLER_CYCLES, s, self.prof["kinds"], self.prof["rice_k"],
                                                                                      self.prof["los_cos"])])
            ch = dabgpu.Channel(ctx, streams, fading=tables)
            ch.apply(self.d_iq, F * dabgpu.NB_FRAME_SAMPLES, CL.N_OUT, d_rx[b:b + 1])
            torch.cuda.synchronize()
            ch.close()
        rx = d_rx.cpu().numpy().view(np.complex64).reshape(K, -1)
        slices = [CL.slices_of(rx[b]) for b in range(K)]
        sdt, rdt = np.dtype(dabgpu.SYNC_STATE_DTYPE), np.dtype(dabgpu.RESULT_DTYPE)
        soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, DL.LEVEL)
        d_st = [torch.zeros(sdt.itemsize, dtype=torch.uint8, device="cuda") for _ in range(K)]
        dq = [torch.zeros((1, 75, 1536, 2), dtype=torch.float32, device="cuda") for _ in range(K)]
        scale = [torch.zeros((1,), dtype=torch.float32, device="cuda") for _ in range(K)]
        hist = [torch.zeros((1, H, NB), dtype=torch.int8, device="cuda") for _ in range(K + 1)]           # one ring per branch, the last the combination's
        d_fib = torch.zeros((1, 4, 96), dtype=torch.uint8, device="cuda"); fres = torch.zeros((4, 16), dtype=torch.uint8, device="cuda")
        msc = torch.zeros((1, 4, nb), dtype=torch.uint8, device="cuda"); mres = torch.zeros((4 * len(self.gsubs), 16), dtype=torch.uint8, device="cuda")
        cifs = self.pay.reshape(4 * F, nb)[:, :self.n0]
        crc, wrong, lost = [0] * (K + 1), [0] * (K + 1), 0
        for j in range(F):
            for b in range(K):
                d_slice = torch.from_numpy(np.ascontiguousarray(slices[b][j:j + 1]).view(np.float32)).cuda()
                hist[b][:, j % H].zero_()                                # a refused frame leaves the slot alone: an erasure, not a stale frame
                ctx.ofdm_sync_demod_frames_branch(d_slice, 1, CL.STRIDE, CL.P, d_st[b], hist[b][:, j % H], soft, dq[b], bits_frame_stride=H * NB,
                                                  soft_scale=scale[b])
            ctx.diversity_combine([(dq[b], scale[b], None, d_st[b]) for b in range(K)], 1, hist[K][:, j % H], bits_frame_stride=H * NB)
            torch.cuda.synchronize()
            lost += int(sum(t.cpu().numpy().view(sdt)[0]["sync_valid"] == 0 for t in d_st))
            for r in range(K + 1):
                ctx.decode_frames(hist[r], 1, H * NB, H, j % H, self.gsubs, d_fib, fres, msc, 4 * nb, mres)
                torch.cuda.synchronize()
                crc[r] += int(sum(bin(int(m)).count("1") for m in fres.cpu().numpy().view(rdt)["crc_ok_mask"].reshape(-1)))
                got = msc.cpu().numpy()[0][:, :self.n0]
                for c in range(4):
                    if 4 * j + c >= 15:
                        wrong[r] += int((got[c] != cifs[4 * j + c - 15]).sum())
        return [(crc[b], wrong[b]) for b in range(K)], (crc[K], wrong[K]), lost


@pytest.fixture(scope="module")
def chain(oracle):
    c = Chain(oracle)
    yield c
    c.close()


@pytest.mark.parametrize("snr_db,seeds", DL.POINTS)
def test_two_branches_deliver_on_the_device_where_neither_does_alone(chain, snr_db, seeds):
    singles, pair, lost = chain.point(snr_db, seeds)
    print(f"{snr_db} dB, branches {seeds}: alone {singles}, together {pair} (FIB CRCs of 60, wrong bytes), frames without sync {lost}")
    for s in singles:
        assert s != DL.DELIVERED
    assert pair == DL.DELIVERED
    assert lost == 0
