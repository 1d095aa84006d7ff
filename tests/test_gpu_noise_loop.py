"""-m gpu: the closed loop of tests/noise_loop.py on the device: TxBank -> one channel bank per branch (the static two-path channel of
tests/channel_loop.py, a noise seed of its own, branch B 9 dB noisier) -> dabgpu_ofdm_sync_demod_frames_branch per branch ->
dabgpu_noise_estimate_frames on the same slice and records, its weight array straight into the branch table ->
dabgpu_diversity_combine_frames, once with unit and once with the estimated weights, into two history rings ->
dabgpu_decode_frames_layout.  One ensemble, five frames, at the operating point of tests/test_noise_closed_loop.py and 1 dB either
side.  The counts (FIB CRCs of 60, wrong bytes of the EEP 3-A sub-channel) equal the CPU loop's cell for cell, unit and estimated:
estimated weights deliver everything where unit weights lose most of it."""
import numpy as np
import pytest

import channel_loop as CL
import channel_model as CM
import noise_loop as NL
import tx_encode_cases as T

pytestmark = pytest.mark.gpu


class Chain:
    """the transmission on the device, once; a point = the SNR of branch A through channels, receivers, estimator, combiner, decoders"""

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

    def close(self):
        self.ctx.close()

    def point(self, snr_db):
        """-> ((FIB CRCs of 60, wrong bytes) with unit weights, the same with estimated weights, frames a synchroniser refused, weights [5][2])"""
        dabgpu, torch, ctx = self.dabgpu, self.torch, self.ctx
        F, nb, H, K, NB = CL.N_FRAMES, self.nb, 8, 2, dabgpu.NB_FRAME_BITS
        d_rx = torch.zeros((K, CL.N_OUT, 2), dtype=torch.float32, device="cuda")
        for b, name in enumerate(("A", "B")):
            ch = dabgpu.Channel(ctx, [CM.to_struct(NL.params(self.iq, snr_db, name), dabgpu.ChannelStream)])
            ch.apply(self.d_iq, F * dabgpu.NB_FRAME_SAMPLES, CL.N_OUT, d_rx[b:b + 1])
            torch.cuda.synchronize()
            ch.close()
        rx = d_rx.cpu().numpy().view(np.complex64).reshape(K, -1)
        slices = [NL.slices_of(rx[b]) for b in range(K)]
        sdt, rdt = np.dtype(dabgpu.SYNC_STATE_DTYPE), np.dtype(dabgpu.RESULT_DTYPE)
        soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, NL.LEVEL)
        d_st = [torch.zeros(sdt.itemsize, dtype=torch.uint8, device="cuda") for _ in range(K)]
        dq = [torch.zeros((1, 75, 1536, 2), dtype=torch.float32, device="cuda") for _ in range(K)]
        scale = [torch.zeros((1,), dtype=torch.float32, device="cuda") for _ in range(K)]
        w = [torch.zeros((1,), dtype=torch.float32, device="cuda") for _ in range(K)]
        own = torch.zeros((1, NB), dtype=torch.int8, device="cuda")
        hist = [torch.zeros((1, H, NB), dtype=torch.int8, device="cuda") for _ in range(2)]              # unit weights, estimated weights
        d_fib = torch.zeros((1, 4, 96), dtype=torch.uint8, device="cuda"); fres = torch.zeros((4, 16), dtype=torch.uint8, device="cuda")
        msc = torch.zeros((1, 4, nb), dtype=torch.uint8, device="cuda"); mres = torch.zeros((4 * len(self.gsubs), 16), dtype=torch.uint8, device="cuda")
        cifs = self.pay.reshape(4 * F, nb)[:, :self.n0]
        crc, wrong, lost, weights = [0, 0], [0, 0], 0, np.zeros((F, K), np.float32)
        for j in range(F):
            for b in range(K):
                d_slice = torch.from_numpy(np.ascontiguousarray(slices[b][j:j + 1]).view(np.float32)).cuda()
                ctx.ofdm_sync_demod_frames_branch(d_slice, 1, NL.STRIDE, NL.P, d_st[b], own, soft, dq[b], soft_scale=scale[b])
                ctx.noise_estimate(d_slice, 1, NL.STRIDE, NL.P - 2656, states=d_st[b], weight=w[b])
            ctx.diversity_combine([(dq[b], scale[b], None, d_st[b]) for b in range(K)], 1, hist[0][:, j % H], bits_frame_stride=H * NB)
            ctx.diversity_combine([(dq[b], scale[b], w[b], d_st[b]) for b in range(K)], 1, hist[1][:, j % H], bits_frame_stride=H * NB)
            torch.cuda.synchronize()
            lost += int(sum(t.cpu().numpy().view(sdt)[0]["sync_valid"] == 0 for t in d_st))
            weights[j] = [float(t.cpu().numpy()[0]) for t in w]
            for r in range(2):
                ctx.decode_frames(hist[r], 1, H * NB, H, j % H, self.gsubs, d_fib, fres, msc, 4 * nb, mres)
                torch.cuda.synchronize()
                crc[r] += int(sum(bin(int(m)).count("1") for m in fres.cpu().numpy().view(rdt)["crc_ok_mask"].reshape(-1)))
                got = msc.cpu().numpy()[0][:, :self.n0]
                for c in range(4):
                    if 4 * j + c >= 15:
                        wrong[r] += int((got[c] != cifs[4 * j + c - 15]).sum())
        return (crc[0], wrong[0]), (crc[1], wrong[1]), lost, weights


@pytest.fixture(scope="module")
def chain(oracle):
    c = Chain(oracle)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cpu_loop(oracle, tmp_path_factory):
    return NL.Loop(oracle, tmp_path_factory.mktemp("noise_loop"))


@pytest.mark.parametrize("snr_db", [NL.POINT_DB - 1.0, NL.POINT_DB, NL.POINT_DB + 1.0])
def test_device_loop_equals_the_cpu_loop(chain, cpu_loop, snr_db):
    unit, est, lost, weights = chain.point(snr_db)
    cpu_unit, cpu_est = cpu_loop.pair(snr_db, "unit"), cpu_loop.pair(snr_db, "estimated")
    print(f"{snr_db} dB: unit {unit} (CPU {cpu_unit}), estimated {est} (CPU {cpu_est}), frames without sync {lost}, weights {weights.tolist()}")
    assert lost == 0
    cpu_w = np.stack([cpu_loop.branch(snr_db, n)["w"] for n in ("A", "B")], axis=1)
    assert np.array_equal(weights.view(np.uint32), cpu_w.view(np.uint32))          # the weights themselves, bit for bit
    assert unit == cpu_unit and est == cpu_est
    assert est == NL.DELIVERED and unit != NL.DELIVERED
