"""-m gpu: the closed loop of tests/interferer_loop.py with every stage on the device: TxBank -> the channel bank (the static two-path
channel of tests/channel_loop.py with white noise) -> the interferer bank, in place on the received stream ->
dabgpu_ofdm_sync_demod_frames_branch -> dabgpu_noise_profile_frames, its state carried from frame to frame -> dabgpu_diversity_combine_frames
(plain) and with band_weights (both alphas) into history rings -> dabgpu_decode_frames_layout.  One ensemble, five frames, at the operating
point of tests/test_interferer_closed_loop.py and 3 dB either side of its I / S: the banded path delivers every FIB and byte, the plain
soft bits fewer than half the FIBs, the received stream equals the CPU chain's bit for bit and the counts its counts."""
import numpy as np
import pytest

import channel_loop as CL
import channel_model as CM
import interferer_loop as IL
import interferer_model as IM
import noise_loop as NL
import noise_profile_loop as PL
import tx_encode_cases as T

pytestmark = pytest.mark.gpu


class Chain:
    """the transmission on the device, once; a point = I / S through channel, interferer, receiver, profile, combiner, decoders"""

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
        self.S = PL.signal_power(self.iq)
        self.shape = dabgpu.interferer_design(IL.WIDTH_HZ / 2.048e6)

    def close(self):
        self.ctx.close()

    def stream(self, snr_db, is_db):
        dabgpu, torch = self.dabgpu, self.torch
        p = CL.params(self.iq, snr_db)
        p["seed"] = NL.NOISE_SEED["A"]
        d_rx = torch.zeros((1, CL.N_OUT, 2), dtype=torch.float32, device="cuda")
        ch = dabgpu.Channel(self.ctx, [CM.to_struct(p, dabgpu.ChannelStream)])
        ch.apply(self.d_iq, CL.N_FRAMES * dabgpu.NB_FRAME_SAMPLES, CL.N_OUT, d_rx)
        jam = dabgpu.Interferer(self.ctx, [IM.to_struct(IL.band_stream(self.S, is_db), dabgpu.InterfererStream)], [self.shape])
        jam.apply(d_rx, CL.N_OUT, d_rx, in_stride_samples=CL.N_OUT)                  # in place
        torch.cuda.synchronize()
        ch.close(); jam.close()
        return d_rx.cpu().numpy().view(np.complex64).reshape(-1)

    def point(self, rx, alphas=IL.ALPHAS):
        """-> (counts {"plain": .., alpha: ..} as (FIB CRCs of 60, wrong bytes), frames the synchroniser refused)"""
        dabgpu, torch, ctx = self.dabgpu, self.torch, self.ctx
        F, nb, H, NB = CL.N_FRAMES, self.nb, 8, dabgpu.NB_FRAME_BITS
        slices = NL.slices_of(rx)
        sdt, rdt = np.dtype(dabgpu.SYNC_STATE_DTYPE), np.dtype(dabgpu.RESULT_DTYPE)
        soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, PL.LEVEL)
        d_st = torch.zeros(sdt.itemsize, dtype=torch.uint8, device="cuda")
        dq = torch.zeros((1, 75, 1536, 2), dtype=torch.float32, device="cuda")
        scale = torch.zeros((1,), dtype=torch.float32, device="cuda")
        state = {a: torch.zeros((1, 128), dtype=torch.float32, device="cuda") for a in alphas}
        bw = {a: torch.zeros((1, 128), dtype=torch.float32, device="cuda") for a in alphas}
        own = torch.zeros((1, NB), dtype=torch.int8, device="cuda")
        rings = ["plain"] + list(alphas)
        hist = {r: torch.zeros((1, H, NB), dtype=torch.int8, device="cuda") for r in rings}
        d_fib = torch.zeros((1, 4, 96), dtype=torch.uint8, device="cuda"); fres = torch.zeros((4, 16), dtype=torch.uint8, device="cuda")
        msc = torch.zeros((1, 4, nb), dtype=torch.uint8, device="cuda"); mres = torch.zeros((4 * len(self.gsubs), 16), dtype=torch.uint8, device="cuda")
        cifs = self.pay.reshape(4 * F, nb)[:, :self.n0]
        crc, wrong, lost = {r: 0 for r in rings}, {r: 0 for r in rings}, 0
        for j in range(F):
            d_slice = torch.from_numpy(np.ascontiguousarray(slices[j:j + 1]).view(np.float32)).cuda()
            ctx.ofdm_sync_demod_frames_branch(d_slice, 1, PL.STRIDE, PL.P, d_st, own, soft, dq, soft_scale=scale)
            for a in alphas:
                ctx.noise_profile(d_slice, 1, PL.STRIDE, PL.P - 2656, states=d_st, profile_in=state[a], alpha=a, profile_out=state[a], band_weight=bw[a])
            table = [(dq, scale, None, d_st)]
            ctx.diversity_combine(table, 1, hist["plain"][:, j % H], bits_frame_stride=H * NB)
            for a in alphas:
                ctx.diversity_combine(table, 1, hist[a][:, j % H], bits_frame_stride=H * NB, band_weights=[bw[a]])
            torch.cuda.synchronize()
            lost += int(d_st.cpu().numpy().view(sdt)[0]["sync_valid"] == 0)
            for r in rings:
                ctx.decode_frames(hist[r], 1, H * NB, H, j % H, self.gsubs, d_fib, fres, msc, 4 * nb, mres)
                torch.cuda.synchronize()
                crc[r] += int(sum(bin(int(m)).count("1") for m in fres.cpu().numpy().view(rdt)["crc_ok_mask"].reshape(-1)))
                got = msc.cpu().numpy()[0][:, :self.n0]
                for c in range(4):
                    if 4 * j + c >= 15:
                        wrong[r] += int((got[c] != cifs[4 * j + c - 15]).sum())
        return {r: (crc[r], wrong[r]) for r in rings}, lost


@pytest.fixture(scope="module")
def chain(oracle):
    c = Chain(oracle)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cpu_loop(oracle, tmp_path_factory):
    return IL.Loop(oracle, tmp_path_factory.mktemp("interferer_loop"))


@pytest.mark.parametrize("is_db", [IL.POINT_DB - 3.0, IL.POINT_DB, IL.POINT_DB + 3.0])
def test_device_loop_equals_the_cpu_loop(chain, cpu_loop, is_db):
    rx = chain.stream(IL.SNR_DB, is_db)
    assert np.array_equal(rx.view(np.uint32), cpu_loop.stream(IL.SNR_DB, is_db).view(np.uint32)), "the received stream differs from the CPU chain's"
    counts, lost = chain.point(rx)
    cpu = {"plain": cpu_loop.plain(IL.SNR_DB, is_db)}
    cpu.update({a: cpu_loop.banded(IL.SNR_DB, is_db, a) for a in IL.ALPHAS})
    print(f"SNR {IL.SNR_DB} dB, I / S {is_db} dB: device {counts}, CPU {cpu}, frames without sync {lost}")
    assert lost == 0 and counts == cpu
    for a in IL.ALPHAS:
        assert counts[a] == IL.DELIVERED
    assert counts["plain"][0] < 6 * CL.N_FRAMES
