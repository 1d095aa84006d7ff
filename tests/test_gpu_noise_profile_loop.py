"""-m gpu: the closed loop of tests/noise_profile_loop.py on the device: TxBank -> the channel bank (the static two-path channel of
tests/channel_loop.py at 9 dB, a noise seed per branch) -> the branch's interferer added to the received stream (made on the host by
the CPU loop's own function, so that both loops hear the same samples) -> dabgpu_ofdm_sync_demod_frames_branch ->
dabgpu_noise_profile_frames on the same slice and records, its state carried from frame to frame in place, its weight array straight
into the banded combiner's table -> dabgpu_diversity_combine_frames (plain) and _banded (both alphas) into history rings ->
dabgpu_decode_frames_layout.  One ensemble, five frames, at the operating point of tests/test_noise_profile_closed_loop.py and 3 dB
either side: the counts (FIB CRCs of 60, wrong bytes of the EEP 3-A sub-channel) equal the CPU loop's cell for cell and the band weights
its weights as bit patterns.  Two branches, each with an interferer of its own elsewhere in the block: each alone and their unit-weight
sum fail, the banded pair delivers."""
import numpy as np
import pytest

import channel_loop as CL
import channel_model as CM
import noise_loop as NL
import noise_profile_loop as PL
import tx_encode_cases as T

pytestmark = pytest.mark.gpu


class Chain:
    """the transmission on the device, once; a point = I / S through channel, interferer, receivers, profile, combiner, decoders"""

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
        self._clean = {}

    def close(self):
        self.ctx.close()

    def stream(self, is_db, name):
        dabgpu, torch = self.dabgpu, self.torch
        if name not in self._clean:
            p = CL.params(self.iq, PL.SNR_DB)
            p["seed"] = NL.NOISE_SEED[name]
            d_rx = torch.zeros((1, CL.N_OUT, 2), dtype=torch.float32, device="cuda")
            ch = dabgpu.Channel(self.ctx, [CM.to_struct(p, dabgpu.ChannelStream)])
            ch.apply(self.d_iq, CL.N_FRAMES * dabgpu.NB_FRAME_SAMPLES, CL.N_OUT, d_rx)
            torch.cuda.synchronize()
            ch.close()
            self._clean[name] = d_rx.cpu().numpy().view(np.complex64).reshape(-1)
        rx = self._clean[name]
        jam = PL.interferer(rx.size, PL.OFFSET[name], PL.WIDTH, self.S * 10.0 ** (is_db / 10.0), PL.JAM_SEED[name])
        return (rx + jam).astype(np.complex64)

    def point(self, is_db, names=("A",), alphas=PL.ALPHAS):
        """-> (counts {"plain": .., alpha: ..} as (FIB CRCs of 60, wrong bytes), frames a synchroniser refused, band weights {alpha: [5][K][128]})"""
        dabgpu, torch, ctx = self.dabgpu, self.torch, self.ctx
        F, nb, H, K, NB = CL.N_FRAMES, self.nb, 8, len(names), dabgpu.NB_FRAME_BITS
        slices = [NL.slices_of(self.stream(is_db, n)) for n in names]
        sdt, rdt = np.dtype(dabgpu.SYNC_STATE_DTYPE), np.dtype(dabgpu.RESULT_DTYPE)
        soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, PL.LEVEL)
        d_st = [torch.zeros(sdt.itemsize, dtype=torch.uint8, device="cuda") for _ in range(K)]
        dq = [torch.zeros((1, 75, 1536, 2), dtype=torch.float32, device="cuda") for _ in range(K)]
        scale = [torch.zeros((1,), dtype=torch.float32, device="cuda") for _ in range(K)]
        state = {a: [torch.zeros((1, 128), dtype=torch.float32, device="cuda") for _ in range(K)] for a in alphas}
        bw = {a: [torch.zeros((1, 128), dtype=torch.float32, device="cuda") for _ in range(K)] for a in alphas}
        own = torch.zeros((1, NB), dtype=torch.int8, device="cuda")
        rings = ["plain"] + list(alphas)
        hist = {r: torch.zeros((1, H, NB), dtype=torch.int8, device="cuda") for r in rings}
        d_fib = torch.zeros((1, 4, 96), dtype=torch.uint8, device="cuda"); fres = torch.zeros((4, 16), dtype=torch.uint8, device="cuda")
        msc = torch.zeros((1, 4, nb), dtype=torch.uint8, device="cuda"); mres = torch.zeros((4 * len(self.gsubs), 16), dtype=torch.uint8, device="cuda")
        cifs = self.pay.reshape(4 * F, nb)[:, :self.n0]
        crc, wrong, lost = {r: 0 for r in rings}, {r: 0 for r in rings}, 0
        weights = {a: np.zeros((F, K, 128), np.float32) for a in alphas}
        for j in range(F):
            for b in range(K):
                d_slice = torch.from_numpy(np.ascontiguousarray(slices[b][j:j + 1]).view(np.float32)).cuda()
                ctx.ofdm_sync_demod_frames_branch(d_slice, 1, PL.STRIDE, PL.P, d_st[b], own, soft, dq[b], soft_scale=scale[b])
                for a in alphas:
                    ctx.noise_profile(d_slice, 1, PL.STRIDE, PL.P - 2656, states=d_st[b], profile_in=state[a][b], alpha=a, profile_out=state[a][b],
                                      band_weight=bw[a][b])
            table = [(dq[b], scale[b], None, d_st[b]) for b in range(K)]
            ctx.diversity_combine(table, 1, hist["plain"][:, j % H], bits_frame_stride=H * NB)
            for a in alphas:
                ctx.diversity_combine(table, 1, hist[a][:, j % H], bits_frame_stride=H * NB, band_weights=bw[a])
            torch.cuda.synchronize()
            lost += int(sum(t.cpu().numpy().view(sdt)[0]["sync_valid"] == 0 for t in d_st))
            for a in alphas:
                weights[a][j] = np.stack([t.cpu().numpy()[0] for t in bw[a]])
            for r in rings:
                ctx.decode_frames(hist[r], 1, H * NB, H, j % H, self.gsubs, d_fib, fres, msc, 4 * nb, mres)
                torch.cuda.synchronize()
                crc[r] += int(sum(bin(int(m)).count("1") for m in fres.cpu().numpy().view(rdt)["crc_ok_mask"].reshape(-1)))
                got = msc.cpu().numpy()[0][:, :self.n0]
                for c in range(4):
                    if 4 * j + c >= 15:
                        wrong[r] += int((got[c] != cifs[4 * j + c - 15]).sum())
        return {r: (crc[r], wrong[r]) for r in rings}, lost, weights


@pytest.fixture(scope="module")
def chain(oracle):
    c = Chain(oracle)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cpu_loop(oracle, tmp_path_factory):
    return PL.Loop(oracle, tmp_path_factory.mktemp("noise_profile_loop"))


@pytest.mark.parametrize("is_db", [PL.POINT_DB - 3.0, PL.POINT_DB, PL.POINT_DB + 3.0])
def test_device_loop_equals_the_cpu_loop(chain, cpu_loop, is_db):
    counts, lost, weights = chain.point(is_db)
    cpu = {"plain": cpu_loop.plain(is_db)}
    cpu.update({a: cpu_loop.banded(is_db, alpha=a) for a in PL.ALPHAS})
    print(f"I / S {is_db} dB: device {counts}, CPU {cpu}, frames without sync {lost}")
    assert lost == 0
    for a in PL.ALPHAS:                                                            # the weights themselves, bit for bit
        assert np.array_equal(weights[a][:, 0].view(np.uint32), cpu_loop.branch(is_db, "A")["w"][a].view(np.uint32)), a
    assert counts == cpu
    for a in PL.ALPHAS:
        assert counts[a] == PL.DELIVERED
    assert counts["plain"][0] < 12 * CL.N_FRAMES and counts["plain"][1] > 0


def test_two_branches_jammed_in_different_bands(chain, cpu_loop):
    is_db = PL.POINT_DB
    counts, lost, weights = chain.point(is_db, ("A", "B"), (1.0,))
    cpu = {"plain": cpu_loop.plain_pair(is_db), 1.0: cpu_loop.banded(is_db, ("A", "B"))}
    print(f"I / S {is_db} dB, two branches: device {counts}, CPU {cpu}")
    assert lost == 0 and counts == cpu
    for b, n in enumerate(("A", "B")):
        assert np.array_equal(weights[1.0][:, b].view(np.uint32), cpu_loop.branch(is_db, n)["w"][1.0].view(np.uint32)), n
        alone = cpu_loop.plain(is_db, n)
        assert alone[0] < 12 * CL.N_FRAMES and alone[1] > 0                        # (each alone: the single-branch cells above, on the device too)
    assert counts[1.0] == PL.DELIVERED
    assert counts["plain"][0] < 12 * CL.N_FRAMES and counts["plain"][1] > 0
