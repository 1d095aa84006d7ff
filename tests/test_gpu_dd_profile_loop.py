"""-m gpu: the closed loop of tests/dd_profile_loop.py on the device: TxBank -> the channel bank (the static two-path channel of
tests/channel_loop.py, branch A's noise seed) -> the gated interferer added to the received stream (made on the host by the CPU loop's own
functions, so that both loops hear the same samples) -> dabgpu_ofdm_sync_demod_frames_branch -> dabgpu_noise_profile_frames on the slice
and dabgpu_dd_profile_frames on the products that call just wrote, each state carried from frame to frame in place, each weight array
straight into the banded combiner's table -> dabgpu_diversity_combine_frames (plain) and _banded into history rings ->
dabgpu_decode_frames_layout.  At every point of tests/test_dd_profile_closed_loop.py the counts (FIB CRCs of 60, wrong bytes of the EEP 3-A
sub-channel) equal the CPU loop's, the decision-directed weights equal the host model over the device's own products as bit patterns, and
the soft bits of the decision-directed path equal the CPU loop's."""
import numpy as np
import pytest

import channel_loop as CL
import channel_model as CM
import dd_profile_loop as DL
import dd_profile_model as DD
import noise_loop as NL
import tx_encode_cases as T

pytestmark = pytest.mark.gpu

RINGS = ("plain", "null", "dd", "dd25")
ALPHA = {"null": 1.0, "dd": 1.0, "dd25": 0.25}


class Chain:
    """the transmission on the device, once; a point = (SNR, I / S, gated) through channel, interferer, receiver, profiles, combiner, decoders"""

    def __init__(self, oracle, cpu_loop):
        import dabgpu
        import torch
        self.dabgpu, self.torch, self.cpu = dabgpu, torch, cpu_loop
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
        self._clean = {}

    def close(self):
        self.ctx.close()

    def stream(self, snr_db, is_db, gated):
        dabgpu, torch = self.dabgpu, self.torch
        if snr_db not in self._clean:
            p = CL.params(self.iq, snr_db)
            p["seed"] = NL.NOISE_SEED["A"]
            d_rx = torch.zeros((1, CL.N_OUT, 2), dtype=torch.float32, device="cuda")
            ch = dabgpu.Channel(self.ctx, [CM.to_struct(p, dabgpu.ChannelStream)])
            ch.apply(self.d_iq, CL.N_FRAMES * dabgpu.NB_FRAME_SAMPLES, CL.N_OUT, d_rx)
            torch.cuda.synchronize()
            ch.close()
            self._clean[snr_db] = d_rx.cpu().numpy().view(np.complex64).reshape(-1)
        rx = self._clean[snr_db]
        return rx if is_db is None else (rx + self.cpu.jam(rx.size, is_db, gated)).astype(np.complex64)

    def point(self, snr_db, is_db, gated=True):
        """-> (counts {ring: (FIB CRCs of 60, wrong bytes)}, frames the synchroniser refused, dd weights {ring: [5][128]}, products [5][75][1536],
        soft bits {ring: [5][230400]})"""
        dabgpu, torch, ctx = self.dabgpu, self.torch, self.ctx
        F, nb, H, NB = CL.N_FRAMES, self.nb, 8, dabgpu.NB_FRAME_BITS
        slices = NL.slices_of(self.stream(snr_db, is_db, gated))
        sdt, rdt = np.dtype(dabgpu.SYNC_STATE_DTYPE), np.dtype(dabgpu.RESULT_DTYPE)
        soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, DL.LEVEL)
        d_st = torch.zeros(sdt.itemsize, dtype=torch.uint8, device="cuda")
        dq = torch.zeros((1, 75, 1536, 2), dtype=torch.float32, device="cuda")
        scale = torch.zeros((1,), dtype=torch.float32, device="cuda")
        state = {r: torch.zeros((1, 128), dtype=torch.float32, device="cuda") for r in RINGS[1:]}
        bw = {r: torch.zeros((1, 128), dtype=torch.float32, device="cuda") for r in RINGS[1:]}
        own = torch.zeros((1, NB), dtype=torch.int8, device="cuda")
        hist = {r: torch.zeros((1, H, NB), dtype=torch.int8, device="cuda") for r in RINGS}
        d_fib = torch.zeros((1, 4, 96), dtype=torch.uint8, device="cuda"); fres = torch.zeros((4, 16), dtype=torch.uint8, device="cuda")
        msc = torch.zeros((1, 4, nb), dtype=torch.uint8, device="cuda"); mres = torch.zeros((4 * len(self.gsubs), 16), dtype=torch.uint8, device="cuda")
        cifs = self.pay.reshape(4 * F, nb)[:, :self.n0]
        crc, wrong, lost = {r: 0 for r in RINGS}, {r: 0 for r in RINGS}, 0
        weights = {r: np.zeros((F, 128), np.float32) for r in RINGS[1:]}
        products = np.zeros((F, 75, 1536), np.complex64)
        bits = {r: np.zeros((F, NB), np.int8) for r in RINGS}
        for j in range(F):
            d_slice = torch.from_numpy(np.ascontiguousarray(slices[j:j + 1]).view(np.float32)).cuda()
            ctx.ofdm_sync_demod_frames_branch(d_slice, 1, DL.STRIDE, DL.P, d_st, own, soft, dq, soft_scale=scale)
            ctx.noise_profile(d_slice, 1, DL.STRIDE, DL.P - 2656, states=d_st, profile_in=state["null"], alpha=ALPHA["null"], profile_out=state["null"],
                              band_weight=bw["null"])
            for r in ("dd", "dd25"):
                ctx.dd_profile(dq, 1, sync=d_st, profile_in=state[r], alpha=ALPHA[r], profile_out=state[r], band_weight=bw[r])
            table = [(dq, scale, None, d_st)]
            ctx.diversity_combine(table, 1, hist["plain"][:, j % H], bits_frame_stride=H * NB)
            for r in RINGS[1:]:
                ctx.diversity_combine(table, 1, hist[r][:, j % H], bits_frame_stride=H * NB, band_weights=[bw[r]])
            torch.cuda.synchronize()
            lost += int(d_st.cpu().numpy().view(sdt)[0]["sync_valid"] == 0)
            products[j] = dq.cpu().numpy().view(np.complex64).reshape(75, 1536)
            for r in RINGS[1:]:
                weights[r][j] = bw[r].cpu().numpy()[0]
            for r in RINGS:
                bits[r][j] = hist[r][0, j % H].cpu().numpy()
                ctx.decode_frames(hist[r], 1, H * NB, H, j % H, self.gsubs, d_fib, fres, msc, 4 * nb, mres)
                torch.cuda.synchronize()
                crc[r] += int(sum(bin(int(m)).count("1") for m in fres.cpu().numpy().view(rdt)["crc_ok_mask"].reshape(-1)))
                got = msc.cpu().numpy()[0][:, :self.n0]
                for c in range(4):
                    if 4 * j + c >= 15:
                        wrong[r] += int((got[c] != cifs[4 * j + c - 15]).sum())
        return {r: (crc[r], wrong[r]) for r in RINGS}, lost, weights, products, bits


@pytest.fixture(scope="module")
def cpu_loop(oracle, tmp_path_factory):
    return DL.Loop(oracle, tmp_path_factory.mktemp("dd_profile_loop"))


@pytest.fixture(scope="module")
def chain(oracle, cpu_loop):
    c = Chain(oracle, cpu_loop)
    yield c
    c.close()


def check_point(chain, cpu_loop, snr_db, is_db, gated):
    counts, lost, weights, products, bits = chain.point(snr_db, is_db, gated)
    cpu = {"plain": cpu_loop.count(cpu_loop.bits(snr_db, is_db, gated, "plain")), "null": cpu_loop.count(cpu_loop.bits(snr_db, is_db, gated, "null", 1.0)),
           "dd": cpu_loop.count(cpu_loop.bits(snr_db, is_db, gated, "dd", 1.0)), "dd25": cpu_loop.count(cpu_loop.bits(snr_db, is_db, gated, "dd", 0.25))}
    print(f"SNR {snr_db} dB, I / S {is_db} dB, {'gated' if gated else 'ungated'}: device {counts}, CPU {cpu}, frames without sync {lost}")
    assert lost == 0
    branch = cpu_loop.branch(snr_db, is_db, gated)
    same_products = np.array_equal(products.view(np.uint32), branch["dq"].view(np.uint32))
    for r in ("dd", "dd25"):                                                       # the weights themselves, bit for bit, from the device's own products
        b = dict(dq=products, valid=np.ones(CL.N_FRAMES, np.int32))
        want = DL.dd_weights(cpu_loop.dd_model, b, (ALPHA[r],))[ALPHA[r]]
        assert np.array_equal(weights[r].view(np.uint32), want.view(np.uint32)), r
        cpu_bits = np.stack(cpu_loop.bits(snr_db, is_db, gated, "dd", ALPHA[r]))
        assert np.array_equal(bits[r], cpu_bits), (r, "products equal the CPU loop's" if same_products else "products differ from the CPU loop's",
                                                   int((bits[r] != cpu_bits).sum()))
    assert counts == cpu
    return counts


@pytest.mark.parametrize("snr_db,is_db", DL.POINTS)
def test_device_loop_under_a_gated_interferer(chain, cpu_loop, snr_db, is_db):
    counts = check_point(chain, cpu_loop, snr_db, is_db, True)
    assert counts["dd"] == DL.DELIVERED and counts["dd25"] == DL.DELIVERED
    for r in ("plain", "null"):
        assert counts[r][0] <= DL.FAIL_CAP and counts[r][1] > 0


def test_device_loop_ungated_and_without_an_interferer(chain, cpu_loop):
    counts = check_point(chain, cpu_loop, *DL.UNGATED, False)
    assert counts["null"] == counts["dd"] == counts["dd25"] == DL.DELIVERED and counts["plain"][0] <= DL.FAIL_CAP
    counts = check_point(chain, cpu_loop, DL.CLEAN_SNR_DB, None, True)
    assert all(counts[r] == DL.DELIVERED for r in RINGS)
