"""-m gpu: the closed loop of tests/sym_profile_loop.py on the device: TxBank -> the channel bank (the static two-path channel of
tests/channel_loop.py, branch A's noise seed) -> the gated white burst added to the received stream (made on the host by the CPU loop's
own function, so that both loops hear the same samples) -> dabgpu_ofdm_sync_demod_frames_branch -> dabgpu_dd_profile_frames and
dabgpu_sym_profile_frames on the products that call just wrote, each weight array straight into the combiner's tables ->
dabgpu_diversity_combine_frames (plain), _banded and _symbols (with and without the band table) into history rings ->
dabgpu_decode_frames_layout.  At every point of tests/test_sym_profile_closed_loop.py the counts (FIB CRCs of 60, wrong bytes of the
EEP 3-A sub-channel) equal the CPU loop's, the symbol weights and noise figures equal the host model over the device's own products as
bit patterns, and the soft bits of both symbol-weighted paths equal the CPU loop's."""
import numpy as np
import pytest

import channel_loop as CL
import channel_model as CM
import noise_loop as NL
import sym_profile_loop as L
import tx_encode_cases as T

pytestmark = pytest.mark.gpu

RINGS = L.PATHS                                        # plain, dd, plain+sym, dd+sym


class Chain:
    """the transmission on the device, once; a point = (SNR, I / S) through channel, burst, receiver, profiles, combiner, decoders"""

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

    def stream(self, snr_db, is_db):
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
        return rx if is_db is None else (rx + L.burst(rx.size, self.cpu.S * 10.0 ** (is_db / 10.0))).astype(np.complex64)

    def point(self, snr_db, is_db):
        """-> (counts {ring: (FIB CRCs of 60, wrong bytes)}, valid [5], v [5][75], q [5][75], sym_ok [5], products [5][75][1536],
        soft bits {ring: [5][230400]})"""
        dabgpu, torch, ctx = self.dabgpu, self.torch, self.ctx
        F, nb, H, NB = CL.N_FRAMES, self.nb, 8, dabgpu.NB_FRAME_BITS
        slices = NL.slices_of(self.stream(snr_db, is_db))
        sdt, rdt = np.dtype(dabgpu.SYNC_STATE_DTYPE), np.dtype(dabgpu.RESULT_DTYPE)
        soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, L.PL.LEVEL)
        d_st = torch.zeros(sdt.itemsize, dtype=torch.uint8, device="cuda")
        dq = torch.zeros((1, 75, 1536, 2), dtype=torch.float32, device="cuda")
        scale = torch.zeros((1,), dtype=torch.float32, device="cuda")
        state = torch.zeros((1, 128), dtype=torch.float32, device="cuda")
        bw = torch.zeros((1, 128), dtype=torch.float32, device="cuda")
        d_v = torch.zeros((1, 75), dtype=torch.float32, device="cuda")
        d_q = torch.zeros((1, 75), dtype=torch.float32, device="cuda")
        d_ok = torch.zeros((1,), dtype=torch.int32, device="cuda")
        own = torch.zeros((1, NB), dtype=torch.int8, device="cuda")
        hist = {r: torch.zeros((1, H, NB), dtype=torch.int8, device="cuda") for r in RINGS}
        d_fib = torch.zeros((1, 4, 96), dtype=torch.uint8, device="cuda"); fres = torch.zeros((4, 16), dtype=torch.uint8, device="cuda")
        msc = torch.zeros((1, 4, nb), dtype=torch.uint8, device="cuda"); mres = torch.zeros((4 * len(self.gsubs), 16), dtype=torch.uint8, device="cuda")
        cifs = self.pay.reshape(4 * F, nb)[:, :self.n0]
        crc, wrong = {r: 0 for r in RINGS}, {r: 0 for r in RINGS}
        valid, sym_ok = np.zeros(F, np.int32), np.zeros(F, np.int32)
        v, q = np.zeros((F, 75), np.float32), np.zeros((F, 75), np.float32)
        products = np.zeros((F, 75, 1536), np.complex64)
        bits = {r: np.zeros((F, NB), np.int8) for r in RINGS}
        for j in range(F):
            d_slice = torch.from_numpy(np.ascontiguousarray(slices[j:j + 1]).view(np.float32)).cuda()
            ctx.ofdm_sync_demod_frames_branch(d_slice, 1, L.PL.STRIDE, L.PL.P, d_st, own, soft, dq, soft_scale=scale)
            ctx.dd_profile(dq, 1, sync=d_st, profile_in=state, alpha=L.ALPHA, profile_out=state, band_weight=bw)
            ctx.sym_profile(dq, 1, sync=d_st, symbol_weight=d_v, symbol_noise=d_q, valid=d_ok)
            table = [(dq, scale, None, d_st)]
            ctx.diversity_combine(table, 1, hist["plain"][:, j % H], bits_frame_stride=H * NB)
            ctx.diversity_combine(table, 1, hist["dd"][:, j % H], bits_frame_stride=H * NB, band_weights=[bw])
            ctx.diversity_combine(table, 1, hist["plain+sym"][:, j % H], bits_frame_stride=H * NB, symbol_weights=[d_v])
            ctx.diversity_combine(table, 1, hist["dd+sym"][:, j % H], bits_frame_stride=H * NB, band_weights=[bw], symbol_weights=[d_v])
            torch.cuda.synchronize()
            valid[j] = int(d_st.cpu().numpy().view(sdt)[0]["sync_valid"])
            if not valid[j]:
                d_st.zero_()                                                             # acquisition starts over, as in the CPU loop's receiver
            sym_ok[j] = int(d_ok.cpu().numpy()[0])
            products[j] = dq.cpu().numpy().view(np.complex64).reshape(75, 1536)
            v[j], q[j] = d_v.cpu().numpy()[0], d_q.cpu().numpy()[0]
            for r in RINGS:
                bits[r][j] = hist[r][0, j % H].cpu().numpy()
                ctx.decode_frames(hist[r], 1, H * NB, H, j % H, self.gsubs, d_fib, fres, msc, 4 * nb, mres)
                torch.cuda.synchronize()
                crc[r] += int(sum(bin(int(m)).count("1") for m in fres.cpu().numpy().view(rdt)["crc_ok_mask"].reshape(-1)))
                got = msc.cpu().numpy()[0][:, :self.n0]
                for c in range(4):
                    if 4 * j + c >= 15:
                        wrong[r] += int((got[c] != cifs[4 * j + c - 15]).sum())
        return {r: (crc[r], wrong[r]) for r in RINGS}, valid, v, q, sym_ok, products, bits


@pytest.fixture(scope="module")
def cpu_loop(oracle, tmp_path_factory):
    return L.Loop(oracle, tmp_path_factory.mktemp("sym_profile_loop"))


@pytest.fixture(scope="module")
def chain(oracle, cpu_loop):
    c = Chain(oracle, cpu_loop)
    yield c
    c.close()


def check_point(chain, cpu_loop, snr_db, is_db, against_cpu=True):
    counts, valid, v, q, sym_ok, products, bits = chain.point(snr_db, is_db)
    cpu = cpu_loop.counts(snr_db, is_db)
    branch = cpu_loop.branch(snr_db, is_db)
    print(f"SNR {snr_db} dB, I / S {is_db} dB: device {counts}, CPU {cpu}, valid {valid.tolist()}, smallest weight {v[valid == 1].min():.4f}")
    if against_cpu:
        assert np.array_equal(valid, branch["valid"])
    same_products = np.array_equal(products[valid == 1].view(np.uint32), branch["dq"][valid == 1].view(np.uint32))
    # the weights themselves, bit for bit, from the device's own products; a refused frame's are zeros
    want = L.symbol_weights(cpu_loop.sym_model, dict(dq=products, valid=valid))
    assert np.array_equal(v.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(q.view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(sym_ok, want[2])
    if not against_cpu:
        return counts, valid, v
    for r in ("plain+sym", "dd+sym"):
        cpu_bits = np.stack(cpu_loop.bits(snr_db, is_db, r))
        for j in np.nonzero(valid)[0]:                                                 # (a refused frame's ring slot holds the erasure the combiner wrote)
            assert np.array_equal(bits[r][j], cpu_bits[j]), (r, j, "products equal the CPU loop's" if same_products else "products differ from the CPU loop's",
                                                             int((bits[r][j] != cpu_bits[j]).sum()))
    assert counts == cpu
    return counts, valid, v


@pytest.mark.parametrize("snr_db,is_db", L.POINTS)
def test_device_loop_under_a_white_burst(chain, cpu_loop, snr_db, is_db):
    counts, valid, v = check_point(chain, cpu_loop, snr_db, is_db)
    assert valid.all()
    assert counts["plain+sym"][1] == 0 and counts["dd+sym"][1] == 0
    assert counts["plain+sym"][0] >= counts["plain"][0] and counts["dd+sym"][0] >= counts["plain"][0]
    assert counts["plain"][1] >= L.CONTRAST and counts["dd"][1] >= L.CONTRAST


def test_device_loop_without_a_burst_and_at_the_limit(chain, cpu_loop):
    counts, valid, v = check_point(chain, cpu_loop, L.CLEAN_SNR_DB, None)
    assert valid.all() and all(counts[r] == L.DELIVERED for r in RINGS) and v.min() > 0.8
    # the limit: the synchroniser refuses a frame on both sides, and acquisition starts over behind it
    counts, valid, v = check_point(chain, cpu_loop, *L.LIMIT)
    assert not valid.all()
    for r in ("plain+sym", "dd+sym"):
        assert counts[r][0] >= counts["plain"][0] and counts[r][1] <= counts["plain"][1]
