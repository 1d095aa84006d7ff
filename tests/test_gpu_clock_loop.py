"""-m gpu: the closed loop of tests/clock_loop.py on the device: TxBank -> the channel bank (the static two-path channel of
tests/channel_loop.py) -> the resampler bank applying the sampling-clock error -> dabgpu_ofdm_sync_demod_frames_branch ->
dabgpu_clock_estimate_frames over an in-place state word and dabgpu_clock_derotate_frames on the products that call just wrote ->
dabgpu_diversity_combine_frames over the one branch, once on the products as they came and once on the de-rotated ones, into history
rings -> dabgpu_decode_frames_layout.  At the contrast point (SNR 12 dB, 200 ppm) and without a clock error (15 dB) the tracker's slopes,
residuals, sums and de-rotated products equal the host model over the device's own products as bit patterns, and the counts (FIB CRCs
of 60, wrong bytes of the EEP 3-A sub-channel) equal the CPU loop's."""
import numpy as np
import pytest

import channel_loop as CL
import channel_model as CM
import clock_loop as L
import clock_model as CK
import noise_loop as NL
import resample_loop as RL
import resample_model as RM
import tx_encode_cases as T

pytestmark = pytest.mark.gpu

RINGS = L.PATHS                                        # plain, tracked


class Chain:
    """the transmission on the device, once; a point = (SNR, ppm) through channel, resampler, receiver, tracker, combiner, decoders"""

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

    def stream(self, snr_db, ppm):
        dabgpu, torch = self.dabgpu, self.torch
        n_rx = CL.N_OUT + L.EXTRA
        d_rx = torch.zeros((n_rx, 2), dtype=torch.float32, device="cuda")
        ch = dabgpu.Channel(self.ctx, [CM.to_struct(CL.params(self.iq, snr_db), dabgpu.ChannelStream)])
        ch.apply(self.d_iq, CL.N_FRAMES * dabgpu.NB_FRAME_SAMPLES, n_rx, d_rx)
        P = RL.clock_params(ppm)
        rs = dabgpu.Resampler(self.ctx, [RM.to_struct(P, dabgpu.ResampleStream)], dabgpu.resample_design(RM.design_max_step(P["step_q62"])))
        d_out = torch.zeros((CL.N_OUT + (CL.N_OUT & 1), 2), dtype=torch.float32, device="cuda")
        rs.apply(d_rx, n_rx, CL.N_OUT, d_out)
        torch.cuda.synchronize()
        ch.close(); rs.close()
        return d_out.cpu().numpy().view(np.complex64).reshape(-1)[:CL.N_OUT]

    def point(self, snr_db, ppm):
        """-> (counts {ring: (FIB CRCs of 60, wrong bytes)}, valid [5], tracker outputs dict of [5] arrays, products [5][75][1536],
        de-rotated products [5][75][1536])"""
        dabgpu, torch, ctx = self.dabgpu, self.torch, self.ctx
        F, nb, H, NB = CL.N_FRAMES, self.nb, 8, dabgpu.NB_FRAME_BITS
        slices = NL.slices_of(self.stream(snr_db, ppm))
        sdt, rdt = np.dtype(dabgpu.SYNC_STATE_DTYPE), np.dtype(dabgpu.RESULT_DTYPE)
        soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, L.PL.LEVEL)
        d_st = torch.zeros(sdt.itemsize, dtype=torch.uint8, device="cuda")
        dq = torch.zeros((1, 75, 1536, 2), dtype=torch.float32, device="cuda")
        dv = torch.zeros((1, 75, 1536, 2), dtype=torch.float32, device="cuda")
        scale = torch.zeros((1,), dtype=torch.float32, device="cuda")
        d_state = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_res = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_corr = torch.zeros(2, dtype=torch.float32, device="cuda")
        d_ok = torch.zeros(1, dtype=torch.int32, device="cuda")
        own = torch.zeros((1, NB), dtype=torch.int8, device="cuda")
        hist = {r: torch.zeros((1, H, NB), dtype=torch.int8, device="cuda") for r in RINGS}
        d_fib = torch.zeros((1, 4, 96), dtype=torch.uint8, device="cuda"); fres = torch.zeros((4, 16), dtype=torch.uint8, device="cuda")
        msc = torch.zeros((1, 4, nb), dtype=torch.uint8, device="cuda"); mres = torch.zeros((4 * len(self.gsubs), 16), dtype=torch.uint8, device="cuda")
        cifs = self.pay.reshape(4 * F, nb)[:, :self.n0]
        crc, wrong = {r: 0 for r in RINGS}, {r: 0 for r in RINGS}
        valid = np.zeros(F, np.int32)
        trk = dict(slope=np.zeros(F, np.int64), residual=np.zeros(F, np.int64), corr=np.zeros((F, 2), np.float32), ok=np.zeros(F, np.int32))
        products, derotated = np.zeros((F, 75, 1536), np.complex64), np.zeros((F, 75, 1536), np.complex64)
        for j in range(F):
            d_slice = torch.from_numpy(np.ascontiguousarray(slices[j:j + 1]).view(np.float32)).cuda()
            ctx.ofdm_sync_demod_frames_branch(d_slice, 1, L.PL.STRIDE, L.PL.P, d_st, own, soft, dq, soft_scale=scale)
            ctx.clock_estimate(dq, 1, sync=d_st, slope_in=d_state, gain=1.0, slope_out=d_state, residual=d_res, corr=d_corr, valid=d_ok)
            ctx.clock_derotate(dq, dv, 1, d_state, sync=d_st)
            ctx.diversity_combine([(dq, scale, None, d_st)], 1, hist["plain"][:, j % H], bits_frame_stride=H * NB)
            ctx.diversity_combine([(dv, scale, None, d_st)], 1, hist["tracked"][:, j % H], bits_frame_stride=H * NB)
            torch.cuda.synchronize()
            valid[j] = int(d_st.cpu().numpy().view(sdt)[0]["sync_valid"])
            if not valid[j]:
                d_st.zero_()                                                             # acquisition starts over, as in the CPU loop's receiver
            trk["slope"][j], trk["residual"][j], trk["ok"][j] = d_state.item(), d_res.item(), d_ok.item()
            trk["corr"][j] = d_corr.cpu().numpy()
            products[j] = dq.cpu().numpy().view(np.complex64).reshape(75, 1536)
            derotated[j] = dv.cpu().numpy().view(np.complex64).reshape(75, 1536)
            for r in RINGS:
                ctx.decode_frames(hist[r], 1, H * NB, H, j % H, self.gsubs, d_fib, fres, msc, 4 * nb, mres)
                torch.cuda.synchronize()
                crc[r] += int(sum(bin(int(m)).count("1") for m in fres.cpu().numpy().view(rdt)["crc_ok_mask"].reshape(-1)))
                got = msc.cpu().numpy()[0][:, :self.n0]
                for c in range(4):
                    if 4 * j + c >= 15:
                        wrong[r] += int((got[c] != cifs[4 * j + c - 15]).sum())
        return {r: (crc[r], wrong[r]) for r in RINGS}, valid, trk, products, derotated


@pytest.fixture(scope="module")
def cpu_loop(oracle, tmp_path_factory):
    return L.Loop(oracle, tmp_path_factory.mktemp("clock_loop"))


@pytest.fixture(scope="module")
def chain(oracle):
    c = Chain(oracle)
    yield c
    c.close()


def check_point(chain, cpu_loop, snr_db, ppm):
    counts, valid, trk, products, derotated = chain.point(snr_db, ppm)
    cpu = cpu_loop.counts(snr_db, ppm)
    branch = cpu_loop.branch(snr_db, ppm)
    tracked = [round(CK.ppm_of(s), 1) for s in trk["slope"]]
    print(f"SNR {snr_db} dB, {ppm} ppm: device {counts}, CPU {cpu}, valid {valid.tolist()}, tracked {tracked} ppm")
    assert valid.all() and np.array_equal(valid, branch["valid"])
    # the tracker's outputs, bit for bit, from the device's own products, the state carried
    state = 0
    for j in range(CL.N_FRAMES):
        e = CK.host_estimate(cpu_loop.clock_lib, products[j], state, 1.0)
        state = e["slope"]
        assert (trk["slope"][j], trk["residual"][j], trk["ok"][j]) == (e["slope"], e["residual"], e["valid"]), j
        assert trk["corr"][j].tobytes() == e["corr"].tobytes(), j
        assert derotated[j].tobytes() == CK.host_derotate(cpu_loop.clock_lib, products[j], state).tobytes(), j
    assert counts == cpu
    if np.array_equal(products.view(np.uint32), branch["dq"].view(np.uint32)):           # the same products: the same slopes as the CPU loop's
        assert np.array_equal(trk["slope"], branch["slope"])
    return counts, trk


def test_device_loop_under_a_clock_error(chain, cpu_loop):
    snr_db, ppm = 12.0, 200.0
    assert (snr_db, ppm) in L.POINTS
    counts, trk = check_point(chain, cpu_loop, snr_db, ppm)
    assert counts["tracked"] == L.DELIVERED and counts["plain"][1] >= L.CONTRAST
    assert all(abs(CK.ppm_of(trk["slope"][j]) - ppm) <= L.ACCURACY_BOUND_PPM for j in L.ACCURACY_FRAMES)


def test_device_loop_without_a_clock_error(chain, cpu_loop):
    counts, trk = check_point(chain, cpu_loop, *L.CLEAN[0])
    assert all(counts[r] == L.DELIVERED for r in RINGS)
