"""-m gpu: the noise estimate behind dabgpu_ofdm_sync_demod_frames_branch, on the call's own samples, stride and records: two branches of
three streams each, the second branch 9 dB noisier and one of its streams noise only (refused by its synchroniser).  The scale of
(level, signal_power) is the call's d_soft_scale word as a bit pattern; the weight arrays go into the branch table of
dabgpu_diversity_combine_frames as they are, and the combined bits equal the numpy diversity model with those weights."""
import numpy as np
import pytest

import diversity_model as DM
import noise_model as M
import softbit_cases as SC

pytestmark = pytest.mark.gpu
P = 3200                                  # the PRS is expected P samples into a slice, so the NULL begins at P - 2656
STRIDE = P + 1544 + 196608
TOFF = 37
NB = SC.NB_FRAME_BITS
LEVEL = 64.0


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


def test_weights_behind_a_branch_go_into_the_combiner(ctx, oracle, tmp_path_factory):
    import dabgpu
    import torch
    rx = SC.received(oracle, tmp_path_factory.mktemp("noise_branch_channel"))[0]
    noise = M.HostModel(M.build_host_model(tmp_path_factory.mktemp("noise_host_model")), oracle)
    dv = DM.build_host_model(tmp_path_factory.mktemp("noise_branch_diversity"))
    rng = np.random.default_rng(9700)
    n = 3
    A = np.stack([rx[a:a + STRIDE] for a in (2656 + j * 196608 + SC.CL.TIMING - (P + TOFF) for j in (1, 2, 3))]).astype(np.complex64)
    extra = float(np.sqrt(np.mean(np.abs(A[0, 900:3100]) ** 2) * (10.0 ** 0.9 - 1.0) / 2.0))       # (inside the NULL, behind the echo: noise only) 9 dB above it
    B = (A + extra * (rng.standard_normal(A.shape) + 1j * rng.standard_normal(A.shape))).astype(np.complex64)
    B[1] = (rng.standard_normal(STRIDE) + 1j * rng.standard_normal(STRIDE)).astype(np.complex64)
    soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, LEVEL)
    sdt = np.dtype(dabgpu.SYNC_STATE_DTYPE)
    table, kept = [], []
    for x in (A, B):
        d_iq = torch.from_numpy(x.view(np.float32).reshape(n, STRIDE, 2)).cuda()
        d_st = torch.from_numpy(np.zeros(n, sdt).view(np.uint8)).cuda()
        bits = torch.zeros((n, NB), dtype=torch.int8, device="cuda")
        dq = torch.zeros((n, 75, 1536, 2), dtype=torch.float32, device="cuda")
        scale = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
        w = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
        sig = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
        ok = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        ctx.ofdm_sync_demod_frames_branch(d_iq, n, STRIDE, P, d_st, bits, soft, dq, soft_scale=scale)
        ctx.noise_estimate(d_iq, n, STRIDE, P - 2656, states=d_st, weight=w, signal_power=sig, valid=ok)
        table.append((dq, scale, w, d_st))
        kept.append((x, d_st, scale, w, sig, ok))
    out = torch.full((n, NB), 9, dtype=torch.int8, device="cuda")
    mask = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ctx.diversity_combine(table, n, out, live_mask=mask)
    torch.cuda.synchronize()
    got = []
    for b, (x, d_st, scale, w, sig, ok) in enumerate(kept):
        st = d_st.cpu().numpy().view(sdt)
        k, wt, P_, v = scale.cpu().numpy(), w.cpu().numpy(), sig.cpu().numpy(), ok.cpu().numpy()
        assert st["sync_valid"].tolist() == ([1, 1, 1] if b == 0 else [1, 0, 1])
        for s in range(n):
            if not st["sync_valid"][s]:
                assert wt[s] == 0 and P_[s] == 0 and v[s] == 0 and k[s] == -1.0          # the demodulator left its row alone, the estimator wrote zeros
                continue
            assert st["fine_time_offset"][s] == TOFF and v[s] == 1
            rec, _ = noise.estimate(x[s], P - 2656 + TOFF, np.float32(st["freq_coarse"][s]) + np.float32(st["freq_fine"][s]))
            assert np.float32(rec["weight"]).view(np.uint32) == wt[s].view(np.uint32) and np.float32(rec["signal_power"]).view(np.uint32) == P_[s].view(np.uint32)
            # signal_power is the power the demodulator scaled this frame by
            assert np.float32(noise.L.noise_host_scale(np.float32(LEVEL), P_[s])).view(np.uint32) == k[s].view(np.uint32), (b, s)
        got.append((st, k, wt))
    # 9 dB: the weights of the two branches differ by a factor of 10^0.9.  The ratio of two independent estimates has sqrt 2 of one
    # estimate's deviation, and the level the extra noise was sized by is itself a mean over 2200 samples (1 / sqrt 2200): five of the sum
    ratio = got[0][2][[0, 2]] / got[1][2][[0, 2]]
    tol = 5.0 * float(np.sqrt(2.0 * M.relative_deviation() ** 2 + 1.0 / 2200.0))
    print("weight ratios A / B:", ratio, "expected", 10.0 ** 0.9, "tolerance", tol)
    assert (np.abs(ratio / 10.0 ** 0.9 - 1.0) < tol).all(), ratio
    mapper = DM.host_mapper(dv)
    bits = out.cpu().numpy()
    for s in range(n):
        dq = [t[0][s].cpu().numpy().view(np.complex64).reshape(75, 1536) for t in table]
        exp, kk, m = DM.combine_frame(dq, [g[1][s] for g in got], mapper, [g[2][s] for g in got], [int(g[0]["sync_valid"][s]) for g in got])
        assert m == int(mask.cpu().numpy()[s]) == (1 if s == 1 else 3)
        assert np.array_equal(bits[s], exp), s
