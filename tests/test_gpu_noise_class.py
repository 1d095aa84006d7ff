"""-m gpu: DAB_Noise_Estimator into DAB_Diversity_Combiner (tests/cpp/noise_class_harness.cpp).  Two branches of two frames of the two-path
reception of tests/softbit_cases.py, the second branch 9 dB noisier; products, scales and records come from
dabgpu_ofdm_sync_demod_frames_branch.  The class's records equal the host model of csrc/noise_core.h as bytes, and the frames combined
with the records' weights equal the host model of csrc/diversity_core.h with those weights."""
import os
import subprocess

import numpy as np
import pytest

import diversity_model as DM
import noise_model as M
import softbit_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "cpp", "noise_class_harness")
P, TOFF = 3200, 37
STRIDE = P + 1544 + 196608
NB = DM.NB_FRAME_BITS


def test_class_weights_into_the_combiner(oracle, tmp_path_factory):
    import dabgpu
    import torch
    d = tmp_path_factory.mktemp("noise_class")
    rx = SC.received(oracle, d)[0]
    rng = np.random.default_rng(9900)
    n = 2
    A = np.stack([rx[a:a + STRIDE] for a in (2656 + j * 196608 + SC.CL.TIMING - (P + TOFF) for j in (1, 2))]).astype(np.complex64)
    extra = float(np.sqrt(np.mean(np.abs(A[0, 900:3100]) ** 2) * (10.0 ** 0.9 - 1.0) / 2.0))
    B = (A + extra * (rng.standard_normal(A.shape) + 1j * rng.standard_normal(A.shape))).astype(np.complex64)
    ctx = dabgpu.Context(0)
    soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0)
    sdt = np.dtype(dabgpu.SYNC_STATE_DTYPE)
    dqs, ks, freqs = [], [], []
    for b, x in enumerate((A, B)):
        d_iq = torch.from_numpy(x.view(np.float32).reshape(n, STRIDE, 2)).cuda()
        d_st = torch.from_numpy(np.zeros(n, sdt).view(np.uint8)).cuda()
        bits = torch.zeros((n, NB), dtype=torch.int8, device="cuda")
        dq = torch.zeros((n, 75, 1536, 2), dtype=torch.float32, device="cuda")
        scale = torch.zeros((n,), dtype=torch.float32, device="cuda")
        ctx.ofdm_sync_demod_frames_branch(d_iq, n, STRIDE, P, d_st, bits, soft, dq, soft_scale=scale)
        torch.cuda.synchronize()
        st = d_st.cpu().numpy().view(sdt)
        assert st["sync_valid"].tolist() == [1, 1] and st["fine_time_offset"].tolist() == [TOFF, TOFF]
        freqs.append((st["freq_coarse"].astype(np.float32) + st["freq_fine"].astype(np.float32)).astype(np.float32))
        dqs.append(dq.cpu().numpy().view(np.complex64).reshape(n, 75, 1536))
        ks.append(scale.cpu().numpy())
        np.ascontiguousarray(x[:, P - 2656:P - 2656 + M.NB_NULL + 2552 + TOFF]).tofile(d / f"null{b}.c32")
        freqs[b].tofile(d / f"freq{b}.bin"); dqs[b].tofile(d / f"dq{b}.bin"); ks[b].tofile(d / f"scale{b}.bin")
    ctx.close()
    e = dict(os.environ)
    e.pop("DABGPU_MIRROR_BANK", None); e.pop("DABGPU_MIRROR_BANK_FROM", None)
    res = subprocess.run([HARNESS, str(d), str(n), str(TOFF)], capture_output=True, timeout=300, env=e)
    assert res.returncode == 0 and res.stdout.decode().strip() == f"frames={n}", res.stderr.decode()[-2000:]
    noise = M.HostModel(M.build_host_model(tmp_path_factory.mktemp("noise_host_model")), oracle)
    dv = DM.build_host_model(tmp_path_factory.mktemp("noise_class_diversity"))
    recs = [np.fromfile(d / f"rec{b}.bin", M.RECORD_DTYPE) for b in range(2)]
    for b, x in enumerate((A, B)):
        for i in range(n):
            exp, _ = noise.estimate(x[i], P - 2656 + TOFF, freqs[b][i])
            assert recs[b][i].tobytes() == exp.tobytes() and exp["valid"] == 1, (b, i, recs[b][i], exp)
    comb = np.fromfile(d / "combined.bin", np.int8).reshape(n, NB)
    ck, live = np.fromfile(d / "combined_scale.bin", np.float32), np.fromfile(d / "live.bin", np.uint32)
    for i in range(n):
        w = [recs[0]["weight"][i], recs[1]["weight"][i]]
        eb, ek, em = DM.host_combine_frame(dv, [dqs[0][i], dqs[1][i]], [ks[0][i], ks[1][i]], w)
        assert np.array_equal(comb[i], eb) and ck[i].view(np.uint32) == ek.view(np.uint32) and em == 3 == live[i], i
        unit = DM.host_combine_frame(dv, [dqs[0][i], dqs[1][i]], [ks[0][i], ks[1][i]])[0]
        assert not np.array_equal(comb[i], unit)                     # the weights did something
