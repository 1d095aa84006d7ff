"""-m gpu: DAB_Symbol_Profile into DAB_Diversity_Combiner's symbol-weight overload (tests/cpp/sym_profile_class_harness.cpp) against the
Python path.  One receiver, three frames of the two-path reception of tests/softbit_cases.py with the white burst of
tests/sym_profile_loop.py added; products and scales come from dabgpu_ofdm_sync_demod_frames_branch.  The object's weights, noise figures
and reference equal Context.sym_profile on the same products and the host model of csrc/sym_profile_core.h as bytes, and the frames
combined with those weights -- alone and on top of band weights -- equal the host model of the symbol-weighted combiner and
Context.diversity_combine(symbol_weights=)."""
import os
import subprocess

import numpy as np
import pytest

import diversity_model as DM
import diversity_symbols_model as DS
import softbit_cases as SC
import sym_profile_loop as L
import sym_profile_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "cpp", "sym_profile_class_harness")
P, TOFF = 3200, 37
STRIDE = P + 1544 + 196608
NB = DM.NB_FRAME_BITS


def test_class_equals_the_python_path(oracle, tmp_path_factory):
    import dabgpu
    import torch
    d = tmp_path_factory.mktemp("sym_profile_class")
    rx = SC.received(oracle, d)[0]
    n = 3
    rx = (rx + L.burst(rx.size, 4.0 * float(np.mean(np.abs(rx[3000:190000]) ** 2)))).astype(np.complex64)          # I / S + 6 dB
    x = np.stack([rx[a:a + STRIDE] for a in (2656 + j * 196608 + SC.CL.TIMING - (P + TOFF) for j in (1, 2, 3))]).astype(np.complex64)
    ctx = dabgpu.Context(0)
    soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0)
    sdt = np.dtype(dabgpu.SYNC_STATE_DTYPE)
    d_iq = torch.from_numpy(x.view(np.float32).reshape(n, STRIDE, 2)).cuda()
    d_st = torch.from_numpy(np.zeros(n, sdt).view(np.uint8)).cuda()
    bits = torch.zeros((n, NB), dtype=torch.int8, device="cuda")
    dq = torch.zeros((n, 75, 1536, 2), dtype=torch.float32, device="cuda")
    scale = torch.zeros((n,), dtype=torch.float32, device="cuda")
    ctx.ofdm_sync_demod_frames_branch(d_iq, n, STRIDE, P, d_st, bits, soft, dq, soft_scale=scale)
    torch.cuda.synchronize()
    assert d_st.cpu().numpy().view(sdt)["sync_valid"].tolist() == [1] * n
    dqs, ks = dq.cpu().numpy().view(np.complex64).reshape(n, 75, 1536), scale.cpu().numpy()
    band = np.exp(np.random.default_rng(9600).uniform(-1.0, 1.0, (n, 128))).astype(np.float32)
    dqs.tofile(d / "dq.bin"); ks.tofile(d / "scale.bin"); band.tofile(d / "band.bin")
    e = dict(os.environ)
    e.pop("DABGPU_MIRROR_BANK", None); e.pop("DABGPU_MIRROR_BANK_FROM", None)
    res = subprocess.run([HARNESS, str(d), str(n)], capture_output=True, timeout=300, env=e)
    assert res.returncode == 0 and res.stdout.decode().strip() == f"frames={n}", res.stderr.decode()[-2000:]
    host = M.build_host_model(tmp_path_factory.mktemp("sym_profile_host_model"))
    w = np.fromfile(d / "weights.bin", np.float32).reshape(n, 75)
    q = np.fromfile(d / "noise.bin", np.float32).reshape(n, 75)
    ref = np.fromfile(d / "ref.bin", np.float32)
    ok = np.fromfile(d / "valid.bin", np.int32)
    comb = np.fromfile(d / "combined.bin", np.int8).reshape(n, NB)
    both = np.fromfile(d / "combined_banded.bin", np.int8).reshape(n, NB)
    ck = np.fromfile(d / "combined_scale.bin", np.float32)
    assert ok.tolist() == [1] * n and not np.fromfile(d / "zero.bin", np.float32).any()
    # the Python path: each frame's call on the products where the demodulator left them
    d_v = torch.zeros((1, 75), dtype=torch.float32, device="cuda")
    d_q = torch.zeros((1, 75), dtype=torch.float32, device="cuda")
    d_r = torch.zeros(1, dtype=torch.float32, device="cuda")
    d_band = torch.from_numpy(band).cuda()
    d_bits = torch.zeros((1, NB), dtype=torch.int8, device="cuda")
    d_k = torch.zeros(1, dtype=torch.float32, device="cuda")
    for i in range(n):
        ctx.sym_profile(dq[i:i + 1], 1, sync=d_st[i * sdt.itemsize:], symbol_weight=d_v, symbol_noise=d_q, ref_noise=d_r)
        ctx.diversity_combine([(dq[i:i + 1], scale[i:i + 1], None, None)], 1, d_bits, soft_scale=d_k, symbol_weights=[d_v])
        torch.cuda.synchronize()
        assert w[i].tobytes() == d_v.cpu().numpy().tobytes() and q[i].tobytes() == d_q.cpu().numpy().tobytes() and ref[i].tobytes() == d_r.cpu().numpy().tobytes(), i
        assert np.array_equal(comb[i], d_bits.cpu().numpy()[0]) and ck[i].tobytes() == d_k.cpu().numpy().tobytes(), i
        ctx.diversity_combine([(dq[i:i + 1], scale[i:i + 1], None, None)], 1, d_bits, band_weights=[d_band[i:i + 1]], symbol_weights=[d_v])
        torch.cuda.synchronize()
        assert np.array_equal(both[i], d_bits.cpu().numpy()[0]), i
        exp = M.host_frame(host, dqs[i])
        assert exp["valid"] == 1 and w[i].tobytes() == exp["symbol_weight"].tobytes() and q[i].tobytes() == exp["symbol_noise"].tobytes(), i
        assert ref[i].view(np.uint32) == exp["ref_noise"].view(np.uint32)
        eb, ek, em = DS.host_combine_frame(host, [dqs[i]], [ks[i]], None, None, None, [w[i]])
        assert np.array_equal(comb[i], eb) and ck[i].view(np.uint32) == ek.view(np.uint32) == ks[i].view(np.uint32) and em == 1, i
        eb, ek, em = DS.host_combine_frame(host, [dqs[i]], [ks[i]], None, None, [band[i]], [w[i]])
        assert np.array_equal(both[i], eb), i
        assert not np.array_equal(comb[i], bits[i].cpu().numpy())                                   # the weights did something
        # the binding's host form
        hv, hq, href, hok = ctx.sym_profile_host(dqs[i])
        assert hok == 1 and hv.tobytes() == w[i].tobytes() and hq.tobytes() == q[i].tobytes()
    ctx.close()
    # the bursts are in the weights: some rows of every frame weigh less than a fifth, and more than half keep weight 1
    assert ((w < 0.2).sum(axis=1) >= 2).all() and ((w == 1).sum(axis=1) >= 38).all()
