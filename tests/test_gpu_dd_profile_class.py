"""-m gpu: DAB_DD_Profile into DAB_Diversity_Combiner's band-weight overload (tests/cpp/dd_profile_class_harness.cpp) against the Python
path.  One receiver, three frames of the two-path reception of tests/softbit_cases.py with a narrowband interferer added; products and
scales come from dabgpu_ofdm_sync_demod_frames_branch.  The object's weights, state and mean equal Context.dd_profile on the same
products with the state carried on the device, and the host model of csrc/dd_profile_core.h, as bytes (scattered carriers excluded, alpha
0.25); Reset starts it again, an empty table takes the exclusion away, and the frames combined with those weights equal the host model of
the banded combiner and Context.diversity_combine(band_weights=)."""
import os
import subprocess

import numpy as np
import pytest

import dd_profile_model as M
import diversity_model as DM
import noise_profile_loop as PL
import noise_profile_model as PM
import softbit_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "cpp", "dd_profile_class_harness")
P, TOFF = 3200, 37
STRIDE = P + 1544 + 196608
NB = DM.NB_FRAME_BITS
ALPHA = 0.25


def test_class_equals_the_python_path(oracle, tmp_path_factory):
    import dabgpu
    import torch
    d = tmp_path_factory.mktemp("dd_profile_class")
    rx = SC.received(oracle, d)[0]
    n = 3
    jam = PL.interferer(rx.size, 300.3, 96, float(np.mean(np.abs(rx[3000:190000]) ** 2)), 9950)
    rx = (rx + jam).astype(np.complex64)
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
    mask = PM.exclude_words(np.random.default_rng(9500).choice(1536, 150, replace=False))
    dqs.tofile(d / "dq.bin"); ks.tofile(d / "scale.bin"); mask.tofile(d / "exclude.bin")
    e = dict(os.environ)
    e.pop("DABGPU_MIRROR_BANK", None); e.pop("DABGPU_MIRROR_BANK_FROM", None)
    res = subprocess.run([HARNESS, str(d), str(n), str(ALPHA)], capture_output=True, timeout=300, env=e)
    assert res.returncode == 0 and res.stdout.decode().strip() == f"frames={n}", res.stderr.decode()[-2000:]
    host = M.build_host_model(tmp_path_factory.mktemp("dd_profile_host_model"))
    np_host = PM.build_host_model(tmp_path_factory.mktemp("noise_profile_host_model"))
    w = np.fromfile(d / "weights.bin", np.float32).reshape(n, 128)
    prof = np.fromfile(d / "profile.bin", np.float32).reshape(n, 128)
    mean = np.fromfile(d / "mean.bin", np.float32)
    comb = np.fromfile(d / "combined.bin", np.int8).reshape(n, NB)
    ck = np.fromfile(d / "combined_scale.bin", np.float32)
    # the Python path: each frame's call on the products where the demodulator left them, the state carried on the device
    d_ex = torch.from_numpy(mask.view(np.int32)).cuda()
    d_state = torch.zeros((1, 128), dtype=torch.float32, device="cuda")
    d_w = torch.zeros((1, 128), dtype=torch.float32, device="cuda")
    d_m = torch.zeros(1, dtype=torch.float32, device="cuda")
    d_bits = torch.zeros((1, NB), dtype=torch.int8, device="cuda")
    d_k = torch.zeros(1, dtype=torch.float32, device="cuda")
    state, py_state = np.zeros(128, np.float32), np.zeros(128, np.float32)
    for i in range(n):
        ctx.dd_profile(dq[i:i + 1], 1, sync=d_st[i * sdt.itemsize:], exclude=d_ex, profile_in=d_state, alpha=ALPHA, profile_out=d_state, band_weight=d_w,
                       mean_noise=d_m)
        ctx.diversity_combine([(dq[i:i + 1], scale[i:i + 1], None, None)], 1, d_bits, soft_scale=d_k, band_weights=[d_w])
        torch.cuda.synchronize()
        assert w[i].tobytes() == d_w.cpu().numpy().tobytes() and prof[i].tobytes() == d_state.cpu().numpy().tobytes(), i
        assert mean[i].tobytes() == d_m.cpu().numpy().tobytes()
        assert np.array_equal(comb[i], d_bits.cpu().numpy()[0]) and ck[i].tobytes() == d_k.cpu().numpy().tobytes(), i
        exp = M.host_frame(host, dqs[i], True, mask, state, ALPHA)
        assert exp["valid"] == 1
        assert w[i].tobytes() == exp["band_weight"].tobytes() and prof[i].tobytes() == exp["profile"].tobytes(), i
        assert mean[i].view(np.uint32) == exp["mean_noise"].view(np.uint32)
        state = exp["profile"]
        eb, ek, em = PM.host_combine_frame(np_host, [dqs[i]], [ks[i]], None, None, [w[i]])
        assert np.array_equal(comb[i], eb) and ck[i].view(np.uint32) == ek.view(np.uint32) and em == 1, i
        assert not np.array_equal(comb[i], bits[i].cpu().numpy())                                   # the weights did something
        # the binding's host form
        bw, m, ok = ctx.dd_profile_host(dqs[i], exclude=mask, profile=py_state, alpha=ALPHA)
        assert ok == 1 and bw.tobytes() == w[i].tobytes() and py_state.tobytes() == prof[i].tobytes()
    ctx.close()
    again = np.fromfile(d / "again.bin", np.float32)
    plain = np.fromfile(d / "plain.bin", np.float32)
    assert again.tobytes() == w[0].tobytes() and not np.array_equal(w[1], M.host_frame(host, dqs[1], True, mask)["band_weight"])
    assert plain.tobytes() == M.host_frame(host, dqs[0])["band_weight"].tobytes() and plain.tobytes() != again.tobytes()
    # the interferer is in the profile: the bands under it weigh far less than the median band
    assert np.median(w[0]) > 20.0 * w[0][85:92].max()
