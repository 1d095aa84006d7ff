"""-m gpu: DAB_Noise_Profile into DAB_Diversity_Combiner's band-weight overload (tests/cpp/noise_profile_class_harness.cpp).  One
receiver, three frames of the two-path reception of tests/softbit_cases.py with a narrowband interferer added; products, scales and
records come from dabgpu_ofdm_sync_demod_frames_branch.  The object's weights, state and mean equal the host model of
csrc/noise_profile_core.h carried from frame to frame as bytes (a transmitter's carriers excluded, alpha 0.25), Reset starts it again,
and the frames combined with those weights equal the host model of the banded combiner.  The Python binding's host forms give the same."""
import os
import subprocess

import numpy as np
import pytest

import diversity_model as DM
import noise_profile_loop as PL
import noise_profile_model as M
import softbit_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "cpp", "noise_profile_class_harness")
P, TOFF = 3200, 37
STRIDE = P + 1544 + 196608
NB = DM.NB_FRAME_BITS
ALPHA, TX = 0.25, (33, 11)


def test_class_weights_into_the_combiner(oracle, tmp_path_factory):
    import dabgpu
    import torch
    d = tmp_path_factory.mktemp("noise_profile_class")
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
    st = d_st.cpu().numpy().view(sdt)
    assert st["sync_valid"].tolist() == [1] * n and st["fine_time_offset"].tolist() == [TOFF] * n
    freqs = (st["freq_coarse"].astype(np.float32) + st["freq_fine"].astype(np.float32)).astype(np.float32)
    dqs, ks = dq.cpu().numpy().view(np.complex64).reshape(n, 75, 1536), scale.cpu().numpy()
    np.ascontiguousarray(x[:, P - 2656:P + TOFF]).tofile(d / "null.c32")
    freqs.tofile(d / "freq.bin"); dqs.tofile(d / "dq.bin"); ks.tofile(d / "scale.bin")
    e = dict(os.environ)
    e.pop("DABGPU_MIRROR_BANK", None); e.pop("DABGPU_MIRROR_BANK_FROM", None)
    res = subprocess.run([HARNESS, str(d), str(n), str(TOFF), str(ALPHA), str(TX[0]), str(TX[1])], capture_output=True, timeout=300, env=e)
    assert res.returncode == 0 and res.stdout.decode().strip() == f"frames={n}", res.stderr.decode()[-2000:]
    host = M.build_host_model(tmp_path_factory.mktemp("noise_profile_host_model"))
    model = M.HostModel(host, oracle)
    mask = dabgpu.noise_profile_exclude([TX])
    w = np.fromfile(d / "weights.bin", np.float32).reshape(n, 128)
    prof = np.fromfile(d / "profile.bin", np.float32).reshape(n, 128)
    mean = np.fromfile(d / "mean.bin", np.float32)
    comb = np.fromfile(d / "combined.bin", np.int8).reshape(n, NB)
    ck = np.fromfile(d / "combined_scale.bin", np.float32)
    state, py_state = np.zeros(128, np.float32), np.zeros(128, np.float32)
    for i in range(n):
        exp = model.profile(x[i], P - 2656 + TOFF, freqs[i], mask, state, ALPHA)
        assert exp["valid"] == 1
        assert w[i].tobytes() == exp["band_weight"].tobytes() and prof[i].tobytes() == exp["profile"].tobytes(), i
        assert mean[i].view(np.uint32) == exp["mean_noise"].view(np.uint32)
        state = exp["profile"]
        eb, ek, em = M.host_combine_frame(host, [dqs[i]], [ks[i]], None, None, [w[i]])
        assert np.array_equal(comb[i], eb) and ck[i].view(np.uint32) == ek.view(np.uint32) and em == 1, i
        assert not np.array_equal(comb[i], bits[i].cpu().numpy())                                   # the weights did something
        # the binding's host forms
        bw, m, ok = ctx.noise_profile_host(x[i], P - 2656, freq_offset=freqs[i], fine_time_offset=TOFF, exclude=mask, profile=py_state, alpha=ALPHA)
        assert ok == 1 and bw.tobytes() == w[i].tobytes() and py_state.tobytes() == prof[i].tobytes()
        pb, pk, pm = ctx.diversity_combine_host([dqs[i]], [ks[i]], band_weights=[bw])
        assert np.array_equal(pb, comb[i]) and np.float32(pk).view(np.uint32) == ck[i].view(np.uint32) and pm == 1
    ctx.close()
    again = np.fromfile(d / "again.bin", np.float32)
    assert again.tobytes() == w[0].tobytes() and not np.array_equal(w[1], model.profile(x[1], P - 2656 + TOFF, freqs[1], mask)["band_weight"])
    # the interferer is in the profile: the bands under it weigh far less than the median band
    assert np.median(w[0]) > 20.0 * w[0][85:92].max()
