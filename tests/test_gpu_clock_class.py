"""-m gpu: DAB_Clock_Tracker (tests/cpp/clock_class_harness.cpp) against the ABI calls.  One receiver, five frames of products with the
ramp of 200 ppm under noise (tests/clock_model.py), the state carried, an all-zero frame in between that must leave the state alone.
The object's slopes, sums, valid words and de-rotated frames equal Context.clock_estimate and Context.clock_derotate over an in-place
state word on the same products, and the host model of csrc/clock_core.h, as bytes."""
import os
import subprocess

import numpy as np
import pytest

import clock_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "cpp", "clock_class_harness")
N, GAIN, PPM = 5, 0.75, 200.0


def test_class_equals_the_abi_calls(tmp_path_factory):
    import dabgpu
    import torch
    d = tmp_path_factory.mktemp("clock_class")
    rng = np.random.default_rng(9800)
    dqs = np.stack([M.products(rng, PPM, snr_db=12.0, amplitude=1000.0) for _ in range(N)])
    dqs.tofile(d / "dq.bin")
    e = dict(os.environ)
    e.pop("DABGPU_MIRROR_BANK", None); e.pop("DABGPU_MIRROR_BANK_FROM", None)
    res = subprocess.run([HARNESS, str(d), str(N), str(GAIN)], capture_output=True, timeout=300, env=e)
    assert res.returncode == 0 and res.stdout.decode().strip() == f"frames={N}", res.stderr.decode()[-2000:]
    out = np.fromfile(d / "out.bin", np.complex64).reshape(N, 75, 1536)
    slope = np.fromfile(d / "slope.bin", np.int64)
    corr = np.fromfile(d / "corr.bin", np.float32).reshape(N, 2)
    ok = np.fromfile(d / "valid.bin", np.int32)
    ppm = np.fromfile(d / "ppm.bin", np.float64)
    assert ok.tolist() == [1] * N
    # the ABI calls: the state word in place, each frame's products where they lie
    host = M.build_host_model(tmp_path_factory.mktemp("clock_host_model"))
    ctx = dabgpu.Context(0)
    d_dq = torch.from_numpy(dqs.view(np.float32).reshape(N, -1).copy()).cuda()
    d_out = torch.zeros_like(d_dq[0])
    d_state = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_corr = torch.zeros(2, dtype=torch.float32, device="cuda")
    d_ok = torch.zeros(1, dtype=torch.int32, device="cuda")
    state = 0
    for i in range(N):
        ctx.clock_estimate(d_dq[i], 1, slope_in=d_state, gain=GAIN, slope_out=d_state, corr=d_corr, valid=d_ok)
        ctx.clock_derotate(d_dq[i], d_out, 1, d_state)
        torch.cuda.synchronize()
        assert slope[i] == d_state.item() and d_ok.item() == 1 and corr[i].tobytes() == d_corr.cpu().numpy().tobytes(), i
        assert out[i].tobytes() == d_out.cpu().numpy().tobytes(), i
        exp = M.host_estimate(host, dqs[i], state, GAIN)
        state = exp["slope"]
        assert slope[i] == state and corr[i].tobytes() == exp["corr"].tobytes() and out[i].tobytes() == M.host_derotate(host, dqs[i], state).tobytes(), i
        assert ppm[i] == dabgpu.clock_ppm(int(slope[i]))
    ctx.close()
    # the loop closes on the ramp that was put on: what is left shrinks over the first frames
    left = np.abs(ppm - PPM)
    print("tracked", np.round(ppm, 2), "ppm")
    assert left[2] < left[1] < left[0] < PPM
