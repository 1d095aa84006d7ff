"""-m gpu: DAB_Diversity_Combiner behind two OFDM_Demod mirrors (tests/cpp/diversity_class_harness.cpp).  Two captures of one transmission
-- the two-path reception of tests/softbit_cases.py at 15 dB, and the same reception under further noise of its own -- each through an
OFDM_Demod under SetSoftDecision(DABGPU_SOFT_CSI, 64); the frames' GetFrameDataVec() and GetSoftScale() are fed, pair by pair, into the
combiner.  GetSoftScale() is the frame's own k: the branch's own soft bits are the host model's over its products and that scale.  The
combined bits, scale and live mask equal the host model of csrc/diversity_core.h, with equal weights and with maximal-ratio weights; a
pair whose second branch has no frame gives the first branch's own bits."""
import os
import subprocess

import numpy as np
import pytest

import channel_loop as CL
import diversity_model as DM
import softbit_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "cpp", "diversity_class_harness")
NB = DM.NB_FRAME_BITS
LEAD = 2656                                  # the capture repeats its first NULL symbol in front: the run-in of the power-dip search


@pytest.fixture(scope="module")
def captures(oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("diversity_class")
    rx = SC.received(oracle, d)[0]
    rng = np.random.default_rng(9640)
    sigma = 0.7 * float(np.sqrt(np.mean(np.abs(rx) ** 2) / 2) / 10 ** (15.0 / 20))
    other = (rx + sigma * (rng.standard_normal(rx.size) + 1j * rng.standard_normal(rx.size))).astype(np.complex64)
    for b, x in enumerate((rx, other)):
        np.concatenate([x[:LEAD], x]).astype(np.complex64).tofile(d / f"iq{b}.c32")
    return d


@pytest.mark.parametrize("weights", [(1.0, 1.0), (1.0, 0.4)])
def test_class_combination_equals_the_model(captures, tmp_path_factory, weights):
    d = captures
    out = d / f"out_{weights[1]:g}"
    os.makedirs(out, exist_ok=True)
    e = dict(os.environ)
    e.pop("DABGPU_MIRROR_BANK", None); e.pop("DABGPU_MIRROR_BANK_FROM", None)
    res = subprocess.run([HARNESS, str(d / "iq0.c32"), str(d / "iq1.c32"), str(out), "65536", "64", repr(weights[0]), repr(weights[1])],
                         capture_output=True, timeout=300, env=e)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    info = dict(kv.split("=") for kv in res.stdout.decode().strip().split(" "))
    pairs = int(info["pairs"])
    assert pairs >= CL.N_FRAMES - 1 and info["frames0"] == info["frames1"]
    host = DM.build_host_model(tmp_path_factory.mktemp("diversity_host_model"))
    dq = [np.fromfile(out / f"dq{b}.bin", np.complex64).reshape(-1, 75, 1536) for b in range(2)]
    k = [np.fromfile(out / f"scale{b}.bin", np.float32) for b in range(2)]
    own = [np.fromfile(out / f"own{b}.bin", np.int8).reshape(-1, NB) for b in range(2)]
    comb = np.fromfile(out / "combined.bin", np.int8).reshape(pairs, NB)
    ck, live = np.fromfile(out / "combined_scale.bin", np.float32), np.fromfile(out / "live.bin", np.uint32)
    assert (k[0] > 0).all() and (k[1] > 0).all() and live.tolist() == [3] * pairs
    for i in range(pairs):
        for b in range(2):
            # the scale the class reports with a frame is the one its soft bits were scaled with
            assert np.array_equal(DM.host_combine_frame(host, [dq[b][i]], [k[b][i]])[0], own[b][i]), (b, i)
        eb, ek, em = DM.host_combine_frame(host, [dq[0][i], dq[1][i]], [k[0][i], k[1][i]], list(weights))
        assert np.array_equal(comb[i], eb) and ck[i].view(np.uint32) == ek.view(np.uint32) and em == 3, i
        assert not np.array_equal(comb[i], own[0][i])
    single = np.fromfile(out / "combined_single.bin", np.int8)
    assert np.array_equal(single, own[0][pairs - 1])
