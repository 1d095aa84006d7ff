"""-m gpu: dabgpu_simulate_transmitter's fading options (--doppler-hz, --fading-seed, --profile, --tap-kind).  With identity fading options
(no Doppler, every tap static) the bytes are the old ones; with --profile tu6 --doppler-hz the output equals the fading host model
(tests/channel_fading_model.py) over the modulator's frames, byte for byte, for the reference's frame and for channel-coded frames.
Two frames each."""
import math
import os
import subprocess

import numpy as np
import pytest

import channel_fading_loop as FL
import channel_fading_model as FM
import channel_model as CM
import tx_encode_cases as T
import tx_model as TX
from test_gpu_channel_cli import CH_ARGS, CLI, S, SUB_ARGS, SUBS, U8_SCALE, cli

pytestmark = pytest.mark.gpu
DOPPLER_HZ, SEED = 120.0, 31
FADE_ARGS = ["--snr-db", "14", "--cfo-hz", "333", "--timing-offset", "37", "--noise-seed", "9", "--profile", "tu6", "--doppler-hz", DOPPLER_HZ, "--fading-seed", SEED]


def params():
    """what the tool derives from FADE_ARGS: tu6 (unit total power), sigma from the symbols' mean power 1536 x sum |tap|^2"""
    taps = FL.tu6_taps()
    h2 = sum(float(np.float32(re)) ** 2 + float(np.float32(im)) ** 2 for _, re, im in taps)
    sigma = np.float32(math.sqrt(1536.0 * h2 / (2.0 * 10.0 ** (14.0 / 10.0))))
    return CM.params_dict(taps=taps, freq_q64=int(round(math.ldexp(333.0 / 2.048e6, 64))), start=37, seed=9, noise_sigma=float(sigma))


def test_identity_fading_options_give_the_old_bytes():
    plain = cli("--frames", 2)
    assert np.array_equal(cli("--frames", 2, "--fading-seed", 5), plain)
    assert np.array_equal(cli("--frames", 2, "--doppler-hz", 0, "--tap-kind", "0:static"), plain)
    old = cli("--frames", 2, *CH_ARGS)
    assert np.array_equal(cli("--frames", 2, *CH_ARGS, "--doppler-hz", 50, "--tap-kind", "0:static", "--tap-kind", "1:static", "--fading-seed", 3), old)
    coded = cli(*SUB_ARGS, "--seed", 4, "--frames", 2, *CH_ARGS)
    assert np.array_equal(cli(*SUB_ARGS, "--seed", 4, "--frames", 2, *CH_ARGS, "--doppler-hz", 0, "--tap-kind", "1:static", "--tap-kind", "0:static"), coded)


def test_refused_options_are_reported():
    for args, text in ((["--profile", "tu7", "--doppler-hz", 10], "unknown profile"), (["--doppler-hz", 1001], "doppler_cycles"),
                       (["--profile", "tu6"], "--doppler-hz"), (["--profile", "tu6", "--tap", "0:1:0", "--doppler-hz", 1], "--tap"),
                       (["--doppler-hz", 10, "--tap-kind", "1:rayleigh"], "tap 1 of 1"), (["--doppler-hz", 10, "--tap-kind", "0:fast"], "--tap-kind")):
        res = subprocess.run([CLI, "--frames", "1"] + [str(a) for a in args], capture_output=True, timeout=300)
        assert res.returncode != 0 and text.encode() in res.stderr, (args, res.stderr[-500:])


def test_reference_frame_through_tu6_equals_the_host_model(oracle, tmp_path):
    host = FM.build_host_model(tmp_path)
    frame = TX.modulate(oracle, 1, TX.scrambler_bytes(TX.payload_bytes(oracle, 1)), TX.LAYOUT_REFERENCE).astype(np.complex64)
    P = params()
    table = FM.plan_stream(P, DOPPLER_HZ / 2.048e6, SEED, 0, [FM.FADING] * 6)
    got = cli("--frames", 2, *FADE_ARGS).reshape(-1, 2)
    exp = FM.host_apply(host, [P], [table], frame, 0, 2 * S, True, fmt=CM.U8, scale=U8_SCALE)[0]
    assert np.array_equal(got, exp)
    # one tap Rice, one static, through --tap-kind
    table = FM.plan_stream(P, DOPPLER_HZ / 2.048e6, SEED, 0, [1, 0, 1, 1, 1, 1], [float(np.float32(10.0 ** 0.6))] + [0.0] * 5, [0.7] + [0.0] * 5)
    got = cli("--frames", 1, *FADE_ARGS, "--tap-kind", "0:rice:6", "--tap-kind", "1:static").reshape(-1, 2)
    assert np.array_equal(got, FM.host_apply(host, [P], [table], frame, 0, S, True, fmt=CM.U8, scale=U8_SCALE)[0])


def test_coded_frames_through_tu6_equal_the_host_model(tmp_path):
    import dabgpu
    host = FM.build_host_model(tmp_path)
    ctx = dabgpu.Context(0)
    bank = dabgpu.TxBank(ctx, 1, [T.g_sub(dabgpu, d) for d in SUBS])
    nb, F = bank.cif_in_bytes, 2
    rng = np.random.default_rng(6500)
    fib = rng.integers(0, 256, (1, F, 4, 3, 30), dtype=np.uint8)
    pay = rng.integers(0, 256, (1, F, 4, nb), dtype=np.uint8)
    fib.tofile(tmp_path / "fib.bin"); pay.tofile(tmp_path / "pay.bin")
    iq = bank.transmit_frames_host(fib, pay, F).reshape(-1)
    P = params()
    table = FM.plan_stream(P, DOPPLER_HZ / 2.048e6, SEED, 0, [FM.FADING] * 6)
    got = cli(*SUB_ARGS, "--fib-file", tmp_path / "fib.bin", "--payload-file", tmp_path / "pay.bin", "--frames", F, *FADE_ARGS).reshape(-1, 2)
    assert np.array_equal(got, FM.host_apply(host, [P], [table], iq, 0, F * S, False, fmt=CM.U8, scale=U8_SCALE)[0])
    bank.close(); ctx.close()
