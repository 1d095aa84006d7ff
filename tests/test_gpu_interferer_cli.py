"""-m gpu: the interferer through the tools.  dabgpu_simulate_transmitter --interferer ...: the bytes equal channel host model + interferer
host model + quantiser for a tone, a band and a gated white source, and without the options they are what they were.  A channel-coded
capture with the band source of tests/interferer_loop.py (96 kHz wide, 300 kHz above the centre, I / S = 0 dB, SNR 12 dB) through
dabgpu_radio_cli: with --soft-bits banded the FIBs and sub-channel bytes that were sent, with --soft-bits csi fewer than half the FIBs;
on a capture made without the interferer options both deliver, as they did."""
import math
import os
import subprocess

import numpy as np
import pytest

import channel_loop as CL
import channel_model as CM
import interferer_loop as IL
import interferer_model as IM
import tx_encode_cases as T
import tx_model as TX

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM = os.path.join(ROOT, "dab-radio_amd", "host", "apps", "dabgpu_simulate_transmitter")
RADIO = os.path.join(ROOT, "dab-radio_amd", "host", "apps", "dabgpu_radio_cli")
S = 196608
TAPS = [(0, 1.0, 0.0), (200, 0.35, -0.35)]
CH_ARGS = ["--snr-db", "12", "--cfo-hz", "333", "--timing-offset", "37", "--tap", "0:1:0", "--tap", "200:0.35:-0.35", "--noise-seed", "9"]
U8_SCALE = float((np.float32(1.0) / np.float32(1536.0) * np.float32(4.0)) * np.float32(127.5))
H2 = sum(float(np.float32(re)) ** 2 + float(np.float32(im)) ** 2 for _, re, im in TAPS)
SUB_ARGS = ["--subchannel", "0:48:eep3-A", "--subchannel", "200:52:uep20"]      # tests/channel_loop.py's SUBS
N_FRAMES = 8


def sim(*args):
    res = subprocess.run([SIM] + [str(a) for a in args], capture_output=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    return np.frombuffer(res.stdout, np.uint8)


def channel_params():
    sigma = np.float32(math.sqrt(1536.0 * H2 / (2.0 * 10.0 ** (12.0 / 10.0))))
    return CM.params_dict(taps=TAPS, freq_q64=int(round(math.ldexp(333.0 / 2.048e6, 64))), start=37, seed=9, noise_sigma=float(sigma))


def amp(is_db, h2=H2):
    """what the tool derives (its --help): IS_DB relative to the signal power 1536 x sum |tap|^2 of --snr-db"""
    return float(np.float32(math.sqrt(1536.0 * h2 * 10.0 ** (is_db / 10.0))))


def word(hz):
    import dabgpu
    return int(dabgpu.lib().dabgpu_channel_freq_q64(hz / 2.048e6))


CASES = {
    "tone": (["--interferer", "tone:-123456.5:-3", "--interferer-seed", "77"],
             lambda: ([IM.source(IM.TONE, amp=amp(-3.0), freq_q64=word(-123456.5))], [])),
    "band": (["--interferer", "band:300000:96000:0", "--interferer-seed", "77"],
             lambda: ([IM.source(IM.BAND, amp=amp(0.0), shape=0, freq_q64=word(300000.0))], [96000.0])),
    "bursts_and_more": (["--interferer", "white:17", "--interferer-gate", "20480:205:-1000", "--interferer", "band:-500000:16000:-6", "--interferer-gate", "3000:3000",
                         "--interferer", "tone:250:-10", "--interferer", "band:0:1200000:-20", "--interferer-seed", "77"],
                        lambda: ([IM.source(IM.BAND, amp=amp(17.0), shape=-1, gate_period=20480, gate_on=205, gate_offset=-1000),
                                  IM.source(IM.BAND, amp=amp(-6.0), shape=0, freq_q64=word(-500000.0), gate_period=3000, gate_on=3000),
                                  IM.source(IM.TONE, amp=amp(-10.0), freq_q64=word(250.0)),
                                  IM.source(IM.BAND, amp=amp(-20.0), shape=1, freq_q64=0)], [16000.0, 1200000.0])),
}


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp("interferer_cli")
    return CM.build_host_model(d), IM.build_host_model(d)


@pytest.fixture(scope="module")
def clean_frames(oracle, hosts):
    """the reference's frame through the channel of CH_ARGS, two frames, complex float: the existing expectation of the tool's channel"""
    frame = TX.modulate(oracle, 1, TX.scrambler_bytes(TX.payload_bytes(oracle, 1)), TX.LAYOUT_REFERENCE).astype(np.complex64)
    return frame, CM.host_apply(hosts[0], [channel_params()], frame, 0, 2 * S, True)[0]


def test_without_the_options_the_bytes_are_what_they_were(hosts, clean_frames):
    frame, rx = clean_frames
    plain = sim("--frames", 2)
    assert np.array_equal(sim("--frames", 2, "--interferer-seed", 5), plain)                  # a seed makes no interferer and no channel
    exp = CM.host_apply(hosts[0], [channel_params()], frame, 0, 2 * S, True, fmt=CM.U8, scale=U8_SCALE)[0]
    assert np.array_equal(sim("--frames", 2, *CH_ARGS).reshape(-1, 2), exp)                   # tests/test_gpu_channel_cli.py's expectation
    assert np.array_equal(sim("--frames", 2, *CH_ARGS, "--interferer-seed", 5).reshape(-1, 2), exp)
    res = subprocess.run([SIM, "--frames", "1", "--interferer-gate", "10:5"], capture_output=True, timeout=60)
    assert res.returncode != 0 and b"--interferer before it" in res.stderr
    res = subprocess.run([SIM, "--frames", "1"] + ["--interferer", "tone:0:0"] * 5, capture_output=True, timeout=60)
    assert res.returncode != 0 and b"at most 4" in res.stderr
    res = subprocess.run([SIM, "--frames", "1", "--interferer", "band:0:100:0"], capture_output=True, timeout=60)
    assert res.returncode != 0 and b"width_cycles" in res.stderr


@pytest.mark.parametrize("case", list(CASES))
def test_bytes_equal_channel_plus_interferer_host_models(hosts, clean_frames, case):
    import dabgpu
    args, make = CASES[case]
    sources, widths = make()
    shapes = [IM.Shape.from_buffer_copy(bytes(dabgpu.interferer_design(w / 2.048e6))) for w in widths]
    got = sim("--frames", 2, *CH_ARGS, *args).reshape(-1, 2)
    exp = IM.host_apply(hosts[1], [IM.stream(sources, seed=77)], shapes, clean_frames[1], 0, 2 * S, IM.U8, U8_SCALE)[0]
    assert np.array_equal(got, exp)
    clean = CM.host_apply(hosts[0], [channel_params()], clean_frames[0], 0, 2 * S, True, fmt=CM.U8, scale=U8_SCALE)[0]
    assert not np.array_equal(got, clean)


def radio(capture, out_dir, *extra):
    res = subprocess.run([RADIO, "-i", str(capture), "--radio-fib-output", str(out_dir / "fib.bin"), "--radio-msc-output", str(out_dir / "sub_"),
                          "--radio-subchannel", "0,48,3,A", "--ofdm-block-size", "65536"] + [str(a) for a in extra], capture_output=True, timeout=300)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    return (out_dir / "fib.bin").read_bytes(), (out_dir / "sub_0.bin").read_bytes(), res.stderr.decode()


def sent_between(fib, cifs, a, b):
    """what a receiver that delivers the frames a .. b - 1 hands out: their FIBs and the sub-channel's CIFs 4 a .. 4 b less the 15 the time
    de-interleaver holds back"""
    return fib[a:b].tobytes(), cifs[4 * a:4 * b - 15].tobytes()


def test_capture_through_the_radio_banded_delivers_csi_does_not(oracle, tmp_path):
    fib, pay, nb = CL.inputs(oracle)
    n0 = oracle.subchannel_plan(T.o_sub(oracle, CL.SUBS[0]))[2]
    fib.tofile(tmp_path / "fib_in.bin"); pay.tofile(tmp_path / "pay_in.bin")
    # the files are read cyclically: frame j carries the FIBs and the payload of frame j mod 5
    fibs = np.concatenate([fib[0].reshape(CL.N_FRAMES, -1)] * 2)[:N_FRAMES]
    cifs = np.concatenate([pay[0].reshape(4 * CL.N_FRAMES, nb)[:, :n0]] * 2)[:4 * N_FRAMES]
    common = [*SUB_ARGS, "--fib-file", tmp_path / "fib_in.bin", "--payload-file", tmp_path / "pay_in.bin", "--frames", N_FRAMES, "--snr-db", IL.SNR_DB,
              "--noise-seed", 9]
    jam = ["--interferer", f"band:{IL.OFFSET_HZ:.0f}:{IL.WIDTH_HZ:.0f}:{IL.POINT_DB:.0f}", "--interferer-seed", 77]
    for name, extra in (("clean", []), ("jammed", jam)):
        sim(*common, *extra, "-o", tmp_path / f"{name}.u8")
        (tmp_path / name).mkdir()
    # the tool may spend a frame or two acquiring, and the last frame is not delivered: no NULL follows it in the file
    expected = [sent_between(fibs, cifs, a, b) for a in range(3) for b in (N_FRAMES - 1, N_FRAMES)]
    # the capture made with the options absent: every policy delivers, as before
    for policy in (["--soft-bits", "csi"], ["--soft-bits", "banded"], []):
        got_fib, got_msc, log = radio(tmp_path / "clean.u8", tmp_path / "clean", *policy)
        assert (got_fib, got_msc) in expected, (policy, len(got_fib) // 30, len(got_msc) // n0, log)
    got_fib, got_msc, log = radio(tmp_path / "jammed.u8", tmp_path / "jammed", "--soft-bits", "banded")
    print(f"banded: {len(got_fib) // 30} FIBs, {len(got_msc) // n0} CIFs; {log.strip().splitlines()[-3:]}")
    assert (got_fib, got_msc) in expected
    assert "frames_kept_csi=0" in log
    csi_fib, csi_msc, log = radio(tmp_path / "jammed.u8", tmp_path / "jammed", "--soft-bits", "csi")
    print(f"csi: {len(csi_fib) // 30} FIBs; {log.strip().splitlines()[-2:]}")
    assert len(csi_fib) // 30 < 6 * N_FRAMES and csi_msc != got_msc
    again, _, _ = radio(tmp_path / "jammed.u8", tmp_path / "jammed", "--soft-bits", "banded", "--alpha", 1.0, "--soft-level", 64)
    assert again == got_fib


def test_banded_option_rules(tmp_path):
    np.zeros(8192, np.uint8).tofile(tmp_path / "iq.u8")
    for extra, text in ((["--alpha", "0.5"], b"--alpha needs --soft-bits banded"), (["--soft-bits", "banded", "--alpha", "0"], b"--alpha"),
                        (["--soft-bits", "banded", "--alpha", "1.5"], b"--alpha"), (["--soft-bits", "banded", "--alpha", "nan"], b"--alpha"),
                        (["--soft-bits", "banded", "--ofdm-block-size", "193953"], b"193952"),
                        (["--soft-bits", "banded", "--input-rate", "2400000"], b"--input-rate is not available"),
                        (["--soft-bits", "banded", "--input-rate", "8192000", "--channel-offset-hz", "1000"], b"--channel-offset-hz is not available")):
        res = subprocess.run([RADIO, "-i", str(tmp_path / "iq.u8")] + extra, capture_output=True, timeout=60)
        assert res.returncode != 0 and text in res.stderr, (extra, res.stderr[-500:])
