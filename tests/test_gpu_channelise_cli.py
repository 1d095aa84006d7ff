"""-m gpu: the channeliser's command-line flags.  dabgpu_simulate_transmitter --wideband 4 --centre-offset-hz 300000 --neighbour
+-1712000:20 writes bytes equal to the host models of the channel and of the combiner over the modulator's frames; with the flags absent,
or at their identity values, it writes today's bytes.  dabgpu_radio_cli --input-rate 8192000 --channel-offset-hz 300000 delivers from that
capture the FIB bodies and sub-channel bytes that were sent, and nothing at another offset.  A 10 MS/s capture (--wideband 4 behind
--output-rate 2500000) exercises channeliser + resampler together.  With --channel-offset-hz absent, or 0 at a rate below 4.096 MS/s, the
radio tool writes what it writes today."""
import math
import os
import subprocess

import numpy as np
import pytest

import channel_model as CHM
import channelise_model as CM
import tx_encode_cases as T
import tx_model as TX

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TX_CLI = os.path.join(ROOT, "dab-radio_amd", "host", "apps", "dabgpu_simulate_transmitter")
RX_CLI = os.path.join(ROOT, "dab-radio_amd", "host", "apps", "dabgpu_radio_cli")
S = 196608
SUBS = [dict(start=0, length=48, is_uep=0, uep_index=0, eep_level=2, eep_type=0), dict(start=201, length=16, is_uep=1, uep_index=0, eep_level=0, eep_type=0)]
SUB_ARGS = ["--subchannel", "0:48:eep3-A", "--subchannel", "201:16:uep0"]
RX_SUB_ARGS = ["--radio-subchannel", "0,48,3,A", "--radio-subchannel", "201,16,uep,0"]
N_FRAMES = 8
OFFSET_HZ, SPACING_HZ, LEVEL_DB = 300000.0, 1712000.0, 20.0


def tx(*args):
    res = subprocess.run([TX_CLI] + [str(a) for a in args], capture_output=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    return np.frombuffer(res.stdout, np.uint8)


def rx(*args):
    res = subprocess.run([RX_CLI] + [str(a) for a in args], capture_output=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    return res


def transmission(tmp_path, *flags):
    """(fib file, payload file, plan, what the tool wrote to its standard output)"""
    import dabgpu
    plan = dabgpu.tx_encode_plan([T.g_sub(dabgpu, d) for d in SUBS])
    nb = plan["cif_in_bytes"]
    rng = np.random.default_rng(6600)
    fib_file = rng.integers(0, 256, N_FRAMES * 360, dtype=np.uint8)
    pay_file = rng.integers(0, 256, N_FRAMES * 4 * nb, dtype=np.uint8)
    fib_file.tofile(tmp_path / "fib.bin"); pay_file.tofile(tmp_path / "pay.bin")
    u8 = tx(*SUB_ARGS, "--fib-file", tmp_path / "fib.bin", "--payload-file", tmp_path / "pay.bin", "--frames", N_FRAMES, "--snr-db", 20, *flags)
    return fib_file, pay_file, plan, u8


def check_delivery(tmp_path, prefix, fib_file, pay_file, plan):
    """every FIB that passed its CRC is a transmitted one, in order; the sub-channels' bytes are consecutive CIFs of the payload file"""
    nb = plan["cif_in_bytes"]
    sent = fib_file.reshape(N_FRAMES * 12, 30)
    got = np.fromfile(tmp_path / f"{prefix}fibs.bin", np.uint8).reshape(-1, 30)
    assert got.shape[0] >= 12 * (N_FRAMES - 3), got.shape
    starts = [s for s in range(0, 12 * 4, 12) if np.array_equal(sent[s], got[0])]
    assert starts and np.array_equal(got, sent[starts[0]:starts[0] + got.shape[0]])
    cifs = pay_file.reshape(N_FRAMES * 4, nb)
    for k, sp in enumerate(plan["subs"][:len(SUBS)]):
        rows = np.fromfile(tmp_path / f"{prefix}msc_{k}.bin", np.uint8).reshape(-1, sp.in_bytes)
        assert rows.shape[0] >= 4 * (N_FRAMES - 3) - 15, rows.shape
        want = cifs[:, sp.in_offset:sp.in_offset + sp.in_bytes]
        best = max(sum(int(np.array_equal(rows[r], want[c0 + r])) for r in range(rows.shape[0]) if c0 + r < want.shape[0]) for c0 in range(16))
        assert best >= rows.shape[0] - 4, (k, best, rows.shape[0])


WIDE_ARGS = ["--wideband", 4, "--centre-offset-hz", OFFSET_HZ, "--neighbour", f"{-SPACING_HZ}:{LEVEL_DB}", "--neighbour", f"{SPACING_HZ}:{LEVEL_DB}"]
TAPS = [(0, 1.0, 0.0), (200, 0.35, -0.35)]
CH_ARGS = ["--snr-db", "12", "--cfo-hz", "333", "--timing-offset", "37", "--tap", "0:1:0", "--tap", "200:0.35:-0.35", "--noise-seed", "9"]
U8_SCALE = float((np.float32(1.0) / np.float32(1536.0) * np.float32(4.0)) * np.float32(127.5))
DELAYS = (50001, 120007)


def channel_params():
    """what the tool derives from CH_ARGS (tests/test_gpu_channel_cli.py)"""
    h2 = sum(float(np.float32(re)) ** 2 + float(np.float32(im)) ** 2 for _, re, im in TAPS)
    sigma = np.float32(math.sqrt(1536.0 * h2 / (2.0 * 10.0 ** (12.0 / 10.0))))
    return CHM.params_dict(taps=TAPS, freq_q64=int(round(math.ldexp(333.0 / 2.048e6, 64))), start=37, seed=9, noise_sigma=float(sigma))


def test_transmitter_wideband_equals_the_host_models(oracle, tmp_path):
    """the reference frame through the channel and the combiner, two frames: the bytes are the host models' over the modulator's float frame
    -- the block at +300 kHz of an 8.192 MS/s capture, its own stream 50001 and 120007 samples late 1.712 MHz to either side and 20 dB up,
    the u8 scale leaving the sum four standard deviations of head room -- whatever the tool's block sizes; the last 143 samples wait for a third frame"""
    ch_host, cs_host = CHM.build_host_model(tmp_path), CM.build_host_model(tmp_path)
    frame = TX.modulate(oracle, 1, TX.scrambler_bytes(TX.payload_bytes(oracle, 1)), TX.LAYOUT_REFERENCE).astype(np.complex64)
    got = tx("--frames", 2, *CH_ARGS, *WIDE_ARGS).reshape(-1, 2)
    impaired = CHM.host_apply(ch_host, [channel_params()], frame, 0, 2 * S, True)[0]
    rows = np.zeros((3, 2 * S), np.complex64)
    rows[0] = impaired
    for k, d in enumerate(DELAYS):
        rows[1 + k, d:] = impaired[:-d]
    level = float(np.float32(10.0 ** (LEVEL_DB / 20.0)))
    chs = [CM.channel(CM.freq_q64(OFFSET_HZ, 8192000.0), 0, 1.0), CM.channel(CM.freq_q64(OFFSET_HZ - SPACING_HZ, 8192000.0), 0, level),
           CM.channel(CM.freq_q64(OFFSET_HZ + SPACING_HZ, 8192000.0), 0, level)]
    F = CM.host_design(cs_host, 4, 768000.0 / 2048000.0, 944000.0 / 2048000.0)
    n = 2 * S * 4 - CM.peak(4)
    scale = np.float32(min(U8_SCALE, 127.5 / (4.0 * math.sqrt(0.5 * 1536 * (1.0 + 2.0 * 10.0 ** (LEVEL_DB / 10.0))))))       # four sigma of head room
    exp = CM.host_combine(cs_host, chs, 1, F, rows, 0, 0, n, False, CM.U8, scale)[0]
    assert got.shape == exp.shape and np.array_equal(got, exp)


def test_transmitter_without_the_flags_and_with_their_identity_values_writes_the_same():
    plain = tx("--frames", 2)
    assert plain.size == 2 * 2 * S
    assert np.array_equal(tx("--frames", 2, "--wideband", 1), plain)                  # D = 1, no offset, no neighbour: the mixer's identity
    assert np.array_equal(tx("--frames", 2, "--wideband", 1, "--centre-offset-hz", 0), plain)
    with_channel = tx("--frames", 2, *CH_ARGS)
    assert np.array_equal(tx("--frames", 2, *CH_ARGS, "--wideband", 1), with_channel)
    coded = tx(*SUB_ARGS, "--seed", 4, "--frames", 3)
    assert np.array_equal(tx(*SUB_ARGS, "--seed", 4, "--frames", 3, "--wideband", 1), coded)
    assert tx("--frames", 1, "--wideband", 2).size == 2 * (2 * S - 71)                 # D x the samples, less the taps still to come
    for bad in (("--wideband", 0), ("--wideband", 9), ("--centre-offset-hz", 300000), ("--neighbour", "1712000:20"), ("--wideband", 4, "--neighbour", "1712000"),
                ("--wideband", 4, "--centre-offset-hz", 5000000), ("--wideband", 4, "--neighbour", "4200000:0"), ("--wideband", 8) + ("--neighbour", "0:0") * 8,
                ("--wideband", 1, "--output-rate", 1500000)):                # the neighbour's edge beyond the capture's Nyquist frequency
        assert subprocess.run([TX_CLI, "--frames", "1", *map(str, bad)], capture_output=True, timeout=300).returncode != 0


def test_transmitter_without_the_flags_writes_the_recorded_bytes():
    """tests/golden/simulate_transmitter_digests.json: digests of what the tool wrote before it had the wideband flags (plain, with a channel,
    channel coded); without the flags, and with --wideband 1, it still writes those bytes"""
    import hashlib
    import json
    runs = json.load(open(os.path.join(ROOT, "tests", "golden", "simulate_transmitter_digests.json")))["runs"]
    assert len(runs) == 3
    for run in runs:
        assert hashlib.sha256(tx(*run["args"]).tobytes()).hexdigest() == run["sha256"], run["args"]
        assert hashlib.sha256(tx(*run["args"], "--wideband", 1).tobytes()).hexdigest() == run["sha256"], run["args"]


def test_block_out_of_an_8192000_capture_with_neighbours_delivers_what_was_sent(tmp_path):
    capture = tmp_path / "capture_8192000.u8"
    fib_file, pay_file, plan, wide = transmission(tmp_path, *WIDE_ARGS, "-o", capture)
    assert os.path.getsize(capture) == 2 * (N_FRAMES * S * 4 - CM.peak(4))
    res = rx("-i", capture, "--input-rate", 8192000, "--channel-offset-hz", OFFSET_HZ,
             "--radio-fib-output", tmp_path / "a_fibs.bin", "--radio-msc-output", tmp_path / "a_msc_", *RX_SUB_ARGS)
    assert b"decimation 4" in res.stderr
    check_delivery(tmp_path, "a_", fib_file, pay_file, plan)
    # the same capture tuned half a block away delivers nothing
    rx("-i", capture, "--input-rate", 8192000, "--channel-offset-hz", OFFSET_HZ + 856000.0,
       "--radio-fib-output", tmp_path / "w_fibs.bin", "--radio-msc-output", tmp_path / "w_msc_", *RX_SUB_ARGS)
    assert os.path.getsize(tmp_path / "w_fibs.bin") == 0


def test_a_10000000_capture_goes_through_channeliser_and_resampler(tmp_path):
    """--wideband 4 behind --output-rate 2500000 writes 10 MS/s; the radio tool splits by 4 and resamples 2.5 -> 2.048 MS/s"""
    capture = tmp_path / "capture_10000000.u8"
    fib_file, pay_file, plan, _ = transmission(tmp_path, "--output-rate", 2500000, *WIDE_ARGS, "-o", capture)
    assert abs(os.path.getsize(capture) / 2 - N_FRAMES * S * 4 * 2.5 / 2.048) < 0.001 * N_FRAMES * S * 4
    res = rx("-i", capture, "--input-rate", 10000000, "--channel-offset-hz", OFFSET_HZ,
             "--radio-fib-output", tmp_path / "b_fibs.bin", "--radio-msc-output", tmp_path / "b_msc_", *RX_SUB_ARGS)
    assert b"decimation 4, 2500000 samples per second" in res.stderr
    check_delivery(tmp_path, "b_", fib_file, pay_file, plan)


def test_radio_cli_without_the_flag_writes_what_it_wrote(tmp_path):
    capture = tmp_path / "capture.u8"
    tx(*SUB_ARGS, "--seed", 11, "--frames", 6, "--snr-db", 20, "--timing-offset", 5, "-o", capture)
    outs = []
    for k, extra in enumerate(((), ("--channel-offset-hz", 0), ("--channel-offset-hz", 0, "--input-rate", 2048000))):
        res = rx("-i", capture, *extra, "--ofdm-enable-output", "--ofdm-output", tmp_path / f"bits{k}.bin", "--radio-fib-output", tmp_path / f"fibs{k}.bin",
                 "--radio-msc-output", tmp_path / f"m{k}_", *RX_SUB_ARGS)
        outs.append([(tmp_path / name).read_bytes() for name in (f"bits{k}.bin", f"fibs{k}.bin", f"m{k}_0.bin", f"m{k}_1.bin")] + [res.stderr])
    assert outs[0] == outs[1] == outs[2] and len(outs[0][0]) >= 4 * 230400 and len(outs[0][1]) >= 30 * 12 * 4
    for bad in (("--channel-offset-hz", 2000000), ("--channel-offset-hz", 5000000, "--input-rate", 8192000), ("--channel-offset-hz", 1, "--input-rate", 40000000),
                ("--channel-offset-hz", 300000, "--input-rate", 8192000, "--tii")):
        assert subprocess.run([RX_CLI, "-i", str(capture), *map(str, bad)], capture_output=True, timeout=300).returncode != 0
