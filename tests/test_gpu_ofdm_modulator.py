"""-m gpu: the OFDM transmitter on the device (dabgpu_ofdm_modulate_frames, dab-radio_amd/csrc/ofdm_mod.hip), its OFDM_Modulator mirror
class and dabgpu_simulate_transmitter, bit for bit against the oracle (mode I: its restatements of OFDM_Modulator::ProcessBlock and of
the frequency-interleaved transmitter; modes II-IV: the composition of tests/tx_model.py, itself pinned to the oracle by
tests/test_tx_model.py)."""
import os
import subprocess

import numpy as np
import pytest

import tx_model as TX

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dab-radio_amd", "host")
LIBDIR = os.path.join(ROOT, "dab-radio_amd")
CLI = os.path.join(HOST, "apps", "dabgpu_simulate_transmitter")


def u32(x):
    return np.ascontiguousarray(x, dtype=np.complex64).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


def formats():
    import dabgpu
    return dabgpu.IQ_FORMATS.index("raw_f32l"), dabgpu.IQ_FORMATS.index("raw_u8")


def modulate_device(ctx, mode, payload, n, layout, fmt=None, freq_norm=0.0, prs=None):
    """payload [n][bytes] numpy -> numpy frames via device buffers (complex64 [n][samples] or uint8 [n][2 * samples])"""
    import torch
    import dabgpu
    f32, u8 = formats()
    fmt = f32 if fmt is None else fmt
    S = dabgpu.ofdm_params(mode)["nb_frame_samples"]
    d_pay = torch.from_numpy(np.ascontiguousarray(payload, np.uint8).reshape(-1)).cuda()
    d_prs = None if prs is None else torch.from_numpy(np.ascontiguousarray(prs, np.complex64).view(np.float32)).cuda()
    if fmt == f32:
        out = torch.empty((n, 2 * S), dtype=torch.float32, device="cuda")
    else:
        out = torch.empty((n, 2 * S), dtype=torch.uint8, device="cuda")
    ctx.ofdm_modulate_frames(mode, d_pay, n, out, layout=layout, out_format=fmt, prs_fft_ref=d_prs, freq_norm=freq_norm)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    return h.view(np.complex64) if fmt == f32 else h


@pytest.mark.parametrize("n", [1, 5, 257])
def test_mode1_reference_payload_f32_bit_exact(oracle, ctx, n):
    rng = np.random.default_rng(4100 + n)
    pay = rng.integers(0, 256, (n, TX.payload_bytes(oracle, 1)), dtype=np.uint8)
    got = modulate_device(ctx, 1, pay, n, TX.LAYOUT_REFERENCE)
    for k in range(n):
        exp = oracle.modulate_frame_reference_payload(pay[k])
        assert np.array_equal(u32(got[k]), u32(exp)), f"frame {k} of {n}"


@pytest.mark.parametrize("mode,layout", [(1, 1), (2, 0), (2, 1), (3, 0), (3, 1), (4, 0), (4, 1)])
def test_modes_and_layouts_bit_exact(oracle, ctx, mode, layout):
    rng = np.random.default_rng(4200 + 10 * mode + layout)
    n = 3
    pay = rng.integers(0, 256, (n, TX.payload_bytes(oracle, mode)), dtype=np.uint8)
    got = modulate_device(ctx, mode, pay, n, layout)
    for k in range(n):
        if mode == 1:
            exp = oracle.modulate_frame(np.unpackbits(pay[k], bitorder="little"))
        else:
            exp = TX.modulate(oracle, mode, pay[k], layout)
        assert np.array_equal(u32(got[k]), u32(exp)), f"mode {mode} layout {layout} frame {k}"


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_round_trip_through_the_demodulator(oracle, ctx, mode):
    """hard bytes -> FRAME_BITS modulation -> frame-buffer layout -> dabgpu_ofdm_demod_frames_mode -> hard bytes: the same bytes"""
    import torch
    import dabgpu
    g = dabgpu.ofdm_params(mode)
    n = 4
    rng = np.random.default_rng(4300 + mode)
    pay = rng.integers(0, 256, (n, g["nb_frame_bits"] // 8), dtype=np.uint8)
    tx = modulate_device(ctx, mode, pay, n, TX.LAYOUT_FRAME_BITS)
    fb = np.stack([TX.to_frame_buffer(oracle, mode, tx[k]) for k in range(n)])
    d_iq = torch.from_numpy(np.ascontiguousarray(fb).view(np.float32)).cuda()
    d_bits = torch.empty((n, g["nb_frame_bits"]), dtype=torch.int8, device="cuda")
    d_bytes = torch.empty((n, g["nb_frame_bits"] // 8), dtype=torch.uint8, device="cuda")
    ctx.ofdm_demod_frames_mode(mode, d_iq, n, d_bits)
    ctx.soft_bits_to_hard_bytes(d_bits, n * g["nb_frame_bits"] // 8, d_bytes)
    torch.cuda.synchronize()
    assert np.array_equal(d_bytes.cpu().numpy(), pay)


@pytest.mark.parametrize("hz", [0.0, 1000.0, -2500.0])
def test_u8_with_frequency_shift(oracle, ctx, hz):
    _, u8 = formats()
    rng = np.random.default_rng(4400 + int(abs(hz)))
    n = 3
    f = TX.freq_norm(hz)
    for mode in (1, 3):
        g = oracle.geometry(mode)
        pay = rng.integers(0, 256, (n, TX.payload_bytes(oracle, mode)), dtype=np.uint8)
        got = modulate_device(ctx, mode, pay, n, TX.LAYOUT_REFERENCE, fmt=u8, freq_norm=f)
        for k in range(n):
            frame = oracle.modulate_frame_reference_payload(pay[k]) if mode == 1 else TX.modulate(oracle, mode, pay[k], TX.LAYOUT_REFERENCE)
            assert np.array_equal(got[k], TX.quantise_u8(oracle, frame, f, g.nb_carriers)), f"mode {mode} {hz} Hz frame {k}"
    if hz != 0.0:
        # the shift applies to complex float output too: apply_pll of the unshifted frame, phase 0 at each frame's first sample
        pay = rng.integers(0, 256, (2, TX.payload_bytes(oracle, 1)), dtype=np.uint8)
        got = modulate_device(ctx, 1, pay, 2, TX.LAYOUT_REFERENCE, freq_norm=f)
        for k in range(2):
            exp = oracle.apply_pll(oracle.modulate_frame_reference_payload(pay[k]), f)
            assert np.array_equal(u32(got[k]), u32(exp))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(HOST, "libdab_mirror.a")) or not os.path.exists(CLI):
        g.build()
    exe = str(tmp_path_factory.mktemp("tx_harness") / "tx_mirror_harness")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + HOST, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "tx_mirror_harness.cpp"), os.path.join(HOST, "libdab_mirror.a"),
                           "-L" + LIBDIR, "-ldabgpu", "-Wl,-rpath," + LIBDIR, "-o", exe])
    return exe


def run_harness(exe, tmp_path, mode, payload, prs=None):
    pf, of = tmp_path / f"pay{mode}.bin", tmp_path / f"out{mode}.bin"
    pf.write_bytes(np.ascontiguousarray(payload, np.uint8).tobytes())
    prs_arg = "-"
    if prs is not None:
        prs_arg = str(tmp_path / f"prs{mode}.bin")
        open(prs_arg, "wb").write(np.ascontiguousarray(prs, np.complex64).tobytes())
    res = subprocess.run([exe, str(mode), str(pf), prs_arg, str(of)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return np.fromfile(str(of), dtype=np.complex64)


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_mirror_class_bit_exact(oracle, harness, tmp_path, mode):
    rng = np.random.default_rng(4500 + mode)
    pay = rng.integers(0, 256, TX.payload_bytes(oracle, mode), dtype=np.uint8)
    got = run_harness(harness, tmp_path, mode, pay)                  # (the harness also checks the short-size refusals)
    exp = oracle.modulate_frame_reference_payload(pay) if mode == 1 else TX.modulate(oracle, mode, pay, TX.LAYOUT_REFERENCE)
    assert np.array_equal(u32(got), u32(exp))


@pytest.mark.parametrize("mode", [1, 3])
def test_mirror_class_uses_the_callers_prs(oracle, harness, tmp_path, mode):
    g = oracle.geometry(mode)
    prs = oracle.prs_fft_mode(mode).copy()
    b = int(TX.carrier_bins(g.nb_fft, g.nb_carriers)[7])
    prs[b] = np.complex64(prs[b] * np.complex64(0.5 - 0.25j))
    rng = np.random.default_rng(4600 + mode)
    pay = rng.integers(0, 256, TX.payload_bytes(oracle, mode), dtype=np.uint8)
    got = run_harness(harness, tmp_path, mode, pay, prs=prs)
    exp = TX.modulate(oracle, mode, pay, TX.LAYOUT_REFERENCE, prs=prs)
    assert np.array_equal(u32(got), u32(exp))
    assert not np.array_equal(u32(got), u32(TX.modulate(oracle, mode, pay, TX.LAYOUT_REFERENCE)))


def run_cli(*args):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = LIBDIR + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    res = subprocess.run([CLI, *[str(a) for a in args]], capture_output=True, env=env, timeout=300)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    return res.stdout


def expected_cli_frame(oracle, mode, hz):
    g = oracle.geometry(mode)
    pay = TX.scrambler_bytes(TX.payload_bytes(oracle, mode))
    frame = TX.modulate(oracle, mode, pay, TX.LAYOUT_REFERENCE)
    return TX.quantise_u8(oracle, frame, TX.freq_norm(hz) if hz != 0 else 0.0, g.nb_carriers)


def test_simulate_transmitter_cli(oracle, harness, tmp_path):
    out = tmp_path / "tx.u8"
    run_cli("-m", 1, "-f", 1000, "--frames", 3, "-o", out)
    exp = expected_cli_frame(oracle, 1, 1000.0)
    assert np.array_equal(np.fromfile(str(out), np.uint8), np.tile(exp, 3))
    got = np.frombuffer(run_cli("-m", 2, "--frames", 2), np.uint8)
    assert np.array_equal(got, np.tile(expected_cli_frame(oracle, 2, 0.0), 2))


def test_mode1_4096_frames_async_with_guard(oracle, ctx):
    import torch
    n = 4096
    nb = TX.payload_bytes(oracle, 1)
    S = oracle.geometry(1).nb_frame_samples
    rng = np.random.default_rng(4700)
    pay = rng.integers(0, 256, (n, nb), dtype=np.uint8)
    d_pay = torch.from_numpy(pay.reshape(-1)).cuda()
    guard = 4096 // 4
    buf = torch.empty(n * 2 * S + guard, dtype=torch.float32, device="cuda")
    bits = ((np.arange(guard, dtype=np.uint64) * 2654435761) & 0x3FFFFFFF | 1).astype(np.int32)      # (finite floats: no NaN payloads)
    pattern = torch.from_numpy(bits.view(np.float32)).cuda()
    buf[n * 2 * S:] = pattern
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        ctx.ofdm_modulate_frames(1, d_pay, n, buf, layout=TX.LAYOUT_REFERENCE, stream=s.cuda_stream)
    s.synchronize()                                                   # the results are read behind the stream's synchronise only
    assert torch.equal(buf[n * 2 * S:].view(torch.int32), pattern.view(torch.int32)), "the guard region after d_out was written"
    frames = buf[:n * 2 * S].view(n, 2 * S)
    for k in (0, 1, 511, 1024, 2047, 2048, 3333, n - 1):
        got = frames[k].cpu().numpy().view(np.complex64)
        assert np.array_equal(u32(got), u32(oracle.modulate_frame_reference_payload(pay[k]))), f"frame {k}"
