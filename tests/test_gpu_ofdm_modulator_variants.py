"""-m gpu: the transmitter kernels of dab-radio_amd/csrc/ofdm_mod.hip where tests/test_gpu_ofdm_modulator.py does not go: all sixteen
template instantiations (mode I / modes II-IV x output format x payload layout x frequency shift) at one and at several symbols per run,
payload patterns, the u8 clamps and the NaN rule, frequency shifts up to just under half a cycle per sample, the host-sync form with
several frames, and a 4 KiB guard pattern on both sides of d_out in every device call.  Expectations are the oracle's mode I
restatements and tests/tx_model.py, followed by oracle.apply_pll and TX.quantise_u8 -- all of them held to a float64 model written from
the standard by tests/test_independent_pins.py -- and compared as bit patterns.

The run length (symbols per workgroup) is a launch decision that the library reads once per process from DABGPU_TX_SPB, so the series
over run lengths starts tests/tx_variants_child.py as a fresh process per run length, one at a time, each under its own time limit.  A
child that ends on a signal or runs into its limit ends the series: every later device call of this module fails at once without
touching the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tx_model as TX
import tx_variants_child as CH

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = CH.GUARD
CHILD_TIMEOUT_S = 120                          # a child runs for two or three seconds; the limit covers a cold start of the runtime
DEAD = []                                      # reason, once a child ended on a signal or a time limit


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


def expected_frame(oracle, mode, pay, layout, prs=None):
    """the unshifted complex float frame: mode I with the built-in PRS from the oracle's own restatements, else tests/tx_model.py"""
    if mode == 1 and prs is None:
        if layout == TX.LAYOUT_REFERENCE:
            return oracle.modulate_frame_reference_payload(pay)
        return oracle.modulate_frame(np.unpackbits(np.ascontiguousarray(pay, np.uint8), bitorder="little"))
    return TX.modulate(oracle, mode, pay, layout, prs=prs)


def expected_output(oracle, mode, frame, is_u8, f):
    """what d_out holds for one frame: uint8 [2 * samples], or the complex floats as uint32 [2 * samples]"""
    if is_u8:
        return TX.quantise_u8(oracle, frame, f, oracle.geometry(mode).nb_carriers)
    return u32(oracle.apply_pll(frame, np.float32(f)) if np.float32(f) != 0 else frame)


def as_output(rows, is_u8):
    return rows if is_u8 else np.ascontiguousarray(rows).view(np.uint32)


def check_guards(front, back, what):
    pattern = CH.guard_pattern()
    assert np.array_equal(front, pattern), f"{what}: the {GUARD} bytes in front of d_out were written"
    assert np.array_equal(back, pattern), f"{what}: the {GUARD} bytes behind d_out were written"


def device_modulate(ctx, oracle, mode, pay, n, layout, is_u8=False, freq_norm=0.0, prs=None, keep=None):
    """every device call of this module: n payloads -> the frames `keep` (default all) of d_out as [len(keep)][bytes per frame] uint8,
    d_out between two guard patterns that are compared after the synchronise and pre-filled with 0xA5 (no stale result of an earlier
    call can stand in for a sample that was not written)"""
    if DEAD:
        pytest.fail(f"not run: {DEAD[0]}")
    import torch
    f32, u8 = formats()
    S = oracle.geometry(mode).nb_frame_samples
    bpf = S * (2 if is_u8 else 8)
    buf = torch.full((2 * GUARD + n * bpf,), 0xA5, dtype=torch.uint8, device="cuda")
    pattern = torch.from_numpy(CH.guard_pattern()).cuda()
    buf[:GUARD] = pattern
    buf[GUARD + n * bpf:] = pattern
    out = buf[GUARD:GUARD + n * bpf]
    assert (buf.data_ptr() + GUARD) % 16 == 0
    d_pay = torch.from_numpy(np.ascontiguousarray(pay, np.uint8).reshape(-1)).cuda()
    d_prs = None if prs is None else torch.from_numpy(np.ascontiguousarray(prs, np.complex64).view(np.float32)).cuda()
    ctx.ofdm_modulate_frames(mode, d_pay, n, buf.data_ptr() + GUARD, layout=layout, out_format=u8 if is_u8 else f32, prs_fft_ref=d_prs,
                             freq_norm=float(freq_norm))
    torch.cuda.synchronize()
    check_guards(buf[:GUARD].cpu().numpy(), buf[GUARD + n * bpf:].cpu().numpy(), f"mode {mode} n {n} layout {layout} u8 {is_u8} f {freq_norm}")
    if n == 0:
        return np.zeros((0, bpf), np.uint8)
    rows = out.view(n, bpf)
    keep = list(range(n)) if keep is None else list(keep)
    return rows[torch.tensor(keep, device="cuda")].cpu().numpy()


# ---- the launcher's own run length: batches that give several symbols per run on any device of up to 300 compute units --------------
@pytest.mark.parametrize("layout", [TX.LAYOUT_REFERENCE, TX.LAYOUT_FRAME_BITS])
@pytest.mark.parametrize("mode", [2, 3, 4])
def test_modes_2_to_4_with_64_frames(oracle, ctx, mode, layout):
    """8 x CUs / 64 <= 38 runs per frame of 76 or 153 symbols: at least two symbols per run"""
    assert "DABGPU_TX_SPB" not in os.environ, "this test is about the launcher's own choice of the run length"
    n = 64
    rng = np.random.default_rng(5100 + 10 * mode + layout)
    pay = rng.integers(0, 256, (n, TX.payload_bytes(oracle, mode)), dtype=np.uint8)
    keep = [0, 1, n // 2, n - 1]
    got = device_modulate(ctx, oracle, mode, pay, n, layout, keep=keep)
    for row, k in zip(got, keep):
        assert np.array_equal(as_output(row, False), u32(expected_frame(oracle, mode, pay[k], layout))), f"frame {k}"


@pytest.mark.parametrize("n", [257, 4096])
def test_mode1_frame_bits_with_many_frames(oracle, ctx, n):
    """257 frames: about ten symbols per run (replay, the two byte loads per carrier one symbol ahead); 4096: one run per frame"""
    assert "DABGPU_TX_SPB" not in os.environ, "this test is about the launcher's own choice of the run length"
    rng = np.random.default_rng(5200 + n)
    pay = rng.integers(0, 256, (n, TX.payload_bytes(oracle, 1)), dtype=np.uint8)
    keep = sorted(set([0, 1, 2, n // 3, n // 2, n // 2 + 1, n - 2, n - 1] + list(range(5, n, 509 if n > 1000 else 31))))
    got = device_modulate(ctx, oracle, 1, pay, n, TX.LAYOUT_FRAME_BITS, keep=keep)
    for row, k in zip(got, keep):
        assert np.array_equal(as_output(row, False), u32(expected_frame(oracle, 1, pay[k], TX.LAYOUT_FRAME_BITS))), f"frame {k} of {n}"


# ---- edges of value ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [TX.LAYOUT_REFERENCE, TX.LAYOUT_FRAME_BITS])
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_payload_patterns(oracle, ctx, mode, layout):
    """all 0x00, all 0xFF, 0x1B repeated (the four phases in every byte), a random payload and its copy with the last bit of the last
    symbol flipped: that bit changes the last symbol and nothing before it"""
    g = oracle.geometry(mode)
    nb = TX.payload_bytes(oracle, mode)
    rng = np.random.default_rng(5300 + 10 * mode + layout)
    pay = np.stack([np.zeros(nb, np.uint8), np.full(nb, 0xFF, np.uint8), np.full(nb, 0x1B, np.uint8),
                    rng.integers(0, 256, nb, dtype=np.uint8), np.zeros(nb, np.uint8)])
    pay[4] = pay[3]
    pay[4, -1] ^= 0x80
    got = as_output(device_modulate(ctx, oracle, mode, pay, 5, layout), False)
    for k in range(5):
        assert np.array_equal(got[k], u32(expected_frame(oracle, mode, pay[k], layout))), f"payload {k}"
    last = 2 * (g.nb_frame_samples - g.nb_symbol_period)
    assert np.array_equal(got[3][:last], got[4][:last])
    assert not np.array_equal(got[3][last:], got[4][last:])
    assert len({got[k].tobytes() for k in range(4)}) == 4                # (four payloads, four frames)


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_u8_clamps_at_both_ends(oracle, ctx, mode, shifted):
    """a caller's PRS of 8 sqrt(NC / 1536) x the built-in one: samples of 74 counts rms around 127.5 in every mode (a sample is a sum of NC
    unit carriers, the scale is 4 / NC x 127.5), so that both clamps of tx_u8 work and most samples still pass unclamped (asserted on the
    expectation, so the case cannot go vacuous)"""
    g = oracle.geometry(mode)
    prs = (oracle.prs_fft_mode(mode) * np.float32(8.0 * np.sqrt(g.nb_carriers / 1536.0))).astype(np.complex64)
    f = TX.SERIES_SHIFT if shifted else 0.0
    rng = np.random.default_rng(5400 + 10 * mode + shifted)
    pay = rng.integers(0, 256, (2, TX.payload_bytes(oracle, mode)), dtype=np.uint8)
    got = device_modulate(ctx, oracle, mode, pay, 2, TX.LAYOUT_REFERENCE, is_u8=True, freq_norm=f, prs=prs)
    for k in range(2):
        exp = expected_output(oracle, mode, expected_frame(oracle, mode, pay[k], TX.LAYOUT_REFERENCE, prs=prs), True, f)
        assert (exp == 0).mean() > 0.01 and (exp == 255).mean() > 0.01 and ((exp > 0) & (exp < 255)).mean() > 0.5
        assert np.array_equal(got[k], exp), f"frame {k}: {int((got[k] != exp).sum())} samples differ"


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_u8_nan_carrier_gives_zero(oracle, ctx, mode, shifted):
    """QuantisedIQ<uint8_t>::from_iq clamps with comparisons that a NaN fails: a NaN becomes 0.  One NaN data carrier in the caller's PRS
    reaches every sample of every symbol through the transform (and every later symbol through the chain); the NULL period stays 127"""
    g = oracle.geometry(mode)
    prs = oracle.prs_fft_mode(mode).copy()
    prs[int(TX.carrier_bins(g.nb_fft, g.nb_carriers)[11])] = np.complex64(complex(np.nan, np.nan))
    rng = np.random.default_rng(5500 + mode)
    pay = rng.integers(0, 256, (2, TX.payload_bytes(oracle, mode)), dtype=np.uint8)
    got = device_modulate(ctx, oracle, mode, pay, 2, TX.LAYOUT_REFERENCE, is_u8=True, freq_norm=TX.SERIES_SHIFT if shifted else 0.0, prs=prs)
    for k in range(2):
        assert (got[k][:2 * g.nb_null_period] == 127).all(), f"frame {k}: NULL period"
        assert not got[k][2 * g.nb_null_period:].any(), f"frame {k}: {int((got[k][2 * g.nb_null_period:] != 0).sum())} samples are not 0"


@pytest.mark.parametrize("f", TX.shift_cases(), ids=lambda f: f"{float(f):+.6e}")
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_frequency_shift_edges(oracle, ctx, mode, f):
    """equality with oracle.apply_pll (held to a float64 rotation by tests/test_independent_pins.py) in both output formats; every frame's
    phase starts at 0: two frames of one payload are equal"""
    rng = np.random.default_rng(5600 + mode)
    one = rng.integers(0, 256, TX.payload_bytes(oracle, mode), dtype=np.uint8)
    pay = np.stack([one, one])
    frame = expected_frame(oracle, mode, one, TX.LAYOUT_REFERENCE)
    for is_u8 in (False, True):
        got = as_output(device_modulate(ctx, oracle, mode, pay, 2, TX.LAYOUT_REFERENCE, is_u8=is_u8, freq_norm=f), is_u8)
        exp = expected_output(oracle, mode, frame, is_u8, f)
        assert np.array_equal(got[0], exp), f"u8 {is_u8}: {int((got[0] != exp).sum())} words differ"
        assert np.array_equal(got[1], got[0]), f"u8 {is_u8}: frame 1 does not start at phase 0"
        if not is_u8:
            assert not np.array_equal(exp, u32(frame))                   # (the expectation is a shifted frame)


@pytest.mark.parametrize("is_u8", [False, True])
def test_zero_frames_is_ok_and_writes_nothing(oracle, ctx, is_u8):
    for mode in (1, 2):
        got = device_modulate(ctx, oracle, mode, np.zeros(0, np.uint8), 0, TX.LAYOUT_REFERENCE, is_u8=is_u8)      # (checks both guards)
        assert got.shape[0] == 0


@pytest.mark.parametrize("mode", [1, 3])
def test_host_sync_form_with_several_frames(oracle, ctx, mode):
    """Context.ofdm_modulate_frames_host: 5 frames, u8 with a shift and a caller's PRS; then 3 frames on the same context (the scratch
    slots of the first call reused): the first call's leading frames"""
    if DEAD:
        pytest.fail(f"not run: {DEAD[0]}")
    _, u8 = formats()
    g = oracle.geometry(mode)
    prs = oracle.prs_fft_mode(mode).copy()
    bins = TX.carrier_bins(g.nb_fft, g.nb_carriers)
    prs[bins[5]] = np.complex64(prs[bins[5]] * np.complex64(0.25 + 0.5j))
    prs[bins[-3]] = np.complex64(prs[bins[-3]] * np.complex64(-1.5))
    f = TX.freq_norm(-2500.0)
    rng = np.random.default_rng(5700 + mode)
    pay = rng.integers(0, 256, (5, TX.payload_bytes(oracle, mode)), dtype=np.uint8)
    for layout in (TX.LAYOUT_REFERENCE, TX.LAYOUT_FRAME_BITS):
        got = ctx.ofdm_modulate_frames_host(mode, pay, 5, layout=layout, out_format=u8, prs_fft_ref=prs, freq_norm=f)
        for k in range(5):
            exp = expected_output(oracle, mode, expected_frame(oracle, mode, pay[k], layout, prs=prs), True, f)
            assert np.array_equal(got[k], exp), f"layout {layout} frame {k}"
        assert not np.array_equal(got[0], expected_output(oracle, mode, expected_frame(oracle, mode, pay[0], layout), True, f))
        again = ctx.ofdm_modulate_frames_host(mode, pay[:3], 3, layout=layout, out_format=u8, prs_fft_ref=prs, freq_norm=f)
        assert np.array_equal(again, got[:3]), f"layout {layout}"


# ---- all sixteen instantiations at forced run lengths: one fresh process per (mode, symbols per run) --------------------------------
def run_lengths(n_sym):
    """one symbol per run; 2 and 3; 7 (divides neither 76 nor 153: a short last run); n_sym - 1 (a last run of one symbol that replays the
    whole chain); the whole frame in one run; more than the frame holds"""
    return [1, 2, 3, 7, n_sym - 1, n_sym, n_sym + 5]


SERIES = [(mode, spb) for mode in (1, 2, 3, 4) for spb in run_lengths(CH.MODE_SYMBOLS[mode])]
SEED_BASE = 5000
SERIES_EXPECTED = {}
CHILDREN = {}                                  # symbols per run -> (output directory, exit status, end of stderr) of its child


def series_expected(oracle, mode):
    """name of the combination -> [N_FRAMES] expected outputs (the same payloads for every run length of a mode)"""
    if mode not in SERIES_EXPECTED:
        pay = CH.payloads(CH.seed_of(SEED_BASE, mode), TX.payload_bytes(oracle, mode))
        frames = {layout: [expected_frame(oracle, mode, pay[k], layout) for k in range(CH.N_FRAMES)] for layout in (0, 1)}
        SERIES_EXPECTED[mode] = {name: [expected_output(oracle, mode, fr, is_u8, TX.SERIES_SHIFT if pll else 0.0) for fr in frames[layout]]
                                 for name, is_u8, layout, pll in CH.combinations()}
    return SERIES_EXPECTED[mode]


def child_of(spb, tmp_path_factory):
    """the child of one run length, started when the first case asks for it: it serves every mode whose series holds that run length
    (ten processes for the 28 cases; one at a time, each under its own limit, none started after one was lost)"""
    if spb not in CHILDREN:
        if DEAD:
            pytest.fail(f"not run: {DEAD[0]}")
        modes = [m for m in (1, 2, 3, 4) if spb in run_lengths(CH.MODE_SYMBOLS[m])]
        out_dir = str(tmp_path_factory.mktemp(f"tx_spb{spb}"))
        env = dict(os.environ)
        env["DABGPU_TX_SPB"] = str(spb)
        cmd = [sys.executable, os.path.join(HERE, "tx_variants_child.py"), str(spb), str(SEED_BASE), out_dir, ",".join(str(m) for m in modes)]
        try:
            res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
            CHILDREN[spb] = (out_dir, res.returncode, res.stderr[-2000:])
            if res.returncode < 0 or res.returncode in (124, 134, 137, 139):
                DEAD.append(f"the child of {spb} symbols per run ended with status {res.returncode}: {res.stderr[-500:]}")
        except subprocess.TimeoutExpired:
            CHILDREN[spb] = (out_dir, None, "")
            DEAD.append(f"the child of {spb} symbols per run was ended after {CHILD_TIMEOUT_S} s")
    return CHILDREN[spb]


@pytest.mark.parametrize("mode,spb", SERIES)
def test_every_variant_at_a_forced_run_length(oracle, tmp_path_factory, mode, spb):
    g = oracle.geometry(mode)
    assert g.nb_frame_symbols == CH.MODE_SYMBOLS[mode]
    if spb not in CHILDREN and DEAD:
        pytest.fail(f"not run: {DEAD[0]}")
    out_dir, status, stderr = child_of(spb, tmp_path_factory)
    assert status == 0, f"the child of {spb} symbols per run: status {status}: {stderr}"
    expected = series_expected(oracle, mode)
    bad = []
    for name, is_u8, layout, pll in CH.combinations():
        buf = np.load(os.path.join(out_dir, CH.file_name(mode, name)))
        bpf = g.nb_frame_samples * (2 if is_u8 else 8)
        assert buf.size == 2 * GUARD + CH.N_FRAMES * bpf
        check_guards(buf[:GUARD], buf[GUARD + CH.N_FRAMES * bpf:], f"mode {mode} spb {spb} {name}")
        got = as_output(buf[GUARD:GUARD + CH.N_FRAMES * bpf].reshape(CH.N_FRAMES, bpf), is_u8)
        for k in range(CH.N_FRAMES):
            diff = got[k] != expected[name][k]
            if diff.any():
                first = int(np.argmax(diff)) // 2
                sym = (first - g.nb_null_period) // g.nb_symbol_period if first >= g.nb_null_period else -1
                bad.append(f"{name} frame {k}: {int(diff.sum())} words differ, the first in sample {first} (symbol {sym})")
    assert not bad, f"mode {mode}, {spb} symbols per run: " + "; ".join(bad)
