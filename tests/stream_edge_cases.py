"""Test infrastructure shared by tests/test_stream_model_edges.py (CPU) and tests/test_gpu_stream_bank_edges.py (-m gpu): the table of
L1 window settings, the captures, the block schedules that end blocks exactly on state boundaries, and the quantisers.  Everything is
built once per session and handed out read-only."""
import numpy as np

import modes_model as MM
import stream_model as SM

# (k, decimate, beta, thresh_null_start, thresh_null_end): dabgpu_stream_cfg's signal_l1_nb_samples, signal_l1_nb_decimate,
# signal_l1_update_beta, thresh_null_start, thresh_null_end.  stream_l1_kernel reduces windows of up to 128 samples in LDS (row pitch
# k + 1) and longer ones directly
L1_TABLE = [
    (100, 5, 0.95, 0.35, 0.75),      # the defaults
    (128, 5, 0.95, 0.35, 0.75),      # the largest k on the LDS path
    (129, 3, 0.95, 0.35, 0.75),      # the first k on the direct path
    (300, 2, 0.95, 0.35, 0.75),      # direct path, k above the 256 threads of a workgroup
    (64, 1, 0.95, 0.35, 0.75),       # adjacent windows
    (1, 7, 0.95, 0.35, 0.75),        # one-sample windows: several failed synchronisations before the lock
    (100, 5, 0.5, 0.2, 0.9),         # another beta and other thresholds
]
IMPULSE_DB = 8.0                     # the reference's default 20 dB rarely passes with the short symbols of mode III
TINY = (1, 7, 99, 100, 101)          # k - 1, k and k + 1 of the default k among them
# lead-in of the mode III edge capture: 36077 samples = 72 level windows, so that the level the first NULL is compared with has settled
# (97.5 %) whether the capture comes in blocks or as one
EDGE_PAD_MODE3 = 30077
_cache = {}


def l1_settings(row):
    k, decimate, beta, start, end = row
    return SM.L1Settings(beta=beta, k=k, decimate=decimate, start=start, end=end)


def model(oracle, mode, row=None):
    m = SM.StreamModel(oracle, mode, None if row is None else l1_settings(row))
    if mode != 1:
        m.cfg.impulse_peak_threshold_db = IMPULSE_DB
    return m


def _frozen(a):
    a.setflags(write=False)
    return a


def mode1_capture(oracle, seed=1, cfo=1.8e-3, pad=1234, noise=3.0):
    """make_stream(oracle, seed, 4, cfo, pad, noise) of tests/test_gpu_stream_bank.py"""
    key = ("m1", seed, cfo, pad, noise)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        frames = [oracle.modulate_frame(rng.integers(0, 2, oracle.NB_FRAME_BITS, dtype=np.uint8)) for _ in range(4)]
        tx = oracle.apply_pll(np.concatenate(frames), cfo, 0.11)
        s = np.concatenate([tx[oracle.NB_NULL_PERIOD:oracle.NB_NULL_PERIOD + 20000 + pad], tx])
        s = s + noise * (rng.standard_normal(s.size) + 1j * rng.standard_normal(s.size))
        _cache[key] = _frozen((s * (1.0 / 39.2)).astype(np.complex64))
    return _cache[key]


def mode3_capture(oracle, seed=1, n_frames=8, cfo_bins=2.1, pad=77, noise=0.05):
    """make(seed, n_frames, cfo_bins, pad, noise) of test_stream_bank_in_other_transmission_modes for mode III (generator seed 3000 + seed)"""
    key = ("m3", seed, n_frames, cfo_bins, pad, noise)
    if key not in _cache:
        g = oracle.geometry(3)
        rng = np.random.default_rng(3000 + seed)
        sent = [rng.integers(0, 2, g.nb_frame_bits, dtype=np.uint8) for _ in range(n_frames)]
        tx = oracle.apply_pll(np.concatenate([MM.make_tx_frame(oracle, 3, b, rng) for b in sent]), cfo_bins / g.nb_fft, 0.2)
        s = np.concatenate([tx[g.nb_null_period:g.nb_null_period + 6000 + pad], tx])
        s = (s + noise * (rng.standard_normal(s.size) + 1j * rng.standard_normal(s.size))) / 39.2
        _cache[key] = _frozen(s.astype(np.complex64))
    return _cache[key]


def noise_with_dips(seed, n, carrier=0.0, first=40000, every=53000, length=2600):
    """no DAB signal: false NULLs, failed synchronisations (tests/test_gpu_stream_bank.py).  White noise alone passes the 8 dB impulse-peak
    test of the mode III banks about every second time and then yields frames; with an unmodulated carrier of amplitude `carrier` (20.3
    bins of the mode III FFT above the centre) beside the noise the impulse response is flat and every synchronisation fails"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.1
    if carrier:
        x = x + carrier * np.exp(2j * np.pi * (20.3 / 256.0) * np.arange(n))
    for a in range(first, n - 4000, every):
        x[a:a + length] *= 0.05
    return x.astype(np.complex64)


def l1_streams(oracle, mode):
    """the three streams of an L1 bank: two captures with different offsets and noise, one noise-only capture with dips; equal lengths,
    ragged against the block length"""
    key = ("l1", mode)
    if key not in _cache:
        if mode == 3:
            a, b = mode3_capture(oracle), mode3_capture(oracle, 2, 8, -3.4, 311, 0.1)
        else:
            a, b = mode1_capture(oracle), mode1_capture(oracle, 2, -7.3e-3, 77, 6.0)
        n = min(a.size, b.size)
        n -= n % 5
        _cache[key] = [_frozen(np.array(a[:n])), _frozen(np.array(b[:n])), _frozen(noise_with_dips(4, n, carrier=1.0 if mode == 3 else 0.0))]
    return _cache[key]


def l1_blocks(row, n):
    """no level update (k - 1; left out for k = 1, a call without samples does nothing), zero windows (k), one window of the level
    update (k + 1, k * decimate, k * decimate + 1: the windows start at i = 0, k * decimate, ... < n - k), two (k * decimate + k + 1),
    then 20002 repeatedly and what is left"""
    k, decimate = row[0], row[1]
    blocks = [b for b in (k - 1, k, k + 1, k * decimate, k * decimate + 1, k * decimate + k + 1) if b > 0]
    left = n - sum(blocks)
    blocks += [20002] * (left // 20002)
    if left % 20002:
        blocks.append(left % 20002)
    assert sum(blocks) == n
    return blocks


def quantise(s, name, full=None):
    """[n] complex float -> [n][2] capture components of format `name`; the integer formats scaled so that `full` (default: the largest
    sample) is the full range"""
    x = np.stack([s.real, s.imag], axis=-1)
    if name == "raw_f32l":
        return x.astype(np.float32)
    full = np.abs(s).max() if full is None else full
    if name == "raw_u8":
        return np.clip(np.rint(x / full * 127.0 + 127.5), 0, 255).astype(np.uint8)
    assert name == "raw_s16l"
    return np.clip(np.rint(x / full * 30000.0), -32768, 32767).astype("<i2")


def dequantise(oracle, q, name):
    """what the bank's loaders make of the capture components q [n][2]: the oracle's reader arithmetic, [n] complex float"""
    if name == "raw_f32l":
        return np.ascontiguousarray(q).view(np.complex64).reshape(-1)
    fmt = oracle.IQ_MODES.index(name)
    return oracle.iq_convert(np.ascontiguousarray(q).view(np.uint8).reshape(-1), fmt).view(np.complex64)


def l1_quantised(oracle, mode, name):
    """(components [3][n][2], what the loaders make of them [3][n]) of l1_streams in capture format `name`"""
    key = ("l1q", mode, name)
    if key not in _cache:
        q = np.stack([quantise(s, name) for s in l1_streams(oracle, mode)])
        _cache[key] = (_frozen(q), [_frozen(dequantise(oracle, x, name)) for x in q])
    return _cache[key]


def ring_blocks(blocks, limit):
    """the same block ends with every block cut into pieces of at most `limit` samples (the ring form takes no more per call)"""
    out = []
    for b in blocks:
        while b > limit:
            out.append(limit)
            b -= limit
        out.append(b)
    return out


def edge_case(oracle, mode, name="raw_f32l", k=100):
    """The exact-block-end case of transmission mode I or III in capture format `name`: five streams, stream e = stream 0's capture
    delayed by 0, 1, 2, 3 and k samples of noise (cut to stream 0's length) -- every exact block end of stream 0 is one, two and three
    samples late for its neighbours, the last is in an unrelated phase.  The schedule is built on what the loaders make of stream 0
    (quantisation can move a fine time offset, and with it every later event).
    dict(q = components [5][n][2], iq = the loaders' view [5][n], blocks, after = stream 0's snapshots, hits = stream 0's)"""
    key = ("edge", mode, name)
    if key not in _cache:
        capture = mode1_capture(oracle) if mode == 1 else mode3_capture(oracle, pad=EDGE_PAD_MODE3)
        full = np.abs(capture).max()
        lead = noise_with_dips(77, k) * (np.sqrt(np.mean(np.abs(capture) ** 2)) / 0.1414)
        q0, ql = quantise(capture, name, full), quantise(lead, name, full)
        q = np.stack([np.concatenate([ql[:d], q0])[:capture.size] for d in (0, 1, 2, 3, k)])
        iq = [_frozen(dequantise(oracle, x, name)) for x in q]
        blocks, after = SM.edge_schedule(lambda: model(oracle, mode), iq[0], 4, TINY, block=50000 if mode == 1 else 20002)
        _cache[key] = dict(q=_frozen(q), iq=iq, blocks=blocks, after=after, hits=SM.edge_hits(oracle.geometry(mode), blocks, after, k))
    return _cache[key]


def one_block(oracle, mode, name="raw_f32l"):
    """the model after stream 0 of edge_case fed as one block"""
    key = ("one", mode, name)
    if key not in _cache:
        m = model(oracle, mode)
        m.process(edge_case(oracle, mode, name)["iq"][0])
        _cache[key] = m
    return _cache[key]


def run_model(m, capture, blocks):
    """m fed `capture` in `blocks`; the snapshots after every block"""
    after, pos = [], 0
    for b in blocks:
        m.process(capture[pos:pos + b])
        pos += b
        after.append(m.snapshot())
    return after
