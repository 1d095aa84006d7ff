"""-m gpu: the channeliser on the device (dabgpu_channeliser_bank_*, dab-radio_amd/csrc/channelise.hip) against the host model -- the same
channelise_core.h under g++ (tests/cpp/channelise_host_model.cpp) -- bit for bit; the host model is tied to the independent numpy model and
to the closed form by tests/test_channelise_model.py.  Small shapes: one output, one tile and its neighbours, two tiles and three."""
import numpy as np
import pytest

import channelise_model as CM
import signal_bank_cases as SB

pytestmark = pytest.mark.gpu

N_IN = 6007                                  # no tile divides it; shorter than what 1027 outputs read at D = 8 (zero-fill; wrap passes the end in a later tile)
N_BLK = 1501                                 # block rows of the combiner
GUARD = 0xA5
DS = [1, 2, 3, 4, 5, 8]
TILE = CM.SPLIT_TILE
N_OUTS = [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3]
START = -37                                  # the peak of output 0 sits 37 samples before the input


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return CM.build_host_model(tmp_path_factory.mktemp("channelise_host_model"))


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def x3():
    rng = np.random.default_rng(7400)
    return (rng.standard_normal((3, N_IN)) + 1j * rng.standard_normal((3, N_IN))).astype(np.complex64)


@pytest.fixture(scope="module")
def blocks12():
    rng = np.random.default_rng(7500)
    return (rng.standard_normal((12, N_BLK)) + 1j * rng.standard_normal((12, N_BLK))).astype(np.complex64)


def channels12(D):
    """streams 0, 1, 2 with 1, 3 and 8 channels: Band III offsets at the rate 2.048 D MS/s (folded into +- half the rate), the skipped
    rotation (0, 0), a phase alone, +- half the rate, gains of both signs"""
    rate = 2048000.0 * D
    fold = lambda hz: (hz + rate / 2) % rate - rate / 2
    f = lambda hz: CM.freq_q64(fold(hz), rate)
    chs = [CM.channel(f(300000.0), 0x0123456789ABCDEF, 1.0, 0)]
    chs += [CM.channel(f(-1412000.0), 1 << 63, -0.5, 1), CM.channel(0, 0, 1.0, 1), CM.channel(f(2012000.0), 0, 2.0, 1)]
    chs += [CM.channel(f(300000.0 + k * 1712000.0), (k * 0x1111111111111111) & CM.M64, 1.0 + 0.25 * k, 2) for k in range(-3, 3)]
    chs += [CM.channel(0, 12345 << 40, 1.0, 2), CM.channel(1 << 63, 0, -1.0, 2)]
    return chs


def bank(ctx, host, chs, n_streams, D, start=0):
    """(device bank, the host model's design record): both from the same dabgpu_channeliser_design source, compared here"""
    import dabgpu
    F = CM.host_design(host, D)
    G = dabgpu.channeliser_design(D)
    assert np.array_equal(np.ctypeslib.as_array(G.table), np.ctypeslib.as_array(F.table)) and G.error == F.error
    return dabgpu.Channeliser(ctx, [CM.to_struct(c, dabgpu.ChanneliserChannel) for c in chs], n_streams, G, start), F


def run_device(cb, split, x, n_out, wrap, fmt=CM.F32, scale=1.0, shared=False, rows=None):
    """one call into guarded rows -> ([rows][n_out] complex64 or [rows][n_out][2] u8, guards intact)"""
    import torch
    rows = (cb.n_channels if split else cb.n_streams) if rows is None else rows
    sb = 8 if fmt == CM.F32 else 2
    stride = ((n_out * sb + 15) & ~15) + 32                                  # guard bytes between the rows
    whole = torch.full((48 + rows * stride + 48,), GUARD, dtype=torch.uint8, device="cuda")
    view = whole[48:48 + rows * stride]
    n_in = x.shape[-1]
    pad = np.zeros(x.shape[:-1] + (n_in + (n_in & 1),), np.complex64)        # rows an even count apart
    pad[..., :n_in] = x
    d_in = torch.from_numpy(pad).cuda()
    in_stride = 0 if shared else pad.shape[-1]
    if split:
        cb.split(d_in, n_in, n_out, view, in_stride_samples=in_stride, wrap=wrap, out_stride_bytes=stride)
    else:
        cb.combine(d_in, n_in, n_out, view, in_stride_samples=in_stride, wrap=wrap, out_format=fmt, out_stride_bytes=stride, u8_scale=scale)
    torch.cuda.synchronize()
    h = whole.cpu().numpy()
    out = h[48:48 + rows * stride].reshape(rows, stride)
    ok = bool(np.all(h[:48] == GUARD) and np.all(h[-48:] == GUARD) and np.all(out[:, n_out * sb:] == GUARD))
    data = np.ascontiguousarray(out[:, :n_out * sb])
    return (data.view(np.complex64) if fmt == CM.F32 else data.reshape(rows, n_out, 2)), ok


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


_ref = {}


def split_reference(host, x3, D, wrap):
    """the host model over the longest call from position 0, once per (D, wrap): shorter calls are its prefixes"""
    key = ("split", D, wrap)
    if key not in _ref:
        _ref[key] = CM.host_split(host, channels12(D), CM.host_design(host, D), x3, 0, START, N_OUTS[-1], wrap)
    return _ref[key]


def combine_reference(host, blocks12, D, wrap, fmt):
    key = ("combine", D, wrap, fmt)
    if key not in _ref:
        _ref[key] = CM.host_combine(host, channels12(D), 3, CM.host_design(host, D), blocks12, 0, START, N_OUTS[-1], wrap, fmt, 25.0)
    return _ref[key]


@pytest.mark.parametrize("n_out", N_OUTS)
@pytest.mark.parametrize("D", DS)
def test_split_equals_the_host_model(host, ctx, x3, D, n_out):
    cb, F = bank(ctx, host, channels12(D), 3, D, START)
    assert cb.plan["split_tile"] == TILE and cb.plan["split_lds_bytes"] == (0 if D == 1 else 2 * 4 * D * 147 * 8)
    for wrap in (False, True):
        cb.seek(0)
        got, ok = run_device(cb, True, x3, n_out, wrap)
        assert ok, "guard bytes before, between or after the rows were written"
        exp = split_reference(host, x3, D, wrap)[:, :n_out]
        for c in range(12):
            assert same_bits(got[c], exp[c]), f"channel {c}, wrap {wrap}"
    cb.close()


@pytest.mark.parametrize("fmt", [CM.F32, CM.U8])
@pytest.mark.parametrize("D", DS)
def test_combine_equals_the_host_model(host, ctx, blocks12, D, fmt):
    cb, F = bank(ctx, host, channels12(D), 3, D, START)
    assert cb.plan["combine_tile"] == 128 * D
    for wrap in (False, True):
        for n_out in N_OUTS:
            cb.seek(0)
            got, ok = run_device(cb, False, blocks12, n_out, wrap, fmt, 25.0)
            assert ok, "guard bytes before, between or after the rows were written"
            exp = combine_reference(host, blocks12, D, wrap, fmt)[:, :n_out]
            for s in range(3):
                assert same_bits(got[s], exp[s]), f"stream {s}, wrap {wrap}, n_out {n_out}"
    cb.close()


@pytest.mark.parametrize("D", [1, 4, 8])
def test_shared_input_far_positions_and_a_call_split_in_two(host, ctx, x3, blocks12, D):
    """one shared wideband row for three streams; a seek to just under the position limit with the `start` that brings the window back
    into the input; a + b at an odd point equal to one call, both directions"""
    chs = channels12(D)
    pos = CM.MAX_POSITION - 700
    start = 100 - pos * D
    assert -CM.MAX_START <= start
    cb, F = bank(ctx, host, chs, 3, D, start)
    for wrap in (False, True):
        cb.seek(pos)
        got, ok = run_device(cb, True, x3[1], 600, wrap, shared=True)
        exp = CM.host_split(host, chs, F, x3[1], pos, start, 600, wrap)
        assert ok and same_bits(got, exp) and np.abs(exp[0]).min() > 0, wrap
        assert not same_bits(got[0], CM.host_split(host, chs[:1], F, x3[1], pos - 1, start, 600, wrap)[0])
    cb.seek(pos + 13)                                                         # a then b: 333 + 267 outputs from an odd position
    a, ok_a = run_device(cb, True, x3[1], 333, True, shared=True)
    b, ok_b = run_device(cb, True, x3[1], 267, True, shared=True)
    exp = CM.host_split(host, chs, F, x3[1], pos + 13, start, 600, True)
    assert ok_a and ok_b and same_bits(a, exp[:, :333]) and same_bits(b, exp[:, 333:])
    cb.close()
    # the combiner at the far position: wideband sample n = pos + i takes block samples around (n - start) / D
    startc = pos - 50 * D - 3
    cb, F = bank(ctx, host, chs, 3, D, startc)
    for wrap in (False, True):
        cb.seek(pos)
        a, ok_a = run_device(cb, False, blocks12, 333, wrap)
        b, ok_b = run_device(cb, False, blocks12, 600 * D - 333, wrap)
        exp = CM.host_combine(host, chs, 3, F, blocks12, pos, startc, 600 * D, wrap)
        assert ok_a and ok_b and same_bits(a, exp[:, :333]) and same_bits(b, exp[:, 333:]) and np.abs(exp[2, 300:]).min() > 0, wrap
    cb.close()


@pytest.mark.parametrize("D", [1, 4])
def test_graph_replays_continue_the_stream_and_set_params_retunes_between_them(host, ctx, x3, D):
    import dabgpu
    import torch
    chs = channels12(D)[:4]
    cb, F = bank(ctx, host, chs, 2, D, START)
    n = 517
    pad = np.zeros((2, N_IN + 1), np.complex64)
    pad[:, :-1] = x3[:2]
    d_in = torch.from_numpy(pad).cuda()
    stride = (n * 8 + 15) & ~15
    out = torch.zeros(4 * stride, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        cb.split(d_in, N_IN, n, out, in_stride_samples=N_IN + 1, wrap=True, out_stride_bytes=stride, stream=side.cuda_stream)
    lists = [chs, chs[:2] + [CM.channel(CM.freq_q64(77000.0, 2048000.0 * D), 5, 0.75, 1)] + chs[3:], chs]       # channel 2 retuned, then back
    for r in range(3):                                                       # (capturing enqueued nothing: the position is still 0)
        cb.set_params([CM.to_struct(c, dabgpu.ChanneliserChannel) for c in lists[r]], START)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(4, stride)[:, :n * 8].copy().view(np.complex64)
        exp = CM.host_split(host, lists[r], F, x3[:2], r * n, START, n, True)
        assert same_bits(got, exp), f"replay {r}"
    assert not same_bits(exp[2], CM.host_split(host, lists[1], F, x3[:2], 2 * n, START, n, True)[2])
    cb.close()


def test_identity_mixer_returns_its_input_and_nan_reaches_only_its_taps(host, ctx, x3):
    ident = [CM.channel(0, 0, 1.0, 0), CM.channel(0, 0, 1.0, 1), CM.channel(0, 0, 1.0, 2)]
    cb, F = bank(ctx, host, ident, 3, 1, -1)
    got, ok = run_device(cb, True, x3, N_IN, False)                           # D = 1, no oscillator, gain 1: the input, one sample late
    assert ok and same_bits(got[0, 1:], x3[0, :-1]) and got[0, 0] == 0 and same_bits(got[2, 1:], x3[2, :-1])
    cb.close()
    x = x3.copy()
    x[:, 1500] = np.nan
    x[:, 2000] = complex(np.inf, -0.0)
    D = 4
    chs = channels12(D)
    cb, F = bank(ctx, host, chs, 3, D, 0)
    got, ok = run_device(cb, True, x, 1200, False)
    exp = CM.host_split(host, chs, F, x, 0, 0, 1200, False)
    bad = ~np.isfinite(exp)
    assert ok and np.array_equal(~np.isfinite(got), bad)
    assert 2 * 72 - 4 <= bad[0].sum() <= 2 * 72 + 2                          # two bad samples, 288 taps = 72 outputs each
    assert same_bits(got[~bad], exp[~bad])
    cb.close()


def test_host_forms_and_refusals(host, ctx, x3, blocks12):
    import dabgpu
    import torch
    D = 4
    chs = channels12(D)
    cb, F = bank(ctx, host, chs, 3, D, START)
    assert same_bits(cb.split_host(x3, 700, in_stride_samples=N_IN, wrap=True), CM.host_split(host, chs, F, x3, 0, START, 700, True))
    got = cb.combine_host(blocks12, 77, in_stride_samples=N_BLK, out_format=CM.U8, u8_scale=25.0)
    assert got.shape == (3, 77, 2) and same_bits(got, CM.host_combine(host, chs, 3, F, blocks12, 700, START, 77, False, CM.U8, 25.0))
    # a list that exceeds the plan is refused, a shorter one runs and leaves the other rows alone
    with pytest.raises(dabgpu.DabGpuError) as err:
        cb.set_params([CM.to_struct(c, dabgpu.ChanneliserChannel) for c in chs + [CM.channel(stream=2)]], START)
    assert "13 channels, the bank was created with 12" in str(err.value)
    for bad, text in (([CM.channel(stream=1), CM.channel(stream=0)], "sorted by stream"), ([CM.channel(stream=3)], "stream 3 of 3"),
                      ([CM.channel(gain=float("inf"))], "gain is not finite"), ([CM.channel(stream=2)] * 9, "more than 8 channels")):
        with pytest.raises(dabgpu.DabGpuError) as err:
            cb.set_params([CM.to_struct(c, dabgpu.ChanneliserChannel) for c in bad], START)
        assert text in str(err.value), str(err.value)
    with pytest.raises(dabgpu.DabGpuError) as err:
        cb.seek((1 << 58) + 1)
    assert "2^58" in str(err.value)
    pad = np.zeros((3, N_IN + 1), np.complex64)
    pad[:, :-1] = x3
    d_in = torch.from_numpy(pad).cuda()
    d_out = torch.full((12 * 1040 * 8,), GUARD, dtype=torch.uint8, device="cuda")
    for change, text in ((dict(n_in=0), "n_in = 0"), (dict(in_stride_samples=N_IN), "in_stride_samples"), (dict(out_stride_bytes=1029 * 8 - 8), "out_stride_bytes"),
                         (dict(d_out=d_out[8:]), "16-byte aligned"), (dict(d_in=None), "null input")):
        a = dict(d_in=d_in, n_in=N_IN, n_out=1029, d_out=d_out, in_stride_samples=N_IN + 1, wrap=True, out_stride_bytes=1040 * 8)
        a.update(change)
        with pytest.raises(dabgpu.DabGpuError) as err:
            cb.split(**a)
        assert text in str(err.value) and "channeliser_bank_split" in str(err.value), (change, str(err.value))
    with pytest.raises(dabgpu.DabGpuError) as err:
        cb.combine(d_in, N_IN, 16, d_out, in_stride_samples=N_IN + 1, out_format=CM.U8, u8_scale=float("nan"))
    assert "u8_scale" in str(err.value)
    torch.cuda.synchronize()
    assert bool((d_out == GUARD).all())
    fewer = chs[:4]
    cb.set_params([CM.to_struct(c, dabgpu.ChanneliserChannel) for c in fewer], 5)
    got, ok = run_device(cb, True, x3, 100, True, rows=12)                   # the stream goes on from where the host forms left it
    assert ok and same_bits(got[:4], CM.host_split(host, fewer, F, x3, 777, 5, 100, True)) and np.all(got[4:].view(np.uint8) == GUARD)
    cb.close()


@pytest.mark.parametrize("split", [True, False])
def test_host_form_three_calls_regrow_the_buffers_of_one_bank(host, ctx, x3, blocks12, split):
    """7 samples out of 64 in, 2049 out of the whole input (both buffers grow), 101 (both larger than needed); then the device form goes on
    from the summed position.  Two wideband streams, the three channels all on stream 1: stream 0 has none and its combined row is zeros.
    (The combine kernel stores those zeros itself and the split kernel writes every channel's row, so the host forms' zeroing of the
    output buffer cannot be told from its absence here.)"""
    import dabgpu
    D = 4
    chs = channels12(D)[1:4]
    cb, F = bank(ctx, host, chs, 2, D, START)
    x = np.ascontiguousarray(x3[:2, :4001]) if split else np.ascontiguousarray(blocks12[:3])
    rows = 3 if split else 2
    L = dabgpu.lib()

    def host_sync(x, n_out, wrap, fmt, out, stride):
        n_in = x.shape[-1]
        if split:
            dabgpu.check(L.dabgpu_channeliser_bank_split_host_sync(cb._h, x.ctypes.data, n_in, n_in, int(wrap), n_out, out.ctypes.data, stride), "host form")
        else:
            dabgpu.check(L.dabgpu_channeliser_bank_combine_host_sync(cb._h, x.ctypes.data, n_in, n_in, int(wrap), n_out, out.ctypes.data, fmt, stride, 25.0),
                         "host form")

    def model(x, pos, n_out, wrap, fmt=CM.F32):
        if split:
            return CM.host_split(host, chs, F, x, pos, START, n_out, wrap)
        return CM.host_combine(host, chs, 2, F, x, pos, START, n_out, wrap, fmt, 25.0)

    pos = SB.host_form_regrowth(host_sync, model, x, rows, CM.F32, None if split else CM.U8)  # (split has no u8 form)
    assert pos == SB.HOST_TOTAL
    got, ok = run_device(cb, split, x, 300, True)
    assert ok and same_bits(got, model(x, pos, 300, True))
    if not split:
        assert not got[0].any() and got[1].any()
    cb.close()


@pytest.mark.parametrize("D, n_in", [(8, 1001), (4, 700), (1, 300)])
def test_wrap_with_an_input_shorter_than_one_tiles_window(host, ctx, x3, D, n_in):
    """a tile's window (584 D samples; 512 at D = 1) longer than the input: the loads reduce every index modulo n_in, more than once"""
    chs = channels12(D)
    x = np.ascontiguousarray(x3[:, :n_in])
    cb, F = bank(ctx, host, chs, 3, D, START)
    got, ok = run_device(cb, True, x, TILE + 5, True)
    assert ok and same_bits(got, CM.host_split(host, chs, F, x, 0, START, TILE + 5, True))
    cb.close()
    cb, F = bank(ctx, host, chs, 3, D, START)
    xb = np.ascontiguousarray(x3[:, :61].repeat(4, axis=0))                   # 12 block rows shorter than the combiner's window of 199
    got, ok = run_device(cb, False, xb, 128 * D + 9, True)
    assert ok and same_bits(got, CM.host_combine(host, chs, 3, F, xb, 0, START, 128 * D + 9, True))
    cb.close()


@pytest.mark.parametrize("D", [1, 4])
def test_combine_graph_replays_continue_the_stream_and_set_params_retunes_between_them(host, ctx, blocks12, D):
    import dabgpu
    import torch
    chs = channels12(D)[:4]
    cb, F = bank(ctx, host, chs, 2, D, START)
    n = 517
    pad = np.zeros((4, N_BLK + 1), np.complex64)
    pad[:, :-1] = blocks12[:4]
    d_in = torch.from_numpy(pad).cuda()
    stride = (n * 8 + 15) & ~15
    out = torch.zeros(2 * stride, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        cb.combine(d_in, N_BLK, n, out, in_stride_samples=N_BLK + 1, wrap=True, out_stride_bytes=stride, stream=side.cuda_stream)
    lists = [chs, chs[:2] + [CM.channel(CM.freq_q64(77000.0, 2048000.0 * D), 5, 0.75, 1)] + chs[3:], chs]       # channel 2 retuned, then back
    for r in range(3):                                                       # (capturing enqueued nothing: the position is still 0)
        cb.set_params([CM.to_struct(c, dabgpu.ChanneliserChannel) for c in lists[r]], START)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(2, stride)[:, :n * 8].copy().view(np.complex64)
        exp = CM.host_combine(host, lists[r], 2, F, blocks12[:4], r * n, START, n, True)
        assert same_bits(got, exp), f"replay {r}"
    assert not same_bits(exp[1], CM.host_combine(host, lists[1], 2, F, blocks12[:4], 2 * n, START, n, True)[1])
    cb.close()


def test_combine_identity_nan_and_refusals(host, ctx, blocks12):
    import dabgpu
    # D = 1, no oscillator, gain 1, one channel per stream: the block rows, one sample late, bit for bit
    ident = [CM.channel(0, 0, 1.0, 0), CM.channel(0, 0, 1.0, 1), CM.channel(0, 0, 1.0, 2)]
    cb, F = bank(ctx, host, ident, 3, 1, 1)
    got, ok = run_device(cb, False, blocks12[:3], N_BLK, False)
    assert ok and same_bits(got[0, 1:], blocks12[0, :-1]) and got[0, 0] == 0 and same_bits(got[2, 1:], blocks12[2, :-1])
    cb.close()
    # NaN and infinity reach only the wideband samples whose 72 taps cover them: 72 D each
    D = 4
    chs = channels12(D)
    x = blocks12.copy()
    x[:, 400] = np.nan
    x[:, 700] = complex(-np.inf, 0.0)
    cb, F = bank(ctx, host, chs, 3, D, 0)
    got, ok = run_device(cb, False, x, 4000, False)
    exp = CM.host_combine(host, chs, 3, F, x, 0, 0, 4000, False)
    bad = ~np.isfinite(exp)
    assert ok and np.array_equal(~np.isfinite(got), bad) and bad[0].sum() == 2 * 72 * D
    assert same_bits(got[~bad], exp[~bad])
    # a bank in use as a combiner refuses a list that exceeds its plan, and goes on with the one it had
    with pytest.raises(dabgpu.DabGpuError) as err:
        cb.set_params([CM.to_struct(c, dabgpu.ChanneliserChannel) for c in chs + [CM.channel(stream=2)]], 0)
    assert "13 channels, the bank was created with 12" in str(err.value)
    with pytest.raises(dabgpu.DabGpuError) as err:
        cb.set_params([CM.to_struct(c, dabgpu.ChanneliserChannel) for c in [CM.channel(stream=2)] * 9], 0)
    assert "more than 8 channels" in str(err.value)
    got, ok = run_device(cb, False, blocks12, 100, True)
    assert ok and cb.n_channels == 12 and same_bits(got, CM.host_combine(host, chs, 3, F, blocks12, 4000, 0, 100, True))
    cb.close()
