"""-m gpu: the channel model on the device (dabgpu_channel_bank_*, dab-radio_amd/csrc/channel.hip) against the host model -- the same
channel_core.h under g++ (tests/cpp/channel_host_model.cpp) -- bit for bit; the host model is tied to the independent numpy model by
tests/test_channel_model.py.  Small shapes: three tiles of 1024 samples plus an odd remainder."""
import ctypes as C

import numpy as np
import pytest

import channel_model as CM
import signal_bank_cases as SB

pytestmark = pytest.mark.gpu

N_IN, N_OUT = 3 * 1024 + 5, 3 * 1024 + 331
GUARD = 0xA5


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return CM.build_host_model(tmp_path_factory.mktemp("channel_host_model"))


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def x3():
    rng = np.random.default_rng(7100)
    return (rng.standard_normal((3, N_IN)) + 1j * rng.standard_normal((3, N_IN))).astype(np.complex64)


def streams3(noise=True):
    """1, 2 and 8 taps; delays 0, 1, the tile length +- 1, the maximum; start negative, zero, positive past the input's end"""
    return [
        CM.params_dict(taps=[(0, 0.8, -0.3)], noise_sigma=0.25 if noise else 0.0, seed=0x1234567890abcdef, freq_q64=int(0.00123 * 2 ** 64),
                       phase0_q64=1 << 62, start=-41),
        CM.params_dict(taps=[(1, 1.0, 0.0), (1023, 0.35, 0.35)], noise_sigma=0.0, seed=7, freq_q64=(1 << 64) - int(3.3e-4 * 2 ** 64), start=0, gain=0.7),
        CM.params_dict(taps=[(3, 0.5, 0.1), (0, -0.2, 0.9), (1, 0.3, 0.3), (1023, 0.1, 0.0), (1025, 0.0, -0.4), (2047, 0.25, 0.25), (77, -0.6, 0.2),
                             (504, 0.2, -0.1)], noise_sigma=1.5 if noise else 0.0, seed=99, freq_q64=int(0.4999 * 2 ** 64), start=N_IN + 100, gain=2.0),
    ]


def g_streams(plist):
    import dabgpu
    return [CM.to_struct(P, dabgpu.ChannelStream) for P in plist]


def run_device(ch, x, n_out, wrap, fmt=CM.F32, scale=1.0, shared=False):
    """one apply into guarded rows -> ([n][n_out] complex64 or [n][n_out][2] u8, guards intact)"""
    import torch
    sb = 8 if fmt == CM.F32 else 2
    stride = ((n_out * sb + 15) & ~15) + 32                                  # guard bytes between the rows
    whole = torch.full((48 + ch.n * stride + 48,), GUARD, dtype=torch.uint8, device="cuda")
    view = whole[48:48 + ch.n * stride]
    n_in = x.shape[-1]
    pad = np.zeros(x.shape[:-1] + (n_in + (n_in & 1),), np.complex64)        # rows an even count apart
    pad[..., :n_in] = x
    d_in = torch.from_numpy(pad).cuda()
    ch.apply(d_in, n_in, n_out, view, in_stride_samples=0 if shared else pad.shape[-1], wrap=wrap, out_format=fmt, out_stride_bytes=stride,
             u8_scale=scale)
    torch.cuda.synchronize()
    h = whole.cpu().numpy()
    rows = h[48:48 + ch.n * stride].reshape(ch.n, stride)
    ok = bool(np.all(h[:48] == GUARD) and np.all(h[-48:] == GUARD) and np.all(rows[:, n_out * sb:] == GUARD))
    data = np.ascontiguousarray(rows[:, :n_out * sb])
    return (data.view(np.complex64) if fmt == CM.F32 else data.reshape(ch.n, n_out, 2)), ok


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("fmt", [CM.F32, CM.U8])
@pytest.mark.parametrize("wrap", [False, True])
def test_three_streams_equal_the_host_model(host, ctx, x3, wrap, fmt):
    import dabgpu
    plist = streams3()
    ch = dabgpu.Channel(ctx, g_streams(plist))
    assert ch.plan["halo"] == 2048 and ch.plan["staged"] == 1
    pos = 0
    for n_out in (N_OUT, 1029):                                              # the second call continues the stream from an odd position
        got, ok = run_device(ch, x3, n_out, wrap, fmt, scale=9.0)
        exp = CM.host_apply(host, plist, x3, pos, n_out, wrap, fmt, scale=9.0)
        assert ok, "guard bytes before, between or after the rows were written"
        assert same_bits(got, exp), f"position {pos}"
        pos += n_out
    ch.close()


def test_tiny_input_wraps_many_times_and_direct_path(host, ctx):
    """n_in below the staged window (the modulo per sample) and a bank of single zero-delay taps (no staging), odd start"""
    import dabgpu
    rng = np.random.default_rng(7101)
    x = (rng.standard_normal((2, 6)) + 1j * rng.standard_normal((2, 6))).astype(np.complex64)[:, :5]
    x = np.ascontiguousarray(x)
    staged = [CM.params_dict(taps=[(0, 1.0, 0.0), (7, 0.5, -0.5)], start=3), CM.params_dict(taps=[(2047, 0.0, 1.0)], noise_sigma=0.5, seed=3)]
    direct = [CM.params_dict(taps=[(0, 0.6, 0.8)], start=-3, noise_sigma=0.1, seed=1), CM.params_dict(taps=[(0, 1.0, 0.0)], start=1, freq_q64=1 << 50)]
    for plist, is_staged in ((staged, 1), (direct, 0)):
        ch = dabgpu.Channel(ctx, g_streams(plist))
        assert ch.plan["staged"] == is_staged
        for wrap in (True, False):
            ch.seek(0)
            got, ok = run_device(ch, x, 1500, wrap)
            assert ok and same_bits(got, CM.host_apply(host, plist, x, 0, 1500, wrap))
        ch.close()
    big = (rng.standard_normal((2, N_IN + 1)) + 1j * rng.standard_normal((2, N_IN + 1))).astype(np.complex64)[:, :N_IN]
    big = np.ascontiguousarray(big)
    ch = dabgpu.Channel(ctx, g_streams(direct))
    for fmt in (CM.F32, CM.U8):
        for wrap in (True, False):
            ch.seek(0)
            got, ok = run_device(ch, big, N_OUT, wrap, fmt, scale=30.0)
            assert ok and same_bits(got, CM.host_apply(host, direct, big, 0, N_OUT, wrap, fmt, scale=30.0))
    ch.close()


@pytest.mark.parametrize("fmt", [CM.F32, CM.U8])
def test_split_calls_equal_one_call(host, ctx, x3, fmt):
    import dabgpu
    plist = streams3()
    one, split = dabgpu.Channel(ctx, g_streams(plist)), dabgpu.Channel(ctx, g_streams(plist))
    whole, ok = run_device(one, x3, N_OUT, True, fmt, scale=9.0)
    assert ok
    at = 0
    for n in (1, 7, 1023, 2, N_OUT - 1033):
        part, ok = run_device(split, x3, n, True, fmt, scale=9.0)
        assert ok and same_bits(part, whole[:, at:at + n]), f"call of {n} samples at {at}"
        at += n
    assert at == N_OUT
    one.close(); split.close()


def test_position_just_below_2_to_33(host, ctx, x3):
    """the counter's high word and the oscillator's wrap: the stretch crosses m = 2^33"""
    import dabgpu
    plist = streams3()
    ch = dabgpu.Channel(ctx, g_streams(plist))
    pos = (1 << 33) - 1701
    ch.seek(pos)
    got, ok = run_device(ch, x3, N_OUT, True)
    assert ok and same_bits(got, CM.host_apply(host, plist, x3, pos, N_OUT, True))
    lo = CM.host_apply(host, plist, x3, 0, N_OUT, True)
    assert not same_bits(got[0], lo[0])
    ch.close()


def test_no_noise_equals_the_signal_part_and_identity_returns_its_input(host, ctx, x3):
    import dabgpu
    quiet = streams3(noise=False)
    ch = dabgpu.Channel(ctx, g_streams(quiet))
    got, ok = run_device(ch, x3, N_OUT, True)
    assert ok and same_bits(got, CM.host_apply(host, quiet, x3, 0, N_OUT, True))
    # set_params: the same bank with noise differs by the noise alone (float64 check of the difference's scale on stream 0)
    noisy = streams3()
    ch.set_params(g_streams(noisy))
    ch.seek(0)
    got2, ok = run_device(ch, x3, N_OUT, True)
    assert ok and same_bits(got2, CM.host_apply(host, noisy, x3, 0, N_OUT, True))
    assert same_bits(got2[1], got[1])                                        # stream 1 has no noise
    d = (got2[0].astype(np.complex128) - got[0].astype(np.complex128)) / 0.25
    assert abs((np.abs(d) ** 2).mean() / 2 - 1) < 0.1
    ch.close()
    ident = [CM.params_dict()] * 3
    for force in (ident, [CM.params_dict(), CM.params_dict(taps=[(5, 1.0, 0.0)]), CM.params_dict()]):      # direct and staged kernels
        ch = dabgpu.Channel(ctx, g_streams(force))
        got, ok = run_device(ch, x3, N_IN, False)
        assert ok and same_bits(got[0], x3[0]) and same_bits(got[2], x3[2])
        ch.close()


def test_nan_and_inf_reach_only_their_samples(host, ctx, x3):
    import dabgpu
    x = x3.copy()
    x[:, 1500] = np.nan
    x[:, 2000] = complex(np.inf, 1.0)
    plist = [CM.params_dict(taps=[(0, 1.0, 0.0), (200, 0.5, 0.0)], noise_sigma=0.1, seed=4)] * 3
    ch = dabgpu.Channel(ctx, g_streams(plist))
    got, ok = run_device(ch, x, N_IN, False)
    assert ok
    bad = np.zeros(N_IN, bool)
    bad[[1500, 1700, 2000, 2200]] = True
    for s in range(3):
        assert np.array_equal(~np.isfinite(got[s]), bad)
    exp = CM.host_apply(host, plist, x, 0, N_IN, False)
    assert same_bits(got[:, ~bad], exp[:, ~bad])
    ch.close()


def test_graph_replays_continue_the_stream(host, ctx, x3):
    import dabgpu
    import torch
    plist = streams3()
    ch = dabgpu.Channel(ctx, g_streams(plist))
    n = 1029
    pad = np.zeros((3, N_IN + 1), np.complex64)
    pad[:, :-1] = x3
    d_in = torch.from_numpy(pad).cuda()
    stride = (n * 8 + 15) & ~15
    out = torch.zeros(3 * stride, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        ch.apply(d_in, N_IN, n, out, in_stride_samples=N_IN + 1, wrap=True, out_stride_bytes=stride, stream=side.cuda_stream)
    exp = CM.host_apply(host, plist, x3, 0, 2 * n, True)
    for r in range(2):                                                       # (capturing enqueued nothing: the position is still 0)
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(3, stride)[:, :n * 8].copy().view(np.complex64)
        assert same_bits(got, exp[:, r * n:(r + 1) * n]), f"replay {r}"
    ch.close()


def test_host_form_and_invalid_arguments(host, ctx, x3):
    import dabgpu
    import torch
    plist = streams3()
    ch = dabgpu.Channel(ctx, g_streams(plist))
    pad = np.zeros((3, N_IN + 1), np.complex64)
    pad[:, :-1] = x3
    L = dabgpu.lib()
    out = np.zeros((3, 1040 * 8), np.uint8)
    dabgpu.check(L.dabgpu_channel_bank_apply_host_sync(ch._h, pad.ctypes.data, N_IN + 1, N_IN, 1, 1029, out.ctypes.data, CM.F32, 1040 * 8, 1.0), "host form")
    assert same_bits(out[:, :1029 * 8].copy().view(np.complex64), CM.host_apply(host, plist, x3, 0, 1029, True))
    # refused before any device call: the position does not move, the output keeps its bytes
    d_in = torch.from_numpy(pad).cuda()
    d_out = torch.full((3 * 1040 * 8,), GUARD, dtype=torch.uint8, device="cuda")
    bad = [
        (dict(out_format=3), "output format"),
        (dict(n_in=0), "n_in = 0"),
        (dict(in_stride_samples=N_IN - 1), "in_stride_samples"),
        (dict(in_stride_samples=N_IN), "in_stride_samples"),                 # odd
        (dict(out_stride_bytes=1029 * 8 - 8), "out_stride_bytes"),
        (dict(out_stride_bytes=1040 * 8 + 8), "out_stride_bytes"),
        (dict(d_out=d_out[8:]), "16-byte aligned"),
        (dict(d_in=None), "null input"),
    ]
    for change, text in bad:
        a = dict(d_in=d_in, n_in=N_IN, n_out=1029, d_out=d_out, in_stride_samples=N_IN + 1, wrap=True, out_stride_bytes=1040 * 8)
        a.update(change)
        with pytest.raises(dabgpu.DabGpuError) as err:
            ch.apply(**a)
        assert text in str(err.value), (change, str(err.value))
    with pytest.raises(dabgpu.DabGpuError) as err:
        ch.apply(d_in, N_IN, 16, d_out, in_stride_samples=N_IN + 1, out_format=CM.U8, u8_scale=float("nan"))
    assert "u8_scale" in str(err.value)
    torch.cuda.synchronize()
    assert bool((d_out == GUARD).all())
    got, ok = run_device(ch, x3, 100, True)
    assert ok and same_bits(got, CM.host_apply(host, plist, x3, 1029, 100, True))
    with pytest.raises(dabgpu.DabGpuError) as err:
        dabgpu.Channel(ctx, g_streams([CM.params_dict(taps=[(2048, 1.0, 0.0)])]))
    assert "delay 2048" in str(err.value)
    ch.close()


def test_host_form_three_calls_regrow_the_buffers_of_one_bank(host, ctx, x3):
    """7 samples out of 64 in, 2049 out of the whole input (both buffers grow), 101 (both larger than needed); then the device form goes on
    from the summed position"""
    import dabgpu
    plist = streams3()
    ch = dabgpu.Channel(ctx, g_streams(plist))
    L = dabgpu.lib()

    def host_sync(x, n_out, wrap, fmt, out, stride):
        n_in = x.shape[-1]
        dabgpu.check(L.dabgpu_channel_bank_apply_host_sync(ch._h, x.ctypes.data, n_in, n_in, int(wrap), n_out, out.ctypes.data, fmt, stride, 9.0), "host form")

    pos = SB.host_form_regrowth(host_sync, lambda x, pos, n_out, wrap, fmt: CM.host_apply(host, plist, x, pos, n_out, wrap, fmt, scale=9.0), x3, 3, CM.F32,
                                CM.U8)
    assert pos == SB.HOST_TOTAL
    got, ok = run_device(ch, x3, 300, True)
    assert ok and same_bits(got, CM.host_apply(host, plist, x3, pos, 300, True))
    ch.close()


def test_handle_closes_twice_and_goes_with_its_last_reference(ctx):
    import dabgpu
    SB.handle_lifecycle(lambda: dabgpu.Channel(ctx, g_streams(streams3())))


def test_set_params_must_fit_the_geometry_of_creation(host, ctx, x3):
    """a captured call has the kernel variant and the LDS size of the bank's creation baked in: wider parameters are refused, narrower run"""
    import dabgpu
    wide = [CM.params_dict(taps=[(0, 1.0, 0.0), (200, 0.5, 0.0)])] * 3
    ch = dabgpu.Channel(ctx, g_streams(wide))
    with pytest.raises(dabgpu.DabGpuError) as err:
        ch.set_params(g_streams([CM.params_dict(taps=[(0, 1.0, 0.0), (202, 0.5, 0.0)])] * 3))
    assert "halo of 202" in str(err.value)
    narrow = [CM.params_dict(taps=[(0, 0.5, 0.5)], noise_sigma=0.2, seed=8)] * 3            # single taps through the staged kernel
    ch.set_params(g_streams(narrow))
    got, ok = run_device(ch, x3, N_OUT, True)
    assert ok and same_bits(got, CM.host_apply(host, narrow, x3, 0, N_OUT, True))
    ch.close()
    direct = dabgpu.Channel(ctx, g_streams(narrow))
    with pytest.raises(dabgpu.DabGpuError) as err:
        direct.set_params(g_streams(wide))
    assert "staged kernel" in str(err.value)
    with pytest.raises(dabgpu.DabGpuError) as err:
        direct.seek((1 << 62) + 1)
    assert "2^62" in str(err.value)
    direct.close()
