"""-m gpu: the interferer on the device (dabgpu_interferer_bank_*, dab-radio_amd/csrc/interferer.hip) against the host model -- the same
interferer_core.h under g++ (tests/cpp/interferer_host_model.cpp) -- bit for bit; the host model is tied to the independent numpy model by
tests/test_interferer_model.py.  Small shapes: at most two tiles of 1024 samples plus an odd remainder."""
import numpy as np
import pytest

import interferer_model as IM
import signal_bank_cases as SB

pytestmark = pytest.mark.gpu

N_MAX = 2 * 1024 + 331
N_OUTS = (1, 5, 1023, 1024, 1025, N_MAX)
POSITIONS = (0, 1, 3, 15, 63, 1023, 1025, (1 << 40) + 3)        # L - 1 for L = 2, 16, 64; a multiple of 1024 +- 1; the counter's high word
WIDTHS = (0.3, 96000.0 / 2048000.0, 2.0 ** -7, 0.6)             # L = 2, 16, 64, 1
GUARD = 0xA5
same_bits = SB.same_bits


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return IM.build_host_model(tmp_path_factory.mktemp("interferer_host_model"))


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shapes():
    import dabgpu
    out = [dabgpu.interferer_design(w) for w in WIDTHS]
    assert [H.interp for H in out] == [2, 16, 64, 1]
    return out


@pytest.fixture(scope="module")
def x3():
    rng = np.random.default_rng(7200)
    return (rng.standard_normal((3, N_MAX + 1)) + 1j * rng.standard_normal((3, N_MAX + 1))).astype(np.complex64)      # rows an even count apart


def q64(cycles):
    return int(round(cycles * 2 ** 64)) & IM.M64


def streams3():
    """four sources of mixed kinds -- a tone, the L = 16 band with a gate edge inside a tile, white bursts of period 1 (always on through the
    gate's arithmetic) and the L = 64 band; a stream with no live source; the L = 2 and L = 1 bands, a tone gated on the tile boundary and an
    ungated white source"""
    return [
        IM.stream([IM.source(IM.TONE, amp=0.7, freq_q64=q64(0.0123), phase0_q64=1 << 62),
                   IM.source(IM.BAND, amp=1.3, shape=1, freq_q64=q64(0.146484375), gate_period=700, gate_on=450, gate_offset=-13),
                   IM.source(IM.BAND, amp=0.5, shape=-1, freq_q64=q64(-0.2), gate_period=1, gate_on=1),
                   IM.source(IM.BAND, amp=2.0, shape=2, phase0_q64=3 << 61)], seed=0x1234567890abcdef),
        IM.stream([IM.source(IM.OFF, amp=1.0), IM.source(IM.TONE, amp=0.0, freq_q64=5), IM.source(IM.BAND, amp=1.0, shape=0, gate_period=9, gate_on=0)], seed=3),
        IM.stream([IM.source(IM.BAND, amp=0.9, shape=0, freq_q64=q64(0.31)),
                   IM.source(IM.TONE, amp=1.1, freq_q64=q64(-0.4999), gate_period=1024, gate_on=512, gate_offset=0),
                   IM.source(IM.BAND, amp=0.4, shape=3),
                   IM.source(IM.BAND, amp=0.8, shape=-1, gate_period=(1 << 40) + 2048, gate_on=(1 << 40) + 1030, gate_offset=-5)], seed=99),
    ]


def g_streams(plist):
    import dabgpu
    return [IM.to_struct(P, dabgpu.InterfererStream) for P in plist]


def m_shapes(shapes):
    return [IM.Shape.from_buffer_copy(bytes(H)) for H in shapes]


def run_device(bank, x, n_out, fmt=IM.F32, scale=1.0, shared=False, in_place=False):
    """one apply into guarded rows -> ([n][n_out] complex64 or [n][n_out][2] u8, guards intact).  x: [n][>= n_out] complex64 with an even row
    length, [>= n_out] for a shared row, or None; in_place: the rows are copied into the output first and d_in = d_out"""
    import torch
    sb = 8 if fmt == IM.F32 else 2
    stride = ((n_out * sb + 15) & ~15) + 32                                  # guard bytes between the rows
    whole = torch.full((48 + bank.n * stride + 48,), GUARD, dtype=torch.uint8, device="cuda")
    view = whole[48:48 + bank.n * stride]
    if x is None:
        bank.apply(None, n_out, view, out_format=fmt, out_stride_bytes=stride, u8_scale=scale)
    elif in_place:
        rows = view.view(bank.n, stride)
        rows[:, :n_out * 8] = torch.from_numpy(np.ascontiguousarray(x[:, :n_out]).view(np.uint8).reshape(bank.n, -1)).cuda()
        bank.apply(view, n_out, view, in_stride_samples=stride // 8, out_format=fmt, out_stride_bytes=stride)
    else:
        d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        bank.apply(d_in, n_out, view, in_stride_samples=0 if shared else x.shape[-1], out_format=fmt, out_stride_bytes=stride, u8_scale=scale)
    torch.cuda.synchronize()
    h = whole.cpu().numpy()
    rows = h[48:48 + bank.n * stride].reshape(bank.n, stride)
    ok = bool(np.all(h[:48] == GUARD) and np.all(h[-48:] == GUARD) and np.all(rows[:, n_out * sb:] == GUARD))
    data = np.ascontiguousarray(rows[:, :n_out * sb])
    return (data.view(np.complex64) if fmt == IM.F32 else data.reshape(bank.n, n_out, 2)), ok


@pytest.mark.parametrize("n_streams", [1, 3])
def test_every_length_at_every_position_equals_the_host_model(host, ctx, shapes, x3, n_streams):
    """q - t < 0 at position 0, every L, odd starts, the tile edges, the high counter word; stream 1 (no live source) returns its input"""
    import dabgpu
    plist = streams3()[:n_streams]
    bank = dabgpu.Interferer(ctx, g_streams(plist), shapes)
    assert bank.plan["band_slots"] == 2 and bank.plan["lds_bytes"] == bank.plan["band_slots"] * bank.plan["slot_bytes"]
    x = x3[:n_streams]
    ms = m_shapes(shapes)
    for pos in POSITIONS:
        for n_out in N_OUTS:
            bank.seek(pos)
            got, ok = run_device(bank, x, n_out)
            assert ok, "guard bytes before, between or after the rows were written"
            assert same_bits(got, IM.host_apply(host, plist, ms, x, pos, n_out)), f"position {pos}, {n_out} samples"
            if n_streams == 3:
                assert same_bits(got[1], x[1, :n_out])
    bank.close()


@pytest.mark.parametrize("fmt,scale", [(IM.F32, 1.0), (IM.U8, 9.0), (IM.U8, 30.0)])
def test_no_input_shared_row_in_place_and_u8(host, ctx, shapes, x3, fmt, scale):
    import dabgpu
    plist = streams3()
    bank = dabgpu.Interferer(ctx, g_streams(plist), shapes)
    ms = m_shapes(shapes)
    pos = 0
    for n_out in (N_MAX, 1029):                                              # the second call continues the stream from an odd position
        got, ok = run_device(bank, None, n_out, fmt, scale)
        assert ok and same_bits(got, IM.host_apply(host, plist, ms, None, pos, n_out, fmt, scale)), f"no input at {pos}"
        pos += n_out
        got, ok = run_device(bank, x3[2], n_out, fmt, scale, shared=True)
        assert ok and same_bits(got, IM.host_apply(host, plist, ms, x3[2], pos, n_out, fmt, scale)), f"shared row at {pos}"
        pos += n_out
        got, ok = run_device(bank, x3, n_out, fmt, scale)
        assert ok and same_bits(got, IM.host_apply(host, plist, ms, x3, pos, n_out, fmt, scale)), f"rows at {pos}"
        pos += n_out
        if fmt == IM.F32:
            got, ok = run_device(bank, x3, n_out, in_place=True)
            assert ok and same_bits(got, IM.host_apply(host, plist, ms, x3, pos, n_out)), f"in place at {pos}"
            pos += n_out
    bank.close()


def test_tones_only_bank_and_gate_edges(host, ctx, x3):
    """a bank without shaped sources (the kernel variant without LDS): gate edges inside a tile, on the tile boundary, period 1, gate_on =
    gate_period, a negative offset, and periods around the stepped form's threshold"""
    import dabgpu
    gates = [(700, 450, -13), (1024, 512, 0), (1, 1, 0), (1, 0, 0), (7, 7, 3), (4095, 4000, 5), (4096, 1, -1), (4097, 4096, 1 << 35), (3, 1, 2)]
    plist = [IM.stream([IM.source(IM.TONE if i % 2 == 0 else IM.BAND, amp=1.0 + 0.1 * i, freq_q64=q64(0.01 * (i + 1)), gate_period=p, gate_on=on,
                                  gate_offset=off) for i, (p, on, off) in enumerate(gates[j:j + 3])], seed=50 + j) for j in (0, 3, 6)]
    bank = dabgpu.Interferer(ctx, g_streams(plist))
    assert bank.plan == {"block_samples": 1024, "band_slots": 0, "slot_bytes": 0, "lds_bytes": 0}
    for pos in (0, 1021, (1 << 40) + 3):
        bank.seek(pos)
        got, ok = run_device(bank, x3, N_MAX)
        assert ok and same_bits(got, IM.host_apply(host, plist, [], x3, pos, N_MAX)), f"position {pos}"
    bank.close()


def test_split_calls_equal_one_call(host, ctx, shapes, x3):
    import dabgpu
    plist = streams3()
    one, split = dabgpu.Interferer(ctx, g_streams(plist), shapes), dabgpu.Interferer(ctx, g_streams(plist), shapes)
    whole, ok = run_device(one, x3, N_MAX)
    assert ok
    at = 0
    for n in (1, 7, 1023, 2, N_MAX - 1033):
        xs = np.ascontiguousarray(x3[:, at:at + n + (n & 1)])               # the following input, rows an even count apart
        part, ok = run_device(split, xs, n)
        assert ok and same_bits(part, whole[:, at:at + n]), f"call of {n} samples at {at}"
        at += n
    assert at == N_MAX
    one.close(); split.close()


def test_graph_replays_continue_the_stream_and_set_params_retunes(host, ctx, shapes, x3):
    """a captured call replayed three times equals one long host-model run; _set_params between replays retunes within the geometry"""
    import dabgpu
    import torch
    plist = streams3()
    bank = dabgpu.Interferer(ctx, g_streams(plist), shapes)
    ms = m_shapes(shapes)
    n = 1029
    d_in = torch.from_numpy(np.ascontiguousarray(x3[:, :n + 1])).cuda()
    stride = (n * 8 + 15) & ~15
    out = torch.zeros(3 * stride, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        bank.apply(d_in, n, out, in_stride_samples=n + 1, out_stride_bytes=stride, stream=side.cuda_stream)
    xin = x3[:, :n]
    long_run = IM.host_apply(host, plist, ms, np.tile(xin, (1, 3)), 0, 3 * n)   # every replay reads the same rows
    for r in range(3):                                                       # (capturing enqueued nothing: the position is still 0)
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(3, stride)[:, :n * 8].copy().view(np.complex64)
        assert same_bits(got, long_run[:, r * n:(r + 1) * n]), f"replay {r}"
    retuned = [plist[2], plist[0], plist[1]]
    bank.set_params(g_streams(retuned))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(3, stride)[:, :n * 8].copy().view(np.complex64)
    assert same_bits(got, IM.host_apply(host, retuned, ms, xin, 3 * n, n)), "replay after set_params"
    bank.close()


def test_set_params_must_fit_the_geometry_of_creation(host, ctx, shapes, x3):
    import dabgpu
    one_band = [IM.stream([IM.source(IM.BAND, amp=1.0, shape=1)], seed=1)] * 3
    bank = dabgpu.Interferer(ctx, g_streams(one_band), shapes)
    with pytest.raises(dabgpu.DabGpuError) as err:
        bank.set_params(g_streams(streams3()))
    assert "created for 1" in str(err.value)
    narrower = [IM.stream([IM.source(IM.TONE, amp=1.0, freq_q64=q64(0.25))], seed=2), IM.stream([], seed=0),
                IM.stream([IM.source(IM.BAND, amp=0.0, shape=0), IM.source(IM.BAND, amp=1.0, shape=2)], seed=4)]
    bank.set_params(g_streams(narrower))
    got, ok = run_device(bank, x3, N_MAX)
    assert ok and same_bits(got, IM.host_apply(host, narrower, m_shapes(shapes), x3, 0, N_MAX))
    bank.close()
    tones = dabgpu.Interferer(ctx, g_streams(narrower[:2]), shapes)
    with pytest.raises(dabgpu.DabGpuError) as err:
        tones.set_params(g_streams(one_band[:2]))
    assert "created for 0" in str(err.value)
    tones.close()


def test_host_form_seek_and_every_refusal(host, ctx, shapes, x3):
    import dabgpu
    import torch
    plist = streams3()
    bank = dabgpu.Interferer(ctx, g_streams(plist), shapes)
    ms = m_shapes(shapes)
    got = bank.apply_host(x3, 1029, in_stride_samples=x3.shape[-1])
    assert same_bits(got, IM.host_apply(host, plist, ms, x3, 0, 1029))
    got = bank.apply_host(None, 77, out_format=IM.U8, u8_scale=20.0)
    assert same_bits(got, IM.host_apply(host, plist, ms, None, 1029, 77, IM.U8, 20.0))
    bank.seek((1 << 62) - 1)
    got = bank.apply_host(x3[0], 300)
    assert same_bits(got, IM.host_apply(host, plist, ms, x3[0], (1 << 62) - 1, 300))
    bank.seek(5)
    # refused before any device call: the position does not move, the output keeps its bytes
    n = 1029
    d_in = torch.from_numpy(x3).cuda()
    d_out = torch.full((3 * 1040 * 8,), GUARD, dtype=torch.uint8, device="cuda")
    stride_in = x3.shape[-1]
    bad = [
        (dict(out_format=3), "output format"),
        (dict(n_out=(1 << 31) + 1), "n_out"),
        (dict(in_stride_samples=n - 1), "in_stride_samples"),
        (dict(in_stride_samples=n), "in_stride_samples"),                    # odd
        (dict(out_stride_bytes=n * 8 - 8), "out_stride_bytes"),
        (dict(out_stride_bytes=1040 * 8 + 8), "out_stride_bytes"),
        (dict(d_out=d_out[8:]), "16-byte aligned"),
        (dict(d_in=d_in.view(torch.uint8).reshape(-1)[8:]), "16-byte aligned"),
        (dict(d_out=None), "null output"),
        (dict(d_in=d_out, in_stride_samples=1040, out_format=IM.U8, out_stride_bytes=1040 * 8), "in place"),
        (dict(d_in=d_out, in_stride_samples=1042, out_stride_bytes=1040 * 8), "in place"),
        (dict(out_format=IM.U8, u8_scale=float("nan")), "u8_scale"),
    ]
    for change, text in bad:
        a = dict(d_in=d_in, n_out=n, d_out=d_out, in_stride_samples=stride_in, out_stride_bytes=1040 * 8)
        a.update(change)
        with pytest.raises(dabgpu.DabGpuError) as err:
            bank.apply(**a)
        assert text in str(err.value), (change, str(err.value))
    with pytest.raises(dabgpu.DabGpuError) as err:
        bank.seek(1 << 62)
    assert "2^62" in str(err.value)
    with pytest.raises(dabgpu.DabGpuError) as err:
        dabgpu.Interferer(ctx, g_streams([IM.stream([IM.source(IM.BAND, amp=1.0, shape=4)])]), shapes)
    assert "shape 4 of 4" in str(err.value)
    torch.cuda.synchronize()
    assert bool((d_out == GUARD).all())
    got, ok = run_device(bank, x3, 100)
    assert ok and same_bits(got, IM.host_apply(host, plist, ms, x3, 5, 100))
    bank.close()


def test_host_form_three_calls_regrow_the_buffers_of_one_bank(host, ctx, shapes, x3):
    import dabgpu
    plist = streams3()
    bank = dabgpu.Interferer(ctx, g_streams(plist), shapes)
    ms = m_shapes(shapes)
    L = dabgpu.lib()

    def host_sync(x, n_out, wrap, fmt, out, stride):
        dabgpu.check(L.dabgpu_interferer_bank_apply_host_sync(bank._h, x.ctypes.data, x.shape[-1], n_out, out.ctypes.data, fmt, stride, 9.0), "host form")

    pos = SB.host_form_regrowth(host_sync, lambda x, pos, n_out, wrap, fmt: IM.host_apply(host, plist, ms, x, pos, n_out, fmt, 9.0), x3, 3, IM.F32, IM.U8)
    assert pos == SB.HOST_TOTAL
    got, ok = run_device(bank, x3, 300)
    assert ok and same_bits(got, IM.host_apply(host, plist, ms, x3, pos, 300))
    bank.close()


def test_handle_closes_twice_and_goes_with_its_last_reference(ctx, shapes):
    import dabgpu
    SB.handle_lifecycle(lambda: dabgpu.Interferer(ctx, g_streams(streams3()), shapes))
