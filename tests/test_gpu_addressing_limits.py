"""-m gpu: the planners' accepted limits, run.  The signal-path banks take n_out and max_samples_per_call up to 2^31 -- pinned by the
test_*_plan.py files and the fuzzers, never launched -- and 2^31 is exactly where an `int` sample index or a 32-bit `tile * 1024`
breaks.  Each bank's output depends on (parameters, absolute position) alone, so the ends of one 2^31-sample call equal short calls at
the same positions, and those equal the host models.  u8 output, a short or no input: 4 GiB of output is the only large buffer.

Not here, for the 12 GiB a test may hold: the blanker (complex float in and out, 16 GiB each, no wrapped or shared short input)."""
import numpy as np
import pytest

import big_buffers as BB
import channel_model as CM
import interferer_model as IM

pytestmark = pytest.mark.gpu

N_BIG = 1 << 31
N_END = 8192


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


def q64(cycles):
    return int(round(cycles * 2 ** 64)) & IM.M64


def short_u8(apply, n):
    """one call of n samples into a guarded buffer -> [n][2] u8"""
    import torch
    d = torch.full((n * 2 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    apply(d[32:32 + 2 * n])
    torch.cuda.synchronize()
    h = d.cpu().numpy()
    assert (h[:32] == 0xA5).all() and (h[-32:] == 0xA5).all()
    return h[32:-32].reshape(n, 2)


def big_output():
    """(view of 2^31 u8 pairs, canaries behind it and where a store with a 32-bit byte or sample offset would land)"""
    view = BB.big(2 * N_BIG + BB.CANARY_BYTES)
    can = BB.Canaries()
    can.at(view, 2 * N_BIG)                                              # behind the output
    can.at(view, -BB.CANARY_BYTES)                                       # in front of it
    can.at(view, -BB.LEAD)                                               # 2 * (int32_t)2^31 = -2^32 is outside; -2^31 is the lead's start
    return view, can


def test_interferer_at_the_planner_limit(ctx, tmp_path_factory):
    import dabgpu
    import torch
    host = IM.build_host_model(tmp_path_factory.mktemp("interferer_host_model"))
    shapes = [dabgpu.interferer_design(96000.0 / 2048000.0)]
    assert shapes[0].interp == 16
    # a tone, white noise, a shaped band behind a gate whose period is no divisor of the tile: edges fall anywhere in the last tiles
    plist = [IM.stream([IM.source(IM.TONE, amp=0.7, freq_q64=q64(0.0123), phase0_q64=1 << 62),
                        IM.source(IM.BAND, amp=0.5, shape=-1),
                        IM.source(IM.BAND, amp=1.3, shape=0, freq_q64=q64(0.146484375), gate_period=700, gate_on=450, gate_offset=-13)], seed=0x1234567890abcdef)]
    ms = [IM.Shape.from_buffer_copy(bytes(H)) for H in shapes]
    bank = dabgpu.Interferer(ctx, [IM.to_struct(P, dabgpu.InterfererStream) for P in plist], shapes)
    scale = 30.0
    view, can = big_output()
    bank.apply(None, N_BIG, view, out_format=IM.U8, u8_scale=scale)
    torch.cuda.synchronize()
    can.check()
    # the position word is 2^31 now: the next call continues there
    after = short_u8(lambda d: bank.apply(None, N_END, d, out_format=IM.U8, u8_scale=scale), N_END)
    assert np.array_equal(after, IM.host_apply(host, plist, ms, None, N_BIG, N_END, IM.U8, scale)[0])
    for pos in (0, N_BIG - N_END):
        bank.seek(pos)
        part = short_u8(lambda d: bank.apply(None, N_END, d, out_format=IM.U8, u8_scale=scale), N_END)
        assert np.array_equal(part, IM.host_apply(host, plist, ms, None, pos, N_END, IM.U8, scale)[0]), pos
        assert np.array_equal(BB.get(view, 2 * pos, 2 * N_END).reshape(N_END, 2), part), f"the 2^31-sample call differs from a short call at {pos}"
        assert len(np.unique(part)) > 50
    bank.close()
    del view, can
    BB.release()


def test_channel_at_the_planner_limit(ctx, tmp_path_factory):
    """a short input that repeats (wrap), two taps, carrier offset and noise: the staged kernel over 2^21 tiles"""
    import dabgpu
    import torch
    host = CM.build_host_model(tmp_path_factory.mktemp("channel_host_model"))
    rng = np.random.default_rng(8100)
    n_in = 5000
    x = (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in)).astype(np.complex64)
    plist = [CM.params_dict(taps=((0, 1.0, 0.0), (37, 0.4, -0.3)), freq_q64=q64(0.0007), phase0_q64=1 << 61, start=-3, seed=77, gain=0.9, noise_sigma=0.2)]
    ch = dabgpu.Channel(ctx, [CM.to_struct(P, dabgpu.ChannelStream) for P in plist])
    d_in = torch.from_numpy(x).cuda()
    scale = 30.0
    view, can = big_output()
    ch.apply(d_in, n_in, N_BIG, view, wrap=True, out_format=CM.U8, u8_scale=scale)
    torch.cuda.synchronize()
    can.check()
    after = short_u8(lambda d: ch.apply(d_in, n_in, N_END, d, wrap=True, out_format=CM.U8, u8_scale=scale), N_END)
    assert np.array_equal(after, CM.host_apply(host, plist, x[None], N_BIG, N_END, True, CM.U8, scale)[0])
    for pos in (0, N_BIG - N_END):
        ch.seek(pos)
        part = short_u8(lambda d: ch.apply(d_in, n_in, N_END, d, wrap=True, out_format=CM.U8, u8_scale=scale), N_END)
        assert np.array_equal(part, CM.host_apply(host, plist, x[None], pos, N_END, True, CM.U8, scale)[0]), pos
        assert np.array_equal(BB.get(view, 2 * pos, 2 * N_END).reshape(N_END, 2), part), f"the 2^31-sample call differs from a short call at {pos}"
        assert len(np.unique(part)) > 50
    ch.close()
    del view, can
    BB.release()


def test_iq_balance_with_the_largest_call_limit(ctx):
    """max_samples_per_call = 2^31 sizes the bank's tile scratch for 2^21 tiles per stream; a normal 65 536-sample call must not notice:
    output, records and tile sums of three calls in a row equal a bank created for 65 536 samples"""
    import dabgpu
    import torch
    n, n_streams = 65536, 2
    rng = np.random.default_rng(8200)
    x = (rng.standard_normal((3, n_streams, n)) + 1j * rng.standard_normal((3, n_streams, n))).astype(np.complex64)
    x = (x + 0.2 * np.conj(x) + (0.05 - 0.02j)).astype(np.complex64)             # an image and a DC term for the tracker to find
    params = [dabgpu.iqbal_stream(), dabgpu.iqbal_stream(forget=dabgpu.iqbal_forget(4 * 65536.0))]
    assert dabgpu.iqbal_plan(params, N_BIG)["tiles_per_call"] == 1 << 21
    banks = [dabgpu.IqBalance(ctx, params, limit) for limit in (N_BIG, n)]
    assert banks[0].plan["tiles_per_call"] == 1 << 21 and banks[1].plan["tiles_per_call"] == 64
    flags = dabgpu.IQBAL_APPLY | dabgpu.IQBAL_MEASURE
    for k in range(3):
        d_in = torch.from_numpy(x[k]).cuda()
        outs = []
        for b in banks:
            d_out = torch.zeros((n_streams, n, 2), dtype=torch.float32, device="cuda")
            b.apply(d_in, n, d_out, flags=flags, in_stride_samples=n)
            torch.cuda.synchronize()
            outs.append(d_out)
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), f"call {k}: output"
        assert banks[0].read_state().tobytes() == banks[1].read_state().tobytes(), f"call {k}: records"
        assert banks[0].read_moments(64).tobytes() == banks[1].read_moments(64).tobytes(), f"call {k}: tile sums"
        if k == 2:
            assert not torch.equal(outs[0].view(torch.int32), d_in.view(torch.float32).view(torch.int32).reshape(n_streams, n, 2)), \
                "after 131 072 samples the tracker must have left the identity"
    for b in banks:
        b.close()
