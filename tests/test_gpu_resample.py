"""-m gpu: the resampler on the device (dabgpu_resample_bank_*, dab-radio_amd/csrc/resample.hip) against the host model -- the same
resample_core.h under g++ (tests/cpp/resample_host_model.cpp) -- bit for bit; the host model is tied to the independent numpy model and to
the closed form by tests/test_resample_model.py.  Small shapes: one output, one block of 1024 and its neighbours, two blocks and one."""
import ctypes as C

import numpy as np
import pytest

import resample_model as RM
import signal_bank_cases as SB

pytestmark = pytest.mark.gpu

ONE = RM.ONE
N_IN = 3001                                  # no block size divides it
GUARD = 0xA5
W_MAX = ONE - (1 << 39)                      # row L - 1 with w = 1 - 2^-15: the interpolation into row L
STEP_UP, STEP_DOWN = ONE + (1 << 47), ONE - (1 << 47)          # 1 +- 2^-15
STEPS7 = [ONE, STEP_UP, STEP_DOWN, ONE >> 1, ONE << 1, RM.step_q62(2.4e6, 2.048e6), RM.step_q62(2.048e6, 2.4e6)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return RM.build_host_model(tmp_path_factory.mktemp("resample_host_model"))


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def x3():
    rng = np.random.default_rng(7300)
    return (rng.standard_normal((3, N_IN)) + 1j * rng.standard_normal((3, N_IN))).astype(np.complex64)


def bank(ctx, host, plist, max_step=2.0):
    """(device bank, the host model's design record): both from the same dabgpu_resample_design source, compared here once per table"""
    import dabgpu
    D = RM.host_design(host, max_step)
    G = dabgpu.resample_design(max_step)
    assert np.array_equal(np.ctypeslib.as_array(G.table), np.ctypeslib.as_array(D.table)) and G.error == D.error
    return dabgpu.Resampler(ctx, [RM.to_struct(P, dabgpu.ResampleStream) for P in plist], G), D


def run_device(rs, x, n_out, wrap, fmt=RM.F32, scale=1.0, shared=False):
    """one apply into guarded rows -> ([n][n_out] complex64 or [n][n_out][2] u8, guards intact)"""
    import torch
    sb = 8 if fmt == RM.F32 else 2
    stride = ((n_out * sb + 15) & ~15) + 32                                  # guard bytes between the rows
    whole = torch.full((48 + rs.n * stride + 48,), GUARD, dtype=torch.uint8, device="cuda")
    view = whole[48:48 + rs.n * stride]
    n_in = x.shape[-1]
    pad = np.zeros(x.shape[:-1] + (n_in + (n_in & 1),), np.complex64)        # rows an even count apart
    pad[..., :n_in] = x
    d_in = torch.from_numpy(pad).cuda()
    rs.apply(d_in, n_in, n_out, view, in_stride_samples=0 if shared else pad.shape[-1], wrap=wrap, out_format=fmt, out_stride_bytes=stride,
             u8_scale=scale)
    torch.cuda.synchronize()
    h = whole.cpu().numpy()
    rows = h[48:48 + rs.n * stride].reshape(rs.n, stride)
    ok = bool(np.all(h[:48] == GUARD) and np.all(h[-48:] == GUARD) and np.all(rows[:, n_out * sb:] == GUARD))
    data = np.ascontiguousarray(rows[:, :n_out * sb])
    return (data.view(np.complex64) if fmt == RM.F32 else data.reshape(rs.n, n_out, 2)), ok


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def streams7():
    """every step of the list; offsets on row 0, on row L - 1 at the largest w, on w = 0 of a middle row; a negative start and one past the end"""
    fracs = [0, 0, W_MAX, 200 << 54, W_MAX, 0, (77 << 54) + 12345]
    starts = [-3, -40, 0, 5, -1000, N_IN - 500, 17]
    return [RM.params_dict(s, o, f, gain=1.0 if k % 2 == 0 else -0.5) for k, (s, o, f) in enumerate(zip(STEPS7, starts, fracs))]


@pytest.mark.parametrize("n_out", [1, 2, 1023, 1024, 1025, 2049])
def test_seven_steps_equal_the_host_model(host, ctx, x3, n_out):
    plist = streams7()
    rs, D = bank(ctx, host, plist)
    assert rs.plan == {"block_samples": 1024, "window_samples": 2048 + 48 + 2, "table_rows": 257, "lds_bytes": 2098 * 8 + 257 * 49 * 4}
    for wrap in (False, True):
        rs.seek(0)
        got, ok = run_device(rs, x3[0], n_out, wrap, shared=True)
        assert ok, "guard bytes before, between or after the rows were written"
        exp = RM.host_apply(host, plist, D, x3[0], 0, n_out, wrap)
        for k in range(len(plist)):
            assert same_bits(got[k], exp[k]), f"stream {k}, wrap {wrap}"
    assert same_bits(got[0, 3:], x3[0, :max(n_out - 3, 0)])                         # the identity stream: its input, three samples late
    rs.close()


def near_one_streams():
    """steps 1 +- 2^-15 and exactly 1 with a fraction: a block touches about 8 rows.  Offsets that make the block pass the end of the row
    circle in either direction (row L - 1 -> row L -> row 0 rising, row 0 -> row L - 1 falling), start on row 0 and sit on w = 0"""
    return [RM.params_dict(STEP_UP, -30, W_MAX), RM.params_dict(STEP_DOWN, 3, 1 << 39), RM.params_dict(STEP_UP, 0, 0),
            RM.params_dict(STEP_DOWN, -5, 0), RM.params_dict(ONE, 7, W_MAX, gain=2.0), RM.params_dict(ONE, -2, 0), RM.params_dict(STEP_UP, 11, 250 << 54)]


@pytest.mark.parametrize("max_step", [1.0001, 2.0])
def test_near_one_rows_in_a_narrow_and_in_a_full_bank(host, ctx, x3, max_step):
    """the same streams in a bank that stages a handful of rows (created with near-1 steps only) and in one that may stage the whole table"""
    plist = near_one_streams() + ([RM.params_dict(STEPS7[5], 0, 5)] if max_step == 2.0 else [])       # (2.4 -> 2.048 MS/s: every row)
    rs, D = bank(ctx, host, plist, max_step)
    assert rs.plan["table_rows"] == (257 if max_step == 2.0 else host.rsm_rows_needed(C.byref(RM.to_struct(plist[0]))))
    if max_step != 2.0:
        assert rs.plan["table_rows"] <= 16 and rs.plan["window_samples"] == 1025 + 48 + 2
    for wrap in (False, True):
        rs.seek(0)
        pos = 0
        for n_out in (2049, 1025):                                           # the second call starts 2049 samples on: other rows
            got, ok = run_device(rs, x3[1], n_out, wrap, shared=True)
            assert ok and same_bits(got, RM.host_apply(host, plist, D, x3[1], pos, n_out, wrap)), (wrap, pos)
            pos += n_out
    rs.close()


def test_three_streams_with_different_steps_strided_and_shared(host, ctx, x3):
    plist = [RM.params_dict(RM.step_q62(2.4e6, 2.048e6, 20.0), -10, 1 << 60), RM.params_dict(RM.step_q62(1.0, 1.0, -200.0), 40, W_MAX, gain=0.25),
             RM.params_dict(ONE >> 1, 1000, 3 << 59)]
    rs, D = bank(ctx, host, plist)
    for shared in (False, True):
        x = x3[2] if shared else x3
        for wrap in (False, True):
            rs.seek(0)
            got, ok = run_device(rs, x, 2049, wrap, shared=shared)
            assert ok and same_bits(got, RM.host_apply(host, plist, D, x, 0, 2049, wrap)), (shared, wrap)
    # the Python host form (Resampler.apply_host): rows an odd count apart and a shared row, complex float and u8
    rs.seek(0)
    assert same_bits(rs.apply_host(x3, 1029, in_stride_samples=N_IN, wrap=True), RM.host_apply(host, plist, D, x3, 0, 1029, True))
    got = rs.apply_host(x3[2], 77, wrap=False, out_format=RM.U8, u8_scale=30.0)
    assert got.shape == (3, 77, 2) and same_bits(got, RM.host_apply(host, plist, D, x3[2], 1029, 77, False, RM.U8, 30.0))
    rs.close()


def test_far_positions_exercise_the_128_bit_time(host, ctx, x3):
    """a seek to 2^40 + 3 and to the position limit minus a block; with step 2 and offset_samples = +2^62 the index passes 2^63 + 2^62 (its
    65th bit); with the offset that cancels m * step the window lies inside the input again (zero-fill, no wrap)"""
    limit = RM.MAX_POSITION
    for pos in ((1 << 40) + 3, limit - 1024):
        far = [RM.params_dict(ONE << 1, limit, W_MAX), RM.params_dict(RM.step_q62(2.4e6, 2.048e6), -limit, 123456789),
               RM.params_dict(STEP_UP, 12345, 1 << 61), RM.params_dict(ONE, -7, 0)]
        rs, D = bank(ctx, host, far)
        rs.seek(pos)
        got, ok = run_device(rs, x3[0], 1024, True, shared=True)
        exp = RM.host_apply(host, far, D, x3[0], pos, 1024, True)
        assert ok and same_bits(got, exp), pos
        assert not same_bits(got[0], RM.host_apply(host, far, D, x3[0], pos - 1, 1024, True)[0])
        rs.close()
        # (at the limit only steps up to 1 leave an index that an offset within +-2^62 can cancel)
        steps = (ONE << 1, STEPS7[5], STEP_DOWN) if pos < limit >> 1 else (ONE >> 1, STEPS7[6], STEP_DOWN)
        near = [RM.params_dict(s, 100 - RM.time_of(RM.params_dict(s), pos)[0], f) for s, f in zip(steps, (5, W_MAX, 0))]
        rs, D = bank(ctx, host, near)
        rs.seek(pos)
        got, ok = run_device(rs, x3[0], 1024, False, shared=True)
        exp = RM.host_apply(host, near, D, x3[0], pos, 1024, False)
        assert ok and same_bits(got, exp) and np.abs(exp).min() > 0, pos
        rs.close()


@pytest.mark.parametrize("fmt", [RM.F32, RM.U8])
def test_split_calls_equal_one_call(host, ctx, x3, fmt):
    plist = streams7()
    (one, D), (split, _) = bank(ctx, host, plist), bank(ctx, host, plist)
    total = 2049 + 331
    whole, ok = run_device(one, x3[0], total, True, fmt, scale=30.0, shared=True)
    assert ok and same_bits(whole, RM.host_apply(host, plist, D, x3[0], 0, total, True, fmt, scale=30.0))
    at = 0
    for n in (1, 7, 1023, 2, total - 1033):
        part, ok = run_device(split, x3[0], n, True, fmt, scale=30.0, shared=True)
        assert ok and same_bits(part, whole[:, at:at + n]), f"call of {n} samples at {at}"
        at += n
    assert at == total
    one.close(); split.close()


def test_graph_replays_continue_the_stream(host, ctx, x3):
    import torch
    plist = streams7()[:3] + [RM.params_dict(STEPS7[5], -9, W_MAX)]
    rs, D = bank(ctx, host, plist)
    n = 1029
    pad = np.zeros((4, N_IN + 1), np.complex64)
    pad[:3, :-1] = x3
    pad[3, :-1] = x3[0]
    d_in = torch.from_numpy(pad).cuda()
    stride = (n * 8 + 15) & ~15
    out = torch.zeros(4 * stride, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        rs.apply(d_in, N_IN, n, out, in_stride_samples=N_IN + 1, wrap=True, out_stride_bytes=stride, stream=side.cuda_stream)
    exp = RM.host_apply(host, plist, D, pad[:, :-1].copy(), 0, 3 * n, True)       # one long call
    for r in range(3):                                                       # (capturing enqueued nothing: the position is still 0)
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(4, stride)[:, :n * 8].copy().view(np.complex64)
        assert same_bits(got, exp[:, r * n:(r + 1) * n]), f"replay {r}"
    rs.close()


def test_identity_bank_returns_its_input(host, ctx, x3):
    """a bank of identity streams stages nothing (no table rows); gain 1 returns the input bit for bit, NaN and infinity included"""
    x = x3.copy()
    x[:, 1500] = np.nan
    x[:, 2000] = complex(np.inf, -0.0)
    ident = [RM.params_dict(), RM.params_dict(ONE, 0, 0), RM.params_dict(ONE, -1, 0)]
    rs, D = bank(ctx, host, ident, 1.0)
    assert rs.plan["table_rows"] == 0
    got, ok = run_device(rs, x, N_IN, False)
    assert ok and same_bits(got[0], x[0]) and same_bits(got[1], x[1]) and same_bits(got[2, 1:], x[2, :-1]) and got[2, 0] == 0
    import dabgpu
    with pytest.raises(dabgpu.DabGpuError) as err:                           # created without rows: a filtering stream does not fit
        rs.set_params([RM.to_struct(P, dabgpu.ResampleStream) for P in [RM.params_dict(), RM.params_dict(ONE, 0, 1), RM.params_dict()]])
    assert "table rows" in str(err.value)
    rs.close()
    # NaN and infinity reach only the outputs whose taps cover them
    plist = [RM.params_dict(STEP_UP, 0, 5)] * 3
    rs, D = bank(ctx, host, plist)
    got, ok = run_device(rs, x, 2500, False)
    exp = RM.host_apply(host, plist, D, x, 0, 2500, False)
    bad = ~np.isfinite(exp)
    assert ok and np.array_equal(~np.isfinite(got), bad) and 90 <= bad[0].sum() <= 100
    assert same_bits(got[~bad], exp[~bad])
    rs.close()


def test_host_form_three_calls_regrow_the_buffers_of_one_bank(host, ctx, x3):
    """7 samples out of 64 in, 2049 out of the whole input (both buffers grow), 101 (both larger than needed); then the device form goes on
    from the summed position"""
    import dabgpu
    plist = [RM.params_dict(RM.step_q62(2.4e6, 2.048e6, 20.0), -10, 1 << 60), RM.params_dict(RM.step_q62(1.0, 1.0, -200.0), 40, W_MAX, gain=0.25),
             RM.params_dict(ONE, 3, 0)]                                         # all rows, a few rows, the copy
    rs, D = bank(ctx, host, plist)
    L = dabgpu.lib()

    def host_sync(x, n_out, wrap, fmt, out, stride):
        n_in = x.shape[-1]
        dabgpu.check(L.dabgpu_resample_bank_apply_host_sync(rs._h, x.ctypes.data, n_in, n_in, int(wrap), n_out, out.ctypes.data, fmt, stride, 30.0), "host form")

    pos = SB.host_form_regrowth(host_sync, lambda x, pos, n_out, wrap, fmt: RM.host_apply(host, plist, D, x, pos, n_out, wrap, fmt, 30.0), x3, 3, RM.F32,
                                RM.U8)
    assert pos == SB.HOST_TOTAL
    got, ok = run_device(rs, x3, 300, True)
    assert ok and same_bits(got, RM.host_apply(host, plist, D, x3, pos, 300, True))
    rs.close()


def test_host_form_and_invalid_arguments(host, ctx, x3):
    import dabgpu
    import torch
    plist = streams7()[:3]
    rs, D = bank(ctx, host, plist)
    pad = np.zeros((3, N_IN + 1), np.complex64)
    pad[:, :-1] = x3
    L = dabgpu.lib()
    out = np.zeros((3, 1040 * 8), np.uint8)
    dabgpu.check(L.dabgpu_resample_bank_apply_host_sync(rs._h, pad.ctypes.data, N_IN + 1, N_IN, 1, 1029, out.ctypes.data, RM.F32, 1040 * 8, 1.0), "host form")
    assert same_bits(out[:, :1029 * 8].copy().view(np.complex64), RM.host_apply(host, plist, D, x3, 0, 1029, True))
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
            rs.apply(**a)
        assert text in str(err.value) and "resample_bank_apply" in str(err.value), (change, str(err.value))
    with pytest.raises(dabgpu.DabGpuError) as err:
        rs.apply(d_in, N_IN, 16, d_out, in_stride_samples=N_IN + 1, out_format=RM.U8, u8_scale=float("nan"))
    assert "u8_scale" in str(err.value)
    with pytest.raises(dabgpu.DabGpuError) as err:
        rs.seek((1 << 62) + 1)
    assert "2^62" in str(err.value)
    for change, text in ((dict(step_q62=(ONE << 1) + 1), "outside [0.5, 2]"), (dict(gain=float("inf")), "gain is not finite"),
                         (dict(offset_frac_q62=ONE), "offset_frac_q62"), (dict(offset_samples=(1 << 62) + 1), "offset_samples")):
        with pytest.raises(dabgpu.DabGpuError) as err:
            rs.set_params([RM.to_struct(RM.params_dict(**change), dabgpu.ResampleStream)] * 3)
        assert text in str(err.value), str(err.value)
    torch.cuda.synchronize()
    assert bool((d_out == GUARD).all())
    got, ok = run_device(rs, x3, 100, True)                                  # the stream goes on from where the host form left it
    assert ok and same_bits(got, RM.host_apply(host, plist, D, x3, 1029, 100, True))
    rs.close()
    with pytest.raises(dabgpu.DabGpuError) as err:                           # a step above the design's max_step
        bank(ctx, host, [RM.params_dict(STEP_UP)], 1.0)
    assert "max_step" in str(err.value)
    # a bank created for near-1 steps refuses what needs a wider window or more rows; narrower parameters run
    rs, D = bank(ctx, host, [RM.params_dict(RM.step_q62(1.0, 1.0, 100.0), 0, 1)] * 3, 1.0002)
    with pytest.raises(dabgpu.DabGpuError) as err:
        rs.set_params([RM.to_struct(RM.params_dict(RM.step_q62(1.0, 1.0, 150.0), 0, 1), dabgpu.ResampleStream)] * 3)
    assert "table rows" in str(err.value)
    narrower = [RM.params_dict(RM.step_q62(1.0, 1.0, -20.0), -4, W_MAX)] * 3
    rs.set_params([RM.to_struct(P, dabgpu.ResampleStream) for P in narrower])
    got, ok = run_device(rs, x3, 2049, True)
    assert ok and same_bits(got, RM.host_apply(host, narrower, D, x3, 0, 2049, True))
    rs.close()
