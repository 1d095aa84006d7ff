"""-m gpu: the IQ balance bank on the device (dabgpu_iqbal_bank_*, dab-radio_amd/csrc/iqbal.hip) against the host model -- the same
iqbal_core.h under g++ (tests/cpp/iqbal_host_model.cpp) -- bit for bit: samples, tile moments and state records; the host model is tied
to the independent numpy model by tests/test_iqbal_model.py.  The shapes -- four streams (OFF, FIXED, TRACK fresh, TRACK primed with
forget < 1), MEASURE over 5 tiles, APPLY over 6000 samples = six or seven tiles with partial ones at both ends -- are the smallest at
which the tree's three stages, the tile order of the fold and the edge stores can go wrong."""
import numpy as np
import pytest

import iqbal_model as IM
import signal_bank_cases as SB

pytestmark = pytest.mark.gpu

N_APPLY = 6000
N_IN = 10 * IM.TILE
MAX_CALL = 10 * IM.TILE
GUARD = 0xA5
same_bits = SB.same_bits


def same_but_nan(got, want):
    """bit for bit, except that where the host model holds a NaN the device must hold one too: sign and payload of a NaN that an operation
    makes (inf - inf, 0 x inf) are the processor's own"""
    got, want = (np.ascontiguousarray(v).view(np.float32) for v in (got, want))
    nan = np.isnan(want)
    return bool(np.all(np.isnan(got[nan]))) and same_bits(got[~nan], want[~nan])


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return IM.build_host_model(tmp_path_factory.mktemp("iqbal_host_model"))


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


def streams4():
    K1, K2 = IM.front_end(0.42, 3.0)
    return [IM.params(mode=IM.OFF), IM.params(mode=IM.FIXED, a=K1, b=K2, c=0.3 + 0.2j),
            IM.params(min_weight=1024.0, forget=1.0), IM.params(min_weight=2048.0, forget=0.9)]


def g_streams(plist):
    import dabgpu
    return [IM.to_struct(P, dabgpu.IqBalanceStream) for P in plist]


def noise(rng, shape, sigma=1.0):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * (sigma / np.sqrt(2.0))).astype(np.complex64)


def signal(shared, seed=7, bad=True):
    """impaired noise, a row per stream (its own imbalance each) or one shared row; with bad: a NaN in tile 2 and an infinity in tile 4 of
    row 2 (or of the shared row), and row 3 all zero"""
    rng = np.random.default_rng(seed)
    x = np.stack([IM.impair(noise(rng, N_IN), 0.3 * k + 0.2, 2.0 * k - 3.0, 0.1 * k - 0.2j).astype(np.complex64) for k in range(1 if shared else 4)])
    if bad:
        row = x[0] if shared else x[2]
        row[2 * IM.TILE + 100] = np.nan
        row[4 * IM.TILE + 1023] = np.complex64(complex(0, -np.inf))
        if not shared:
            x[3] = 0
    return x[0] if shared else x


class Pair:
    """a device bank and the host model's records beside it, walked through the same calls"""

    def __init__(self, ctx, host, plist, prime=None):
        import dabgpu
        self.host, self.plist = host, plist
        self.bank = dabgpu.IqBalance(ctx, g_streams(plist), MAX_CALL)
        self.rec = IM.host_records(host, len(plist))
        self.pos = 0
        if prime is not None:                                                # MEASURE over 3 tiles, then back to the start
            self.call(prime, 3 * IM.TILE, IM.MEASURE)
            self.seek(0)

    def seek(self, pos):
        self.bank.seek(pos)
        self.pos = pos

    def call(self, x, n, flags, u8=False, scale=1.0, in_place=False, x_off=0):
        """one device call into guarded rows and the same call of the host model; asserts samples, moments, records and guards.  x_off: the
        call reads the rows from this sample on"""
        import dabgpu
        import torch
        bank, sb = self.bank, 2 if u8 else 8
        xs = np.ascontiguousarray(x[..., x_off:])
        if xs.shape[-1] & 1:
            xs = np.ascontiguousarray(xs[..., :-1])
        stride = ((n * sb + 15) & ~15) + 32
        d_in = torch.from_numpy(xs).cuda()
        in_stride = 0 if xs.ndim == 1 else xs.shape[-1]
        whole = view = None
        if flags & IM.APPLY and not in_place:
            whole = torch.full((48 + bank.n * stride + 48,), GUARD, dtype=torch.uint8, device="cuda")
            view = whole[48:48 + bank.n * stride]
        fmt = dabgpu.IQ_FORMATS.index("raw_u8") if u8 else None
        if in_place:
            bank.apply(d_in, n, d_in, flags=flags, in_stride_samples=in_stride, out_stride_bytes=in_stride * 8)
        else:
            bank.apply(d_in, n, view, flags=flags, in_stride_samples=in_stride, out_format=fmt, out_stride_bytes=stride if view is not None else 0,
                       u8_scale=scale)
        torch.cuda.synchronize()
        want_y, want_m, adv = IM.host_apply(self.host, self.plist, self.rec, xs, self.pos, n, flags, u8=u8, scale=scale)
        where = f"{n} samples at {self.pos}, flags {flags}"
        if flags & IM.APPLY and adv:
            if in_place:
                got = d_in.cpu().numpy()
                assert same_but_nan(got[:, :n], want_y), f"in place: {where}"
                assert same_bits(got[:, n:], xs[:, n:]), f"in place, behind the call: {where}"
            else:
                h = whole.cpu().numpy()
                rows = h[48:48 + bank.n * stride].reshape(bank.n, stride)
                assert np.all(h[:48] == GUARD) and np.all(h[-48:] == GUARD) and np.all(rows[:, n * sb:] == GUARD), f"guard bytes: {where}"
                got = np.ascontiguousarray(rows[:, :n * sb])
                assert same_bits(got.reshape(bank.n, n, 2), want_y) if u8 else same_but_nan(got, want_y), f"samples: {where}"
        elif whole is not None:
            assert bool((whole == GUARD).all()), f"a refused call wrote: {where}"
        if flags & IM.MEASURE and adv:
            assert same_but_nan(bank.read_moments(n // IM.TILE), want_m), f"tile moments: {where}"
        state = bank.read_state()
        for name in state.dtype.names:
            assert same_bits(state[name], self.rec[name]), f"record field {name}: {where}\n{state[name]}\n{self.rec[name]}"
        self.pos += adv
        return adv


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("pos", [0, (1 << 40) + 1024])
def test_measure_equals_the_host_model(host, ctx, pos, shared):
    """5 tiles with a NaN tile, an infinite tile and an all-zero row; then the coefficients they gave applied, float and u8"""
    x = signal(shared)
    p = Pair(ctx, host, streams4(), prime=signal(shared, seed=8, bad=False))
    assert p.bank.plan == {"tile_samples": 1024, "tiles_per_call": 10, "scratch_bytes": 4 * 10 * 32}
    assert p.rec["valid"][3] == 1 and p.rec["tiles_used"][3] == 3
    p.seek(pos)
    assert p.call(x, 5 * IM.TILE, IM.MEASURE) == 5 * IM.TILE
    assert p.rec["tiles_skipped"][2] == 2 and p.rec["valid"][2] == 1
    if not shared:
        assert p.rec["valid"][3] == 1 and p.rec["tiles_used"][3] == 8          # zeros fold in: the primed state decays, P stays positive
    assert p.rec["tiles_used"][0] == p.rec["tiles_used"][1] == 0               # OFF and FIXED streams do not fold
    p.seek(pos)
    p.call(x, 5 * IM.TILE, IM.APPLY)
    p.seek(pos)
    p.call(x, 5 * IM.TILE, IM.APPLY, u8=True, scale=40.0)
    p.bank.close()


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("pos", [0, 31, 1000, (1 << 40) + 5])
def test_apply_alone_at_any_position(host, ctx, pos, shared):
    """6000 samples with partial tiles at both ends, float and u8, rows of their own and one shared row; the next call goes on"""
    x = signal(shared)
    p = Pair(ctx, host, streams4(), prime=signal(shared, seed=8, bad=False))
    p.seek(pos)
    p.call(x, N_APPLY, IM.APPLY)
    p.call(x, 701, IM.APPLY, x_off=N_APPLY)                                  # from an even or odd position on
    p.seek(pos)
    p.call(x, N_APPLY, IM.APPLY, u8=True, scale=40.0)
    p.call(x, 3, IM.APPLY, u8=True, scale=40.0, x_off=N_APPLY)
    p.bank.close()


def test_in_place_both_flags_in_one_pass(host, ctx):
    """MEASURE | APPLY in place: the output is mapped with the coefficients as they stood before the call"""
    x = signal(False)
    p = Pair(ctx, host, streams4(), prime=signal(False, seed=8, bad=False))
    before = p.rec.copy()
    p.call(x, 5 * IM.TILE, IM.MEASURE | IM.APPLY, in_place=True)
    assert before["valid"][2] == 1 and before["b_re"][2] != p.rec["b_re"][2]      # (the call's output came from `before`: the model's order)
    p.call(x, 5 * IM.TILE, IM.MEASURE | IM.APPLY, x_off=5 * IM.TILE)
    p.call(x, 777, IM.APPLY, in_place=True)
    p.bank.close()


def test_measure_off_a_tile_edge_is_refused_and_writes_nothing(host, ctx):
    import dabgpu
    x = signal(False)
    p = Pair(ctx, host, streams4())
    p.seek(31)
    assert p.call(x, 2 * IM.TILE, IM.MEASURE | IM.APPLY) == 0                 # (asserts the guarded output untouched, the records equal)
    assert p.call(x, 2 * IM.TILE, IM.MEASURE) == 0
    assert list(p.rec["calls_refused"]) == [2, 2, 2, 2] and p.rec["N"][2] == 0
    assert p.call(x, 100, IM.APPLY) == 100                                   # the position did not move: still 31
    with pytest.raises(dabgpu.DabGpuError) as err:                           # the host form reports it
        p.bank.apply_host(x, IM.TILE, flags=IM.MEASURE, in_stride_samples=N_IN)
    assert "multiple of 1024" in str(err.value)
    p.rec["calls_refused"] += 1
    # refused on the host: n off a tile, more than the bank was created for, no flags, a u8 call in place
    import torch
    d = torch.from_numpy(x).cuda()
    for kw, text in ((dict(n=1000, flags=IM.MEASURE), "multiple of 1024"), (dict(n=11 * IM.TILE, flags=IM.MEASURE, in_stride_samples=0), "created for"),
                     (dict(n=IM.TILE, flags=0), "flags"), (dict(n=IM.TILE, flags=4), "flags"),
                     (dict(n=IM.TILE, flags=IM.APPLY, d_out=None), "null input / output"),
                     (dict(n=IM.TILE, flags=IM.APPLY, d_out=d, out_format=dabgpu.IQ_FORMATS.index("raw_u8")), "in place"),
                     (dict(n=0, flags=IM.APPLY), "n = 0")):
        a = dict(d_in=d, d_out=torch.zeros(4 * 11 * IM.TILE * 8, dtype=torch.uint8, device="cuda"), in_stride_samples=N_IN)
        a.update(kw)
        with pytest.raises(dabgpu.DabGpuError) as err:
            p.bank.apply(**a)
        assert text in str(err.value), (kw, str(err.value))
    state = p.bank.read_state()
    assert same_bits(state, p.rec)
    p.bank.close()


def test_one_call_of_ten_tiles_equals_four_then_six(host, ctx):
    x = signal(False)
    one, two = Pair(ctx, host, streams4()), Pair(ctx, host, streams4())
    one.call(x, 10 * IM.TILE, IM.MEASURE)
    two.call(x, 4 * IM.TILE, IM.MEASURE)
    two.call(x, 6 * IM.TILE, IM.MEASURE, x_off=4 * IM.TILE)
    assert same_bits(one.bank.read_state(), two.bank.read_state())
    assert one.rec["tiles_used"][2] == 8 and one.rec["tiles_skipped"][2] == 2
    one.bank.close(); two.bank.close()


def test_a_captured_both_flags_call_replayed_twice_continues_the_stream(host, ctx):
    import torch
    plist = streams4()
    p = Pair(ctx, host, plist)
    x = signal(False, bad=False)
    n = 3 * IM.TILE
    d_in = torch.from_numpy(x).cuda()
    stride = n * 8
    out = torch.zeros(4 * stride, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        p.bank.apply(d_in, n, out, flags=IM.MEASURE | IM.APPLY, in_stride_samples=N_IN, out_stride_bytes=stride, stream=side.cuda_stream)
    rec = IM.host_records(host, 4)
    for r in range(2):                                                       # (capturing enqueued nothing: the position is still 0)
        g.replay()
        torch.cuda.synchronize()
        want_y, _, adv = IM.host_apply(host, plist, rec, x, r * n, n, IM.MEASURE | IM.APPLY)
        assert adv == n
        assert same_bits(out.cpu().numpy().reshape(4, stride).view(np.complex64), want_y), f"replay {r}"
        assert same_bits(p.bank.read_state(), rec), f"records after replay {r}"
    assert rec["tiles_used"][2] == 6 and rec["valid"][2] == 1
    p.pos, p.rec = 2 * n, rec
    p.call(x, 500, IM.APPLY)                                                 # the position stands behind the two replays
    p.bank.close()


def test_host_form_reset_and_set_params(host, ctx):
    import dabgpu
    plist = streams4()
    p = Pair(ctx, host, plist)
    x = signal(False)
    assert p.bank.apply_host(x, 4 * IM.TILE, flags=IM.MEASURE, in_stride_samples=N_IN) is None
    IM.host_apply(host, plist, p.rec, x, 0, 4 * IM.TILE, IM.MEASURE)
    assert same_bits(p.bank.read_state(), p.rec)
    y = p.bank.apply_host(x, 3001, flags=IM.APPLY, in_stride_samples=N_IN)   # from position 4096 on, the input rows from their start
    want, _, _ = IM.host_apply(host, plist, p.rec, x, 4 * IM.TILE, 3001, IM.APPLY)
    assert same_but_nan(y, want)
    y8 = p.bank.apply_host(x[1], 1001, flags=IM.APPLY, out_format=dabgpu.IQ_FORMATS.index("raw_u8"), u8_scale=30.0)     # a shared row, odd position
    want8, _, _ = IM.host_apply(host, plist, p.rec, x[1], 4 * IM.TILE + 3001, 1001, IM.APPLY, u8=True, scale=30.0)
    assert same_bits(y8, want8)
    p.bank.seek(8 * IM.TILE)
    y = p.bank.apply_host(x, 2 * IM.TILE, flags=IM.MEASURE | IM.APPLY, in_stride_samples=N_IN)
    want, _, _ = IM.host_apply(host, plist, p.rec, x, 8 * IM.TILE, 2 * IM.TILE, IM.MEASURE | IM.APPLY)
    assert same_but_nan(y, want) and same_bits(p.bank.read_state(), p.rec)
    swapped = [plist[2], plist[3], plist[1], plist[0]]                       # new parameters, the records stay
    p.bank.set_params(g_streams(swapped))
    p.plist = swapped
    p.pos = 10 * IM.TILE
    p.call(x, 2 * IM.TILE, IM.MEASURE | IM.APPLY)
    p.bank.reset()
    p.rec = IM.host_records(host, 4)
    p.call(x, 2 * IM.TILE, IM.MEASURE | IM.APPLY)
    with pytest.raises(dabgpu.DabGpuError) as err:
        p.bank.set_params(g_streams([IM.params(forget=0.0)] * 4))
    assert "stream 0: forget" in str(err.value)
    with pytest.raises(dabgpu.DabGpuError) as err:
        p.bank.seek((1 << 62) + 1)
    assert "2^62" in str(err.value)
    p.bank.close()


def test_handle_closes_twice_and_goes_with_its_last_reference(ctx):
    import dabgpu
    SB.handle_lifecycle(lambda: dabgpu.IqBalance(ctx, g_streams(streams4()), MAX_CALL))
