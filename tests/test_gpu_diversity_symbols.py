"""-m gpu: the symbol-weighted combiner on the device (dabgpu_diversity_combine_frames_symbols, csrc/diversity.hip's third instantiation)
against the compiled rule (tests/cpp/sym_profile_host_model.cpp, which tests/test_diversity_symbols_model.py holds to the numpy rule bit
for bit): soft bits, the scale and the live mask byte for byte -- for 1, 2 and 8 branches, run lengths 1, 5 and the default, both
layouts, 1, 3 and 67 frames, a dead branch whose products are NaN, symbol weights of 0, NaN and infinity, branches with a symbol table
beside branches with none and with band tables, written into a history ring's stride, a captured call, the host-sync form; a table of ones
equals the banded call byte for byte, and an array without any table is the banded call."""
import numpy as np
import pytest

import diversity_model as DM
import diversity_symbols_model as M

pytestmark = pytest.mark.gpu
NB = DM.NB_FRAME_BITS
F32 = np.float32
N_FRAMES = 3
N_MANY = 67


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return M.build_host_model(tmp_path_factory.mktemp("diversity_symbols_host_model"))


@pytest.fixture(scope="module")
def data():
    """eight branches x three frames of random products, scales, scalar weights, band tables over two decades and symbol tables in (0, 1]
    of which about half are exactly 1"""
    rng = np.random.default_rng(9800)
    shape = (8, N_FRAMES, 75, 1536)
    dq = ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.exp(rng.uniform(-1, 1, (8, N_FRAMES, 1, 1)))).astype(np.complex64)
    k = (40 * np.exp(rng.uniform(-1, 1, (8, N_FRAMES)))).astype(F32)
    w = np.exp(rng.uniform(-2, 2, (8, N_FRAMES))).astype(F32)
    band = np.exp(rng.uniform(-2.3, 2.3, (8, N_FRAMES, 128))).astype(F32)
    sym = np.minimum(1.0, np.exp(rng.uniform(-3.0, 3.0, (8, N_FRAMES, 75)))).astype(F32)
    for a in (dq, k, w, band, sym):
        a.setflags(write=False)
    return dict(dq=dq, k=k, w=w, band=band, sym=sym)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def sync_records(valid):
    import dabgpu
    rec = np.zeros(len(valid), np.dtype(dabgpu.SYNC_STATE_DTYPE))
    rec["sync_valid"] = valid
    return rec


class Branches:
    """K branches on the device: products [n][75][1536], scales [n]; per branch a band table [n][128] or None, a symbol table [n][75] or
    None, scalar weights [n] or None, sync flags [n] or None"""

    def __init__(self, dq, k, band=None, sym=None, w=None, valid=None):
        self.n = len(dq)
        self.frames = len(dq[0])
        opt = lambda x, t: [None if v is None else np.array(v, t) for v in (x or [None] * self.n)]
        self.h = dict(dq=[np.array(d) for d in dq], k=np.array(k, F32), band=opt(band, F32), sym=opt(sym, F32), w=opt(w, F32), valid=opt(valid, np.int32))
        self.d_dq = [to_dev(d) for d in self.h["dq"]]
        self.d_k = [to_dev(x) for x in self.h["k"]]
        self.d_band = [None if x is None else to_dev(x) for x in self.h["band"]]
        self.d_sym = [None if x is None else to_dev(x) for x in self.h["sym"]]
        self.d_w = [None if x is None else to_dev(x) for x in self.h["w"]]
        self.d_sync = [None if x is None else to_dev(sync_records(x)) for x in self.h["valid"]]

    def table(self):
        return [(self.d_dq[b], self.d_k[b], self.d_w[b], self.d_sync[b]) for b in range(self.n)]

    def expected(self, host, layout, sym="own"):
        bits, ks, masks = [], [], []
        for f in range(self.frames):
            w = [F32(1) if x is None else x[f] for x in self.h["w"]]
            v = [1 if x is None else x[f] for x in self.h["valid"]]
            band = [None if x is None else x[f] for x in self.h["band"]]
            s = [None if x is None else x[f] for x in self.h["sym"]] if sym == "own" else sym
            b, k, m = M.host_combine_frame(host, [d[f] for d in self.h["dq"]], self.h["k"][:, f], w, v, band, s, layout)
            bits.append(b); ks.append(k); masks.append(m)
        return np.stack(bits), np.array(ks, F32), np.array(masks, np.uint32)


def combine(ctx, br, layout=0, spb=0, out=None, stride=0, syms="own", bands="own", stream=None):
    import torch
    bits = out if out is not None else torch.full((br.frames, NB), 55, dtype=torch.int8, device="cuda")
    scale = torch.full((br.frames,), -1.0, dtype=torch.float32, device="cuda")
    mask = torch.full((br.frames,), -1, dtype=torch.int32, device="cuda")
    ctx.diversity_combine(br.table(), br.frames, bits, bits_frame_stride=stride, bits_layout=layout, symbols_per_block=spb, soft_scale=scale,
                          live_mask=mask, band_weights=br.d_band if bands == "own" else bands, symbol_weights=br.d_sym if syms == "own" else syms,
                          stream=stream)
    torch.cuda.synchronize()
    return bits.cpu().numpy(), scale.cpu().numpy(), mask.cpu().numpy().view(np.uint32)


def same(got, exp):
    return np.array_equal(got[0], exp[0]) and np.array_equal(got[1].view(np.uint32), exp[1].view(np.uint32)) and np.array_equal(got[2], exp[2])


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 8])
def test_device_equals_the_host_model_for_every_run_length(ctx, host, data, n, layout):
    # branch b: a band table where b is even, a scalar weight where b % 4 == 1, a symbol table unless b % 3 == 1 -- from n = 2 on a branch
    # with a symbol table stands beside one without, from n = 8 on every combination of the three occurs
    band = [data["band"][b] if b % 2 == 0 else None for b in range(n)]
    w = [data["w"][b] if b % 4 == 1 else None for b in range(n)]
    sym = [data["sym"][b] if b % 3 != 1 else None for b in range(n)]
    br = Branches(data["dq"][:n], data["k"][:n] * F32(n), band, sym, w)
    exp = br.expected(host, layout)
    assert (exp[1] > 0).all() and (exp[2] == (1 << n) - 1).all() and len(np.unique(exp[0])) > 200
    for spb in (0, 1, 5):
        assert same(combine(ctx, br, layout, spb), exp), spb
    # the symbol tables matter: the banded call on the same branches gives other bits, the same scale and the same mask
    banded = combine(ctx, br, layout, 0, syms=None)
    assert not np.array_equal(banded[0], exp[0]) and same((exp[0], banded[1], banded[2]), exp)
    if n == 2 and layout == 0:
        # the numpy rule itself, one frame
        bits, k, m = M.combine_frame([data["dq"][0][1], data["dq"][1][1]], data["k"][:2, 1] * F32(2), M.host_mapper(host), [1.0, data["w"][1][1]], None,
                                     [data["band"][0][1], None], [data["sym"][0][1], None])
        assert np.array_equal(bits, exp[0][1]) and F32(k).view(np.uint32) == exp[1][1].view(np.uint32)


@pytest.mark.parametrize("frames", [1, N_MANY])
def test_one_and_many_frames(ctx, host, frames):
    """one branch with a symbol table over 1 and 67 frames (more than one pass of any grid rule would take), class order, default runs"""
    rng = np.random.default_rng(9801 + frames)
    dq = ((rng.standard_normal((1, frames, 75, 1536)) + 1j * rng.standard_normal((1, frames, 75, 1536))) * 3.0).astype(np.complex64)
    k = (40 * np.exp(rng.uniform(-1, 1, (1, frames)))).astype(F32)
    sym = np.minimum(1.0, np.exp(rng.uniform(-3.0, 3.0, (1, frames, 75)))).astype(F32)
    br = Branches(dq, k, None, [sym[0]])
    exp = br.expected(host, 1)
    assert same(combine(ctx, br, 1, 0), exp) and np.array_equal(exp[1].view(np.uint32), k[0].view(np.uint32))       # one branch of weight 1 keeps its scale


def test_ring_slot_stride_leaves_the_other_slots_alone(ctx, host, data):
    import torch
    br = Branches(data["dq"][:2], data["k"][:2], [data["band"][0], None], [data["sym"][0], data["sym"][1]])
    for layout in (0, 1):
        H, slot = 3, 1
        ring = torch.full((N_FRAMES, H, NB), 77, dtype=torch.int8, device="cuda")
        got = combine(ctx, br, layout, 5, out=ring[:, slot], stride=H * NB)
        ring = ring.cpu().numpy()
        assert same((ring[:, slot], got[1], got[2]), br.expected(host, layout))
        assert (ring[:, :slot] == 77).all() and (ring[:, slot + 1:] == 77).all()


def test_dead_branches_and_weights_that_are_not_weights(ctx, host, data):
    """symbol weights of 0, NaN, infinity and a negative value count as 0 in the sum and nowhere else: scale and mask are the banded call's;
    a dead branch's products -- NaN here -- are never read, whatever its symbol table says"""
    nan = np.full((75, 1536), np.nan + 1j * np.nan, np.complex64)
    sym = data["sym"][:3].copy()
    sym[0, :, 5], sym[0, :, 64], sym[0, :, 74], sym[0, :, 30] = 0.0, np.nan, np.inf, -3.0
    dq = data["dq"][:3].copy()
    valid = np.ones((3, N_FRAMES), np.int32)
    valid[2, 0] = 0                                    # frame 0: branch 2 dead by its record
    dq[2, 0] = nan
    k = data["k"][:3].copy()
    k[0, 2] = 0.0                                      # frame 2: branch 0 dead by its scale
    dq[0, 2] = nan
    band = [None, data["band"][1].copy(), None]
    band[1][1] = 0.0                                   # frame 1: branch 1 dead by its band table
    dq[1, 1] = nan
    br = Branches(dq, k, band, list(sym), None, list(valid))
    for layout in (0, 1):
        exp = br.expected(host, layout)
        assert exp[2].tolist() == [3, 5, 6] and (exp[1] > 0).all()
        got = combine(ctx, br, layout, 5)
        assert same(got, exp)
        assert all(len(np.unique(got[0][f])) > 200 for f in range(3))            # no NaN got in: a NaN component would zero its soft bit
        banded = combine(ctx, br, layout, 5, syms=None)
        assert np.array_equal(banded[1].view(np.uint32), got[1].view(np.uint32)) and np.array_equal(banded[2], got[2])
    # the rows that count as 0 leave their soft bits at 0 when the branch is alone
    one = Branches(dq[:1, :2], k[:1, :2], None, [sym[0][:2]])
    got = combine(ctx, one, 0, 0)
    assert same(got, one.expected(host, 0))
    rows = got[0].reshape(2, 75, 3072)
    assert not rows[:, [5, 64, 74, 30]].any() and rows[:, np.delete(np.arange(75), [5, 64, 74, 30])].any(axis=2).all()
    # all rows 0 in every branch: zeros, but the frame is not erased -- k and the mask stay
    none = Branches(dq[:2, :1], k[:2, :1], None, [np.zeros((1, 75), F32), np.full((1, 75), np.nan, F32)])
    got = combine(ctx, none, 1, 0)
    assert same(got, none.expected(host, 1)) and not got[0].any() and got[1][0] > 0 and got[2][0] == 3


def test_ones_and_no_tables_are_the_banded_call(ctx, host, data):
    """a table of ones reproduces the banded call byte for byte, on every branch or on some; an array of NULLs and a NULL array are the
    banded call itself, which without band tables is the scalar call"""
    ones = np.ones((N_FRAMES, 75), F32)
    band = [data["band"][0], None, data["band"][2]]
    w = [None, data["w"][1], None]
    br = Branches(data["dq"][:3], data["k"][:3], band, [ones, ones, ones], w)
    part = Branches(data["dq"][:3], data["k"][:3], band, [None, ones, None], w)
    for layout in (0, 1):
        ref = combine(ctx, br, layout, 5, syms=None)                             # dabgpu_diversity_combine_frames_banded
        assert (ref[2] == 7).all() and len(np.unique(ref[0])) > 200
        assert same(combine(ctx, br, layout, 5), ref)
        assert same(combine(ctx, part, layout, 1), ref)
        assert same(combine(ctx, br, layout, 0, syms=[None, None, None]), ref)
    scalar = Branches(data["dq"][:2], data["k"][:2], None, [ones, ones], [data["w"][0], data["w"][1]])
    ref = combine(ctx, scalar, 0, 0, syms=None, bands=None)                       # dabgpu_diversity_combine_frames
    assert same(combine(ctx, scalar, 0, 0, bands=None), ref) and same(combine(ctx, scalar, 0, 0, syms=[None, None], bands=None), ref)
    single = Branches(data["dq"][3:4], data["k"][3:4], None, [ones])
    got = combine(ctx, single, 1, 0, bands=None)
    assert same(got, combine(ctx, single, 1, 0, syms=None, bands=None)) and np.array_equal(got[1].view(np.uint32), data["k"][3].view(np.uint32))


def test_captured_call(ctx, host, data):
    import torch
    br = Branches(data["dq"][:2], data["k"][:2], [data["band"][0], None], [None, data["sym"][1]])
    bits = torch.zeros((N_FRAMES, NB), dtype=torch.int8, device="cuda")
    scale = torch.zeros(N_FRAMES, dtype=torch.float32, device="cuda")
    mask = torch.zeros(N_FRAMES, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctx.diversity_combine(br.table(), N_FRAMES, bits, bits_layout=1, soft_scale=scale, live_mask=mask, band_weights=br.d_band,
                              symbol_weights=br.d_sym, stream=side.cuda_stream)
    exp = br.expected(host, 1)
    for _ in range(2):
        bits.fill_(33)
        g.replay()
        torch.cuda.synchronize()
        assert same((bits.cpu().numpy(), scale.cpu().numpy(), mask.cpu().numpy().view(np.uint32)), exp)
    # new weights in the same buffer: the replay reads them
    new = np.ascontiguousarray(data["sym"][2])
    br.d_sym[1].copy_(to_dev(new))
    br.h["sym"][1] = new
    g.replay()
    torch.cuda.synchronize()
    exp2 = br.expected(host, 1)
    assert same((bits.cpu().numpy(), scale.cpu().numpy(), mask.cpu().numpy().view(np.uint32)), exp2) and not np.array_equal(exp2[0], exp[0])


def test_host_sync_form(ctx, host, data):
    for layout in (0, 1):
        dq = [data["dq"][0][2], None, data["dq"][2][2]]
        k, w, valid = [data["k"][0][2], 5.0, data["k"][2][2]], [7.0, 1.0, data["w"][2][2]], [1, 0, 1]
        band = [data["band"][0][2], data["band"][1][2], None]
        sym = [data["sym"][0][2], None, data["sym"][2][2]]
        bits, kk, mask = ctx.diversity_combine_host(dq, k, w, valid, layout, band_weights=band, symbol_weights=sym)
        eb, ek, em = M.host_combine_frame(host, dq, k, w, valid, band, sym, layout)
        assert np.array_equal(bits, eb) and F32(kk).view(np.uint32) == ek.view(np.uint32) and mask == em == 5
        banded = ctx.diversity_combine_host(dq, k, w, valid, layout, band_weights=band)
        none = ctx.diversity_combine_host(dq, k, w, valid, layout, band_weights=band, symbol_weights=[None] * 3)
        assert np.array_equal(none[0], banded[0]) and none[1:] == banded[1:] and not np.array_equal(banded[0], bits) and banded[1:] == (kk, mask)
        only = ctx.diversity_combine_host(dq, k, w, valid, layout, symbol_weights=sym)                   # no band array at all
        eb, ek, em = M.host_combine_frame(host, dq, k, w, valid, None, sym, layout)
        assert np.array_equal(only[0], eb) and F32(only[1]).view(np.uint32) == ek.view(np.uint32) and only[2] == em


def test_refusals(ctx, data):
    import dabgpu
    import torch
    br = Branches(data["dq"][:2], data["k"][:2], [data["band"][0], None], [data["sym"][0], None], [None, data["w"][1]])
    bits = torch.zeros((N_FRAMES, NB), dtype=torch.int8, device="cuda")
    t = br.table()
    for kw, text in ((dict(symbol_weights=[br.d_sym[0][2:], None]), "symbol weights must be 4-byte"), (dict(band_weights=[br.d_band[0][2:], None]), "4-byte"),
                     (dict(bits_layout=2), "bits_layout"), (dict(symbols_per_block=76), "symbols_per_block")):
        args = dict(branches=t, n_frames=N_FRAMES, bits=bits, band_weights=br.d_band, symbol_weights=br.d_sym)
        args.update(kw)
        with pytest.raises(dabgpu.DabGpuError, match=text):
            ctx.diversity_combine(**args)
    with pytest.raises(ValueError):
        ctx.diversity_combine(t, N_FRAMES, bits, symbol_weights=[br.d_sym[0]])
    g = dabgpu.diversity_plan_symbols(t, 1024, bits, br.d_band, br.d_sym)
    assert (g.symbols_per_block, g.runs_per_frame, g.grid, g.threads, g.lds_bytes) == (25, 3, 3072, 256, 6144 + 64)
