"""-m gpu: the banded combiner on the device (dabgpu_diversity_combine_frames_banded, csrc/diversity.hip's second instantiation) against
the compiled arithmetic header (tests/cpp/noise_profile_host_model.cpp, which tests/test_noise_profile_model.py holds to the numpy model
bit for bit): soft bits, the scale and the live mask byte for byte -- for 1, 2 and 8 branches, run lengths 0, 1, 7 and 75, both
layouts, into a ring slot, band weights of 0, NaN and infinity, a branch with a table beside one with a scalar weight, dead branches
whose products are NaN, the host-sync form; a table of one value equals the scalar call with that weight, a table of ones on one branch
the single-branch call, and an array without any table the existing call."""
import numpy as np
import pytest

import diversity_model as DM
import noise_profile_model as M

pytestmark = pytest.mark.gpu
NB = DM.NB_FRAME_BITS
F32 = np.float32
N_FRAMES, SHAPE = 3, (3, 75, 1536)


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return M.build_host_model(tmp_path_factory.mktemp("noise_profile_host_model"))


@pytest.fixture(scope="module")
def data():
    """eight branches x three frames of random products, scales, scalar weights and band tables whose weights spread over two decades"""
    rng = np.random.default_rng(9700)
    dq = ((rng.standard_normal((8,) + SHAPE) + 1j * rng.standard_normal((8,) + SHAPE)) * np.exp(rng.uniform(-1, 1, (8, 3, 1, 1)))).astype(np.complex64)
    k = (40 * np.exp(rng.uniform(-1, 1, (8, 3)))).astype(F32)
    w = np.exp(rng.uniform(-2, 2, (8, 3))).astype(F32)
    band = np.exp(rng.uniform(-2.3, 2.3, (8, 3, 128))).astype(F32)
    for a in (dq, k, w, band):
        a.setflags(write=False)
    return dict(dq=dq, k=k, w=w, band=band)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def sync_records(valid):
    import dabgpu
    rec = np.zeros(len(valid), np.dtype(dabgpu.SYNC_STATE_DTYPE))
    rec["sync_valid"] = valid
    return rec


class Branches:
    """K branches on the device: products [3][75][1536], scales [3]; per branch a band table [3][128] or None, scalar weights [3] or None,
    sync flags [3] or None"""

    def __init__(self, dq, k, band=None, w=None, valid=None):
        self.n = len(dq)
        opt = lambda x, t: [None if v is None else np.array(v, t) for v in (x or [None] * self.n)]
        self.h = dict(dq=[np.array(d) for d in dq], k=np.array(k, F32), band=opt(band, F32), w=opt(w, F32), valid=opt(valid, np.int32))
        self.d_dq = [to_dev(d) for d in self.h["dq"]]
        self.d_k = [to_dev(x) for x in self.h["k"]]
        self.d_band = [None if x is None else to_dev(x) for x in self.h["band"]]
        self.d_w = [None if x is None else to_dev(x) for x in self.h["w"]]
        self.d_sync = [None if x is None else to_dev(sync_records(x)) for x in self.h["valid"]]

    def table(self):
        return [(self.d_dq[b], self.d_k[b], self.d_w[b], self.d_sync[b]) for b in range(self.n)]

    def expected(self, host, layout):
        bits, ks, masks = [], [], []
        for f in range(N_FRAMES):
            w = [F32(1) if x is None else x[f] for x in self.h["w"]]
            v = [1 if x is None else x[f] for x in self.h["valid"]]
            band = [None if x is None else x[f] for x in self.h["band"]]
            b, k, m = M.host_combine_frame(host, [d[f] for d in self.h["dq"]], self.h["k"][:, f], w, v, band, layout)
            bits.append(b); ks.append(k); masks.append(m)
        return np.stack(bits), np.array(ks, F32), np.array(masks, np.uint32)


def combine(ctx, br, layout=0, spb=0, out=None, stride=0, bands="own"):
    import torch
    bits = out if out is not None else torch.full((N_FRAMES, NB), 55, dtype=torch.int8, device="cuda")
    scale = torch.full((N_FRAMES,), -1.0, dtype=torch.float32, device="cuda")
    mask = torch.full((N_FRAMES,), -1, dtype=torch.int32, device="cuda")
    ctx.diversity_combine(br.table(), N_FRAMES, bits, bits_frame_stride=stride, bits_layout=layout, symbols_per_block=spb, soft_scale=scale,
                          live_mask=mask, band_weights=br.d_band if bands == "own" else bands)
    torch.cuda.synchronize()
    return bits.cpu().numpy(), scale.cpu().numpy(), mask.cpu().numpy().view(np.uint32)


def same(got, exp):
    return np.array_equal(got[0], exp[0]) and np.array_equal(got[1].view(np.uint32), exp[1].view(np.uint32)) and np.array_equal(got[2], exp[2])


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 8])
def test_device_equals_the_host_model_for_every_run_length(ctx, host, data, n, layout):
    # every other branch has a table, the ones between a scalar weight or none: a table beside a scalar weight from n = 2 on
    band = [data["band"][b] if b % 2 == 0 else None for b in range(n)]
    w = [data["w"][b] if b % 4 == 1 else None for b in range(n)]
    br = Branches(data["dq"][:n], data["k"][:n] * F32(n), band, w)
    exp = br.expected(host, layout)
    assert (exp[1] > 0).all() and (exp[2] == (1 << n) - 1).all() and len(np.unique(exp[0])) > 200
    for spb in (0, 1, 7, 75):
        assert same(combine(ctx, br, layout, spb), exp), spb
    if n == 2 and layout == 0:
        # the numpy model itself, one frame
        bits, k, m = M.combine_frame([data["dq"][0][1], data["dq"][1][1]], data["k"][:2, 1] * F32(2), DM.host_mapper(host), [1.0, data["w"][1][1]],
                                     None, [data["band"][0][1], None])
        assert np.array_equal(bits, exp[0][1]) and F32(k).view(np.uint32) == exp[1][1].view(np.uint32)
        # the tables matter: the scalar call on the same branches gives other bits
        assert not np.array_equal(combine(ctx, br, 0, 25, bands=None)[0], exp[0])


def test_ring_slot_stride_leaves_the_other_slots_alone(ctx, host, data):
    import torch
    br = Branches(data["dq"][:2], data["k"][:2], [data["band"][0], data["band"][1]])
    for layout in (0, 1):
        H, slot = 3, 1
        ring = torch.full((N_FRAMES, H, NB), 77, dtype=torch.int8, device="cuda")
        got = combine(ctx, br, layout, 7, out=ring[:, slot], stride=H * NB)
        ring = ring.cpu().numpy()
        assert same((ring[:, slot], got[1], got[2]), br.expected(host, layout))
        assert (ring[:, :slot] == 77).all() and (ring[:, slot + 1:] == 77).all()


def test_band_weights_that_are_not_weights(ctx, host, data):
    """bands of 0, NaN, infinity and a negative value count as 0 in the sum and in the branch's mean; a table of nothing but those is a
    dead branch, and a dead branch's products -- NaN here -- are never read"""
    nan = np.full((75, 1536), np.nan + 1j * np.nan, np.complex64)
    band = data["band"][:3].copy()
    band[0, :, 5], band[0, :, 64], band[0, :, 127], band[0, :, 90] = 0.0, np.nan, np.inf, -3.0
    band[1, 0] = 0.0                                   # frame 0: branch 1 dead by its table
    band[1, 1] = np.nan                                # frame 1: too
    band[2, 2] = np.inf                                # frame 2: branch 2 dead by its table
    dq = data["dq"][:3].copy()
    dq[1, 0] = nan; dq[1, 1] = nan; dq[2, 2] = nan
    valid = np.ones((3, 3), np.int32)
    valid[2, 0] = 0                                    # ... and frame 0: branch 2 by its record
    dq[2, 0] = nan
    k = data["k"][:3].copy()
    k[0, 2] = 0.0                                      # ... and frame 2: branch 0 by its scale
    dq[0, 2] = nan
    br = Branches(dq, k, list(band), None, list(valid))
    for layout in (0, 1):
        exp = br.expected(host, layout)
        assert exp[2].tolist() == [1, 5, 2] and (exp[1] > 0).all()
        got = combine(ctx, br, layout, 25)
        assert same(got, exp)
        assert all(len(np.unique(got[0][f])) > 200 for f in range(3))            # no NaN got in: a NaN component would zero its soft bit
    # the bands that count as 0 leave their carriers' soft bits at 0 when the branch is alone
    one = Branches(dq[:1, :], k[:1], [band[0]])
    got = combine(ctx, one, 0, 0)
    assert same(got, one.expected(host, 0))
    mapper = DM.host_mapper(host)
    zero_bits = np.isin(mapper // 12, [5, 64, 127, 90])
    sym = got[0][0].reshape(75, 2, 1536)
    assert not sym[:, :, zero_bits].any() and sym[:, :, ~zero_bits].any(axis=(0, 1)).mean() > 0.99
    # every branch dead: zeros, k = 0, mask 0
    none = Branches(dq[:2], k[:2], [np.zeros((3, 128), F32), np.full((3, 128), np.nan, F32)])
    got = combine(ctx, none, 1, 7)
    assert same(got, none.expected(host, 1)) and not got[0].any() and not got[1].any() and not got[2].any()


def test_uniform_table_equals_the_scalar_call(ctx, host, data):
    """one normal value w in all 128 bands: the branch weight is w exactly and the output that of the existing call with d_weight = w;
    a table of ones on one branch is that branch's own scale and bits (the demodulator's weighted soft bits, by the existing call's
    test); an array without any table is the existing call"""
    import torch
    w = data["w"][:2].copy()
    w[1, 0], w[1, 1] = 1.0, F32(1.17549435e-38) * F32(3e4)
    tables = [np.repeat(w[b][:, None], 128, axis=1) for b in range(2)]
    scalar = Branches(data["dq"][:2], data["k"][:2], None, [w[0], w[1]])
    banded = Branches(data["dq"][:2], data["k"][:2], tables)
    mixed = Branches(data["dq"][:2], data["k"][:2], [tables[0], None], [None, w[1]])
    for layout in (0, 1):
        ref = combine(ctx, scalar, layout, 25, bands=None)                       # dabgpu_diversity_combine_frames
        assert (ref[2] == 3).all() and len(np.unique(ref[0])) > 200
        assert same(combine(ctx, banded, layout, 25), ref)
        assert same(combine(ctx, mixed, layout, 7), ref)
        assert same(combine(ctx, scalar, layout, 25, bands=[None, None]), ref)      # all NULL: exactly the existing call
    ones = Branches(data["dq"][3:4], data["k"][3:4], [np.ones((3, 128), F32)])
    plain = Branches(data["dq"][3:4], data["k"][3:4])
    for layout in (0, 1):
        ref = combine(ctx, plain, layout, 0, bands=None)
        got = combine(ctx, ones, layout, 0)
        assert same(got, ref) and np.array_equal(got[1].view(np.uint32), data["k"][3].view(np.uint32))


def test_host_sync_form(ctx, host, data):
    for layout in (0, 1):
        dq = [data["dq"][0][2], None, data["dq"][2][2]]
        k, w, valid = [data["k"][0][2], 5.0, data["k"][2][2]], [7.0, 1.0, data["w"][2][2]], [1, 0, 1]
        band = [data["band"][0][2], data["band"][1][2], None]
        bits, kk, mask = ctx.diversity_combine_host(dq, k, w, valid, layout, band_weights=band)
        eb, ek, em = M.host_combine_frame(host, dq, k, w, valid, band, layout)
        assert np.array_equal(bits, eb) and F32(kk).view(np.uint32) == ek.view(np.uint32) and mask == em == 5
        plain = ctx.diversity_combine_host(dq, k, w, valid, layout)
        none = ctx.diversity_combine_host(dq, k, w, valid, layout, band_weights=[None] * 3)
        assert np.array_equal(none[0], plain[0]) and none[1:] == plain[1:] and not np.array_equal(plain[0], bits)
    bits, kk, mask = ctx.diversity_combine_host([None], [1.0], band_weights=[np.zeros(128, F32)])
    assert not bits.any() and kk == 0 and mask == 0


def test_refusals(ctx, data):
    import dabgpu
    import torch
    br = Branches(data["dq"][:2], data["k"][:2], [data["band"][0], None], [None, data["w"][1]])
    bits = torch.zeros((N_FRAMES, NB), dtype=torch.int8, device="cuda")
    t = br.table()
    both = [(t[0][0], t[0][1], br.d_w[1], None), t[1]]
    for kw, text in ((dict(branches=both), "both a band table and d_weight"), (dict(band_weights=[br.d_band[0][2:], None]), "4-byte"),
                     (dict(bits_layout=2), "bits_layout"), (dict(symbols_per_block=76), "symbols_per_block")):
        args = dict(branches=t, n_frames=N_FRAMES, bits=bits, band_weights=br.d_band)
        args.update(kw)
        with pytest.raises(dabgpu.DabGpuError, match=text):
            ctx.diversity_combine(**args)
    with pytest.raises(ValueError):
        ctx.diversity_combine(t, N_FRAMES, bits, band_weights=[br.d_band[0]])
    g = dabgpu.diversity_plan_banded(t, 1024, bits, br.d_band)
    assert (g.symbols_per_block, g.runs_per_frame, g.grid, g.threads, g.lds_bytes) == (25, 3, 3072, 256, 6144 + 64)
    assert dabgpu.diversity_plan_banded(t, 1024, bits, [None, None]).lds_bytes == 6144
