"""-m gpu: receive diversity on the device (dabgpu_diversity_combine_frames, csrc/diversity.hip) against the compiled arithmetic header
(tests/cpp/diversity_host_model.cpp, which tests/test_diversity_model.py holds to the numpy model bit for bit): soft bits, the scale and
the live mask byte for byte -- for 1, 2, 3 and 8 branches, every run length, both layouts, into a ring slot, with branches dead by sync
record, by zero scale and by zero weight whose products are NaN, the all-dead frame, from a captured graph replayed after its inputs
changed in place, through the host-sync form; and one branch fed by the demodulator's own products and scale reproduces the
demodulator's weighted soft bits in both layouts."""
import numpy as np
import pytest

import diversity_model as DM
import softbit_cases as SC

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
    return DM.build_host_model(tmp_path_factory.mktemp("diversity_host_model"))


@pytest.fixture(scope="module")
def data():
    """eight branches x three frames of random products, per-frame scales that put the combined soft bits over the whole range, weights"""
    rng = np.random.default_rng(9600)
    dq = ((rng.standard_normal((8,) + SHAPE) + 1j * rng.standard_normal((8,) + SHAPE)) * np.exp(rng.uniform(-1, 1, (8, 3, 1, 1)))).astype(np.complex64)
    k = (40 * np.exp(rng.uniform(-1, 1, (8, 3)))).astype(F32)
    w = np.exp(rng.uniform(-2, 2, (8, 3))).astype(F32)
    w[3] = 1.0
    return dict(dq=dq, k=k, w=w)


def sync_records(valid):
    import dabgpu
    rec = np.zeros(len(valid), np.dtype(dabgpu.SYNC_STATE_DTYPE))
    rec["sync_valid"] = valid
    rec["fine_time_offset"] = 17
    return rec


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


class Branches:
    """K branches on the device: products [3][75][1536], scales [3], weights [3] or None, sync flags [3] or None, per branch"""

    def __init__(self, dq, k, w=None, valid=None):
        self.n = len(dq)
        self.h = dict(dq=[np.array(d) for d in dq], k=np.array(k, F32), w=[None if x is None else np.array(x, F32) for x in (w or [None] * self.n)],
                      valid=[None if x is None else np.array(x, np.int32) for x in (valid or [None] * self.n)])
        self.d_dq = [to_dev(d) for d in self.h["dq"]]
        self.d_k = [to_dev(x) for x in self.h["k"]]
        self.d_w = [None if x is None else to_dev(x) for x in self.h["w"]]
        self.d_sync = [None if x is None else to_dev(sync_records(x)) for x in self.h["valid"]]

    def table(self):
        return [(self.d_dq[b], self.d_k[b], self.d_w[b], self.d_sync[b]) for b in range(self.n)]

    def expected(self, host, layout):
        bits, ks, masks = [], [], []
        for f in range(N_FRAMES):
            w = [F32(1) if x is None else x[f] for x in self.h["w"]]
            v = [1 if x is None else x[f] for x in self.h["valid"]]
            b, k, m = DM.host_combine_frame(host, [d[f] for d in self.h["dq"]], self.h["k"][:, f], w, v, layout)
            bits.append(b); ks.append(k); masks.append(m)
        return np.stack(bits), np.array(ks, F32), np.array(masks, np.uint32)


def combine(ctx, br, layout=0, spb=0, out=None, stride=0, stream=None):
    import torch
    bits = out if out is not None else torch.full((N_FRAMES, NB), 55, dtype=torch.int8, device="cuda")
    scale = torch.full((N_FRAMES,), -1.0, dtype=torch.float32, device="cuda")
    mask = torch.full((N_FRAMES,), -1, dtype=torch.int32, device="cuda")
    ctx.diversity_combine(br.table(), N_FRAMES, bits, bits_frame_stride=stride, bits_layout=layout, symbols_per_block=spb, soft_scale=scale,
                          live_mask=mask, stream=stream)
    torch.cuda.synchronize()
    return bits.cpu().numpy(), scale.cpu().numpy(), mask.cpu().numpy().view(np.uint32)


def same(got, exp):
    return np.array_equal(got[0], exp[0]) and np.array_equal(got[1].view(np.uint32), exp[1].view(np.uint32)) and np.array_equal(got[2], exp[2])


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_device_equals_the_host_model_for_every_run_length(ctx, host, data, n, layout):
    # branches with an even number carry weights, the others none (branch 3's weights are all exactly 1)
    # (the scales grow with the number of branches, so that the combined one stays near 40 and the soft bits cover their range)
    br = Branches(data["dq"][:n], data["k"][:n] * F32(n), [data["w"][b] if b % 2 == 0 or b == 3 else None for b in range(n)])
    exp = br.expected(host, layout)
    assert (exp[1] > 0).all() and (exp[2] == (1 << n) - 1).all() and len(np.unique(exp[0])) > 200
    for spb in (1, 7, 25, 75, 0):
        assert same(combine(ctx, br, layout, spb), exp), spb
    if n == 2 and layout == 0:
        # the numpy model itself, one frame
        bits, k, m = DM.combine_frame([data["dq"][0][1], data["dq"][1][1]], data["k"][:2, 1] * F32(2), DM.host_mapper(host), [data["w"][0][1], 1.0])
        assert np.array_equal(bits, exp[0][1]) and k.view(np.uint32) == exp[1][1].view(np.uint32)


def test_ring_slot_stride_leaves_the_other_slots_alone(ctx, host, data):
    import torch
    br = Branches(data["dq"][:2], data["k"][:2])
    for layout in (0, 1):
        H, slot = 3, 1
        ring = torch.full((N_FRAMES, H, NB), 77, dtype=torch.int8, device="cuda")
        got = combine(ctx, br, layout, 7, out=ring[:, slot], stride=H * NB)
        ring = ring.cpu().numpy()
        assert same((ring[:, slot], got[1], got[2]), br.expected(host, layout))
        assert (ring[:, :slot] == 77).all() and (ring[:, slot + 1:] == 77).all()


def test_dead_branches_are_never_read(ctx, host, data):
    """frame f loses branch f: by its sync record, by a zero scale, by a zero weight -- and the dead branch's products are NaN.  Then the
    frames with one live branch (weight 3, and weight exactly 1: its own scale), and the all-dead frame: zeros, k = 0, mask 0."""
    nan = np.full((75, 1536), np.nan + 1j * np.nan, np.complex64)
    dq = data["dq"][:3].copy()
    k, w = data["k"][:3].copy(), data["w"][:3].copy()
    valid = np.ones((3, 3), np.int32)
    valid[0, 0] = 0; k[1, 1] = 0.0; w[2, 2] = 0.0
    for b in range(3):
        dq[b, b] = nan
    br = Branches(dq, k, list(w), list(valid))
    for layout in (0, 1):
        exp = br.expected(host, layout)
        assert exp[2].tolist() == [6, 5, 3] and (exp[1] > 0).all()
        got = combine(ctx, br, layout, 25)
        assert same(got, exp)
        assert len(np.unique(got[0][0])) > 200                          # no NaN got in: a NaN component would zero its soft bit
    dq = data["dq"][:3].copy()
    k, w = data["k"][:3].copy(), data["w"][:3].copy()
    valid = np.ones((3, 3), np.int32)
    k[0, 0] = 0.0; valid[1, 0] = 0; w[2, 0] = -1.0                       # frame 0: nobody
    k[0, 1] = np.inf; w[2, 1] = np.nan; w[1, 1] = 3.0                    # frame 1: branch 1 alone, weight 3
    valid[0, 2] = 0; valid[1, 2] = 0; w[2, 2] = 1.0                      # frame 2: branch 2 alone, weight exactly 1
    dq[:, 0] = nan; dq[0, 1] = nan; dq[2, 1] = nan; dq[0, 2] = nan; dq[1, 2] = nan
    br = Branches(dq, k, list(w), list(valid))
    for layout in (0, 1):
        exp = br.expected(host, layout)
        got = combine(ctx, br, layout, 0)
        assert same(got, exp)
        assert got[2].tolist() == [0, 2, 4] and got[1][0] == 0 and not got[0][0].any()
        assert got[1][2].view(np.uint32) == k[2, 2].view(np.uint32) and got[1][1] != k[1, 1]


def test_graph_capture_replayed_after_the_inputs_changed_in_place(ctx, host, data):
    import torch
    br = Branches(data["dq"][:2], data["k"][:2], [data["w"][0], None])
    bits = torch.zeros((N_FRAMES, NB), dtype=torch.int8, device="cuda")
    scale = torch.zeros((N_FRAMES,), dtype=torch.float32, device="cuda")
    mask = torch.zeros((N_FRAMES,), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctx.diversity_combine(br.table(), N_FRAMES, bits, bits_layout=1, symbols_per_block=25, soft_scale=scale, live_mask=mask)
    torch.cuda.synchronize()

    def replay_and_check():
        bits.fill_(9); scale.fill_(-3.0); mask.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert same((bits.cpu().numpy(), scale.cpu().numpy(), mask.cpu().numpy().view(np.uint32)), br.expected(host, 1))

    replay_and_check()
    # other scales (one of them dead now) and other products, written into the same buffers
    new_k = data["k"][4:6].copy(); new_k[1, 0] = 0.0
    for b in range(2):
        br.h["k"][b] = new_k[b]; br.h["dq"][b] = data["dq"][6 + b]
        br.d_k[b].copy_(to_dev(new_k[b])); br.d_dq[b].copy_(to_dev(data["dq"][6 + b]))
    torch.cuda.synchronize()
    replay_and_check()


def test_host_sync_form(ctx, host, data):
    for layout in (0, 1):
        dq = [data["dq"][0][2], None, data["dq"][2][2]]
        k, w, valid = [data["k"][0][2], 5.0, data["k"][2][2]], [1.0, 1.0, data["w"][2][2]], [1, 0, 1]
        bits, kk, mask = ctx.diversity_combine_host(dq, k, w, valid, layout)
        eb, ek, em = DM.host_combine_frame(host, dq, k, w, valid, layout)
        assert np.array_equal(bits, eb) and F32(kk).view(np.uint32) == ek.view(np.uint32) and mask == em == 5
    bits, kk, mask = ctx.diversity_combine_host([None], [0.0])
    assert not bits.any() and kk == 0 and mask == 0


def test_refusals(ctx, data):
    import dabgpu
    import torch
    br = Branches(data["dq"][:1], data["k"][:1])
    bits = torch.zeros((N_FRAMES, NB + 16), dtype=torch.int8, device="cuda")
    t = br.table()
    for kw, text in ((dict(branches=t * 9), "n_branches"), (dict(branches=[]), "n_branches"), (dict(bits_layout=2), "bits_layout"),
                     (dict(symbols_per_block=76), "symbols_per_block"), (dict(bits_frame_stride=NB - 16), "bits_frame_stride"),
                     (dict(bits=bits.view(-1)[8:]), "d_bits"), (dict(branches=[(t[0][0], None)]), "no products or no scales"),
                     (dict(branches=[(br.d_dq[0][8:], t[0][1])]), "16-byte")):
        args = dict(branches=t, n_frames=N_FRAMES, bits=bits)
        args.update(kw)
        with pytest.raises(dabgpu.DabGpuError, match=text):
            ctx.diversity_combine(**args)
    g = dabgpu.diversity_plan(t, 1024, bits)
    assert (g.symbols_per_block, g.runs_per_frame, g.grid, g.threads) == (25, 3, 3072, 256)
    assert dabgpu.DIVERSITY_MAX_BRANCHES == 8
    k, m = dabgpu.diversity_scale([0.5, 0.25], [1.0, 1.0], [1, 1])
    assert m == 3 and abs(k - 1 / 6) < 1e-7


def test_one_branch_fed_by_the_demodulator_reproduces_its_weighted_soft_bits(ctx, oracle, tmp_path_factory):
    """dabgpu_ofdm_demod_frames_soft (display views, natural layout) writes d_dqpsk, d_soft_scale and d_bits; the combiner over that one
    branch gives those d_bits bit for bit, and in class order the d_bits of a second demodulation in DABGPU_BITS_MSC_CLASSED"""
    import dabgpu
    import torch
    rx = SC.received(oracle, tmp_path_factory.mktemp("diversity_channel"))[0]
    frames = np.stack([SC.frame_at(rx, j) for j in range(N_FRAMES)])
    d_raw = torch.from_numpy(frames.view(np.float32).reshape(N_FRAMES, -1, 2)).cuda()
    fmt = dabgpu.IQ_FORMATS.index("raw_f32l")
    soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0)
    bits = torch.zeros((N_FRAMES, NB), dtype=torch.int8, device="cuda")
    classed = torch.zeros((N_FRAMES, NB), dtype=torch.int8, device="cuda")
    dq = torch.zeros((N_FRAMES, 75, 1536, 2), dtype=torch.float32, device="cuda")
    scale = torch.zeros((N_FRAMES,), dtype=torch.float32, device="cuda")
    ctx.ofdm_demod_frames_soft(d_raw, fmt, N_FRAMES, bits, soft, dqpsk=dq, soft_scale=scale)
    ctx.ofdm_demod_frames_soft(d_raw, fmt, N_FRAMES, classed, soft, bits_layout=dabgpu.BITS_MSC_CLASSED)
    out = torch.full((2, N_FRAMES, NB), 55, dtype=torch.int8, device="cuda")
    k = torch.zeros((2, N_FRAMES), dtype=torch.float32, device="cuda")
    for layout in (0, 1):
        ctx.diversity_combine([(dq, scale)], N_FRAMES, out[layout], bits_layout=layout, soft_scale=k[layout])
    torch.cuda.synchronize()
    out, bits, classed = out.cpu().numpy(), bits.cpu().numpy(), classed.cpu().numpy()
    assert (scale.cpu().numpy() > 0).all() and len(np.unique(bits)) > 100 and not np.array_equal(bits, classed)
    assert np.array_equal(out[0], bits) and np.array_equal(out[1], classed)
    assert np.array_equal(k.cpu().numpy().view(np.uint32), np.stack([scale.cpu().numpy()] * 2).view(np.uint32))
