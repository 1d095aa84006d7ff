"""-m gpu: the impulse blanker on the device (dabgpu_blanker_bank_*, dab-radio_amd/csrc/blanker.hip) against the host model -- the same
blanker_core.h under g++ (tests/cpp/blanker_host_model.cpp) -- bit for bit, samples and mask words; the host model is tied to the
independent numpy model by tests/test_blanker_model.py.  The shape -- four streams (three sets of parameters, one disabled), 6000 output
samples = six or seven tiles with partial ones at both ends -- is the smallest at which halo, tile-edge and partial-word handling can go
wrong."""
import numpy as np
import pytest

import blanker_model as BM
import signal_bank_cases as SB

pytestmark = pytest.mark.gpu

N_OUT = 6000
N_IN = 7200
POSITIONS = (0, 31, 1000, (1 << 40) + 5)
GUARD = 0xA5
GUARD_WORD = 0xA5A5A5A5
same_bits = SB.same_bits


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return BM.build_host_model(tmp_path_factory.mktemp("blanker_host_model"))


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


def streams4(base=0):
    """the defaults behind a negative start; the widest reach (gap 32, window 32, guard 4) behind a positive start; a window of one block
    with no gap and no guard; a disabled stream.  base: added to every start (the input is read at m - start)"""
    return [BM.params(start=base - 37), BM.params(start=base + 20, gap=32, window=32, guard=4, threshold=2.5),
            BM.params(start=base, gap=0, window=1, guard=0, threshold=8.0), BM.params(start=base + 5, enabled=0)]


def g_streams(plist):
    import dabgpu
    return [BM.to_struct(P, dabgpu.BlankerStream) for P in plist]


def noise(rng, shape, sigma=1.0):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * (sigma / np.sqrt(2.0))).astype(np.complex64)


def planted(pos, plist, shared, seed=11):
    """noise with bursts 20 dB above it where they hurt: in the call's first and last block, across a tile edge inside the call, just before
    the call (a halo block), and samples that are not finite.  Strided: every row carries them at its own stream's indices"""
    rng = np.random.default_rng(seed)
    x = noise(rng, (1 if shared else len(plist), N_IN))
    edge = ((pos + 2048) >> 10) << 10
    for row, P in zip(x, plist[:len(x)]):
        for m0, m1 in ((pos, pos + 20), (pos + N_OUT - 20, pos + N_OUT + 10), (edge - 30, edge + 30), (pos - 40, pos - 8), (pos + 4000, pos + 4200)):
            i0, i1 = max(m0 - P["start"], 0), min(m1 - P["start"], N_IN)
            if i1 > i0:
                row[i0:i1] += noise(rng, i1 - i0, 10.0)
        for m, bad in ((pos + 3000, np.nan), (pos + 3500, np.inf), (pos + 5100, -np.inf)):
            if 0 <= m - P["start"] < N_IN:
                row[m - P["start"]] = bad
    return x[0] if shared else x


def run_device(bank, x, n_out, mask=True, n_in=None):
    """one apply into guarded rows -> ([n][n_out] complex64, [n][words] uint32 or None, guards intact).  x: [n][n_in] complex64 with an even
    row length, or [n_in] for a shared row"""
    import dabgpu
    import torch
    n_in = x.shape[-1] if n_in is None else n_in
    stride = ((n_out * 8 + 15) & ~15) + 32                                   # guard bytes between the rows
    whole = torch.full((48 + bank.n * stride + 48,), GUARD, dtype=torch.uint8, device="cuda")
    view = whole[48:48 + bank.n * stride]
    words = dabgpu.blanker_mask_words(n_out)
    mstride = words + 3
    d_mask = torch.full((4 * (4 + bank.n * mstride),), GUARD, dtype=torch.uint8, device="cuda") if mask else None
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    bank.apply(d_in, n_in, n_out, view, in_stride_samples=0 if x.ndim == 1 else x.shape[-1], out_stride_bytes=stride,
               d_mask=d_mask[16:] if mask else None, mask_stride_words=mstride if mask else 0)
    torch.cuda.synchronize()
    h = whole.cpu().numpy()
    rows = h[48:48 + bank.n * stride].reshape(bank.n, stride)
    ok = bool(np.all(h[:48] == GUARD) and np.all(h[-48:] == GUARD) and np.all(rows[:, n_out * 8:] == GUARD))
    m = None
    if mask:
        hm = d_mask.cpu().numpy().view(np.uint32)
        mrows = hm[4:].reshape(bank.n, mstride)
        ok = ok and bool(np.all(hm[:4] == GUARD_WORD) and np.all(mrows[:, words:] == GUARD_WORD))
        m = np.ascontiguousarray(mrows[:, :words])
    return np.ascontiguousarray(rows[:, :n_out * 8]).view(np.complex64), m, ok


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("pos", POSITIONS)
def test_device_equals_the_host_model(host, ctx, pos, shared):
    """bursts in the first and last block of the call, across a tile edge and in the halo, NaN and infinities; positions inside a block, inside
    a tile and in the high word; rows of their own and one shared row"""
    import dabgpu
    plist = streams4(pos & ~1023 if pos > (1 << 30) else 0)
    bank = dabgpu.Blanker(ctx, g_streams(plist))
    assert bank.plan == {"reach_blocks": 68, "block_samples": 1024, "lds_bytes": (32 + 136) * 4 + 40 * 4}
    x = planted(pos, plist, shared)
    bank.seek(pos)
    y, m, ok = run_device(bank, x, N_OUT)
    assert ok, "guard bytes or words before, between or after the rows were written"
    want_y, want_m = BM.host_apply(host, plist, x, pos, N_OUT)
    assert same_bits(m, want_m), f"mask words at position {pos}"
    assert same_bits(y, want_y), f"samples at position {pos}"
    assert BM.popcount(m[0]) >= 6 and BM.popcount(m[3]) == 0
    if not shared:
        i = np.arange(pos, pos + N_OUT) - plist[3]["start"]
        assert same_bits(y[3][i >= 0], x[3][i[i >= 0]])                    # the disabled stream copies
    # the following call goes on where this one ended (the position advanced on the device), without a mask
    y2, _, ok = run_device(bank, x, 700, mask=False)
    assert ok and same_bits(y2, BM.host_apply(host, plist, x, pos + N_OUT, 700)[0])
    bank.close()


def test_all_zeros_and_short_calls(host, ctx):
    import dabgpu
    plist = streams4()
    bank = dabgpu.Blanker(ctx, g_streams(plist))
    z = np.zeros(N_IN, np.complex64)
    y, m, ok = run_device(bank, z, N_OUT)
    assert ok and not m.any() and np.all(y.view(np.uint32) == 0)
    x = planted(0, plist, False)
    pos = N_OUT
    for n_out in (1, 2, 31, 33, 1023):                                       # odd and even positions, less than a block, less than a tile
        y, m, ok = run_device(bank, x, n_out)
        want_y, want_m = BM.host_apply(host, plist, x, pos, n_out)
        assert ok and same_bits(y, want_y) and same_bits(m, want_m), f"{n_out} samples at {pos}"
        pos += n_out
    # an input shorter than the call: zeros behind it
    bank.seek(0)
    y, m, ok = run_device(bank, x, N_OUT, n_in=3001)
    want_y, want_m = BM.host_apply(host, plist, x, 0, N_OUT, n_in=3001)
    assert ok and same_bits(y, want_y) and same_bits(m, want_m)
    bank.close()


@pytest.mark.parametrize("at", [1, 33, 1025])
def test_split_calls_equal_one_call(host, ctx, at):
    import dabgpu
    plist = streams4()
    pos = 31
    x = planted(pos, plist, False)
    one, split = dabgpu.Blanker(ctx, g_streams(plist)), dabgpu.Blanker(ctx, g_streams(plist))
    one.seek(pos); split.seek(pos)
    y, m, ok = run_device(one, x, N_OUT)
    assert ok
    ya, ma, ok_a = run_device(split, x, at)
    yb, mb, ok_b = run_device(split, x, N_OUT - at)
    assert ok_a and ok_b and same_bits(np.concatenate([ya, yb], axis=1), y)
    whole = np.zeros((4, m.shape[1] + 2), np.uint32)
    whole[:, :ma.shape[1]] |= ma
    off = ((pos + at) >> 10) - (pos >> 10)
    whole[:, off:off + mb.shape[1]] |= mb
    assert same_bits(whole[:, :m.shape[1]], m) and not whole[:, m.shape[1]:].any()
    one.close(); split.close()


def test_graph_replays_continue_the_stream_and_set_params_retunes(host, ctx):
    """a captured call replayed three times equals one long host-model run over the same input; _set_params between replays retunes"""
    import dabgpu
    import torch
    plist = streams4()
    bank = dabgpu.Blanker(ctx, g_streams(plist))
    x = planted(0, plist, False)
    n = 1777
    words = dabgpu.blanker_mask_words(n)
    d_in = torch.from_numpy(x).cuda()
    stride = (n * 8 + 15) & ~15
    out = torch.zeros(4 * stride, dtype=torch.uint8, device="cuda")
    d_mask = torch.zeros(4 * words, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        bank.apply(d_in, N_IN, n, out, in_stride_samples=N_IN, out_stride_bytes=stride, d_mask=d_mask, stream=side.cuda_stream)

    def result():
        torch.cuda.synchronize()
        return (out.cpu().numpy().reshape(4, stride)[:, :n * 8].copy().view(np.complex64), d_mask.cpu().numpy().view(np.uint32).reshape(4, words))

    for r in range(3):                                                       # (capturing enqueued nothing: the position is still 0)
        g.replay()
        y, m = result()
        want_y, want_m = BM.host_apply(host, plist, x, r * n, n)
        assert same_bits(y, want_y) and same_bits(m, want_m), f"replay {r}"
    retuned = [plist[2], plist[3], plist[0], plist[0]]
    with torch.cuda.stream(side):                                            # enqueued on the stream the call was captured on, behind the replays
        bank.set_params(g_streams(retuned), stream=side.cuda_stream)
        g.replay()
    y, m = result()
    want_y, want_m = BM.host_apply(host, retuned, x, 3 * n, n)
    assert same_bits(y, want_y) and same_bits(m, want_m), "replay after set_params"
    bank.close()


def test_host_form_seek_and_every_refusal(host, ctx):
    import dabgpu
    import torch
    plist = streams4()
    bank = dabgpu.Blanker(ctx, g_streams(plist))
    x = planted(0, plist, False)
    y, m = bank.apply_host(x, 1029, in_stride_samples=N_IN, mask=True)
    want_y, want_m = BM.host_apply(host, plist, x, 0, 1029)
    assert same_bits(y, want_y) and same_bits(m, want_m)
    y = bank.apply_host(x[1], N_OUT)                                         # a shared row, larger buffers, no mask
    assert same_bits(y, BM.host_apply(host, plist, x[1], 1029, N_OUT)[0])
    big = [dict(P, start=P["start"] + (1 << 62) - 3000) for P in plist]
    bank.set_params(g_streams(big))
    bank.seek((1 << 62) - 3000)
    y, m = bank.apply_host(x, 3000, in_stride_samples=N_IN, mask=True)
    want_y, want_m = BM.host_apply(host, big, x, (1 << 62) - 3000, 3000)
    assert same_bits(y, want_y) and same_bits(m, want_m)
    bank.set_params(g_streams(plist))
    bank.seek(5)
    # refused before any device call: the position does not move, the output and the mask keep their bytes
    n = 1029
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.full((4 * 1040 * 8,), GUARD, dtype=torch.uint8, device="cuda")
    d_mask = torch.full((4 * 4 * 4,), GUARD, dtype=torch.uint8, device="cuda")
    bad = [
        (dict(n_in=0), "n_in"),
        (dict(n_out=(1 << 31) + 1), "n_out"),
        (dict(in_stride_samples=N_IN - 2), "in_stride_samples"),
        (dict(in_stride_samples=N_IN + 1), "in_stride_samples"),             # odd
        (dict(out_stride_bytes=n * 8 - 8), "out_stride_bytes"),
        (dict(out_stride_bytes=1040 * 8 + 8), "out_stride_bytes"),
        (dict(d_out=d_out[8:]), "16-byte aligned"),
        (dict(d_in=d_in.view(torch.uint8).reshape(-1)[8:]), "16-byte aligned"),
        (dict(d_out=None), "null input / output"),
        (dict(d_in=None), "null input / output"),
        (dict(d_in=d_out, n_in=1040, in_stride_samples=1040), "in place"),
        (dict(mask_stride_words=2), "mask_stride_words"),
        (dict(d_mask=d_mask[2:]), "4-byte aligned"),
    ]
    for change, text in bad:
        a = dict(d_in=d_in, n_in=N_IN, n_out=n, d_out=d_out, in_stride_samples=N_IN, out_stride_bytes=1040 * 8, d_mask=d_mask, mask_stride_words=4)
        a.update(change)
        with pytest.raises(dabgpu.DabGpuError) as err:
            bank.apply(**a)
        assert text in str(err.value), (change, str(err.value))
    with pytest.raises(dabgpu.DabGpuError) as err:
        bank.seek((1 << 62) + 1)
    assert "2^62" in str(err.value)
    with pytest.raises(dabgpu.DabGpuError) as err:
        dabgpu.Blanker(ctx, g_streams([BM.params(window=33)]))
    assert "stream 0: window 33" in str(err.value)
    narrow = dabgpu.Blanker(ctx, g_streams([BM.params()]))
    with pytest.raises(dabgpu.DabGpuError) as err:
        narrow.set_params(g_streams([BM.params(gap=9)]))
    assert "reaches 26 blocks, the bank was created for 25" in str(err.value)
    narrow.set_params(g_streams([BM.params(gap=2, window=20, guard=3)]))
    narrow.close()
    torch.cuda.synchronize()
    assert bool((d_out == GUARD).all()) and bool((d_mask == GUARD).all())
    y, m, ok = run_device(bank, x, 100)
    want_y, want_m = BM.host_apply(host, plist, x, 5, 100)
    assert ok and same_bits(y, want_y) and same_bits(m, want_m)
    bank.close()


def test_handle_closes_twice_and_goes_with_its_last_reference(ctx):
    import dabgpu
    SB.handle_lifecycle(lambda: dabgpu.Blanker(ctx, g_streams(streams4())))
