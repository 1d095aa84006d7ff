"""-m gpu: the symbol noise profile on the device (include/dabgpu.h, "Symbol noise profile") against the float32 host model of
tests/sym_profile_model.py (csrc/sym_profile_core.h compiled by g++), bit for bit on every output: batch sizes 1, 3 and 67, products
aligned to 16 bytes and no more, a refused frame between valid ones whose stale products are NaN, an all-zero frame, NaN and infinity
rows, a frame with 38 bad rows, every subset of outputs between guard bands, a captured call replayed twice, the host form."""
import itertools

import numpy as np
import pytest

import sym_profile_model as M

pytestmark = pytest.mark.gpu

F32 = np.float32
N = 67                            # more frames than one pass of any grid rule would take, a multiple of nothing
GUARD = 1024                      # floats: 4 KB on either side of every output
NAMES = ("symbol_weight", "symbol_noise", "ref_noise", "valid")
SIZE = dict(symbol_weight=75, symbol_noise=75, ref_noise=1, valid=1)
REFUSED = (1, 40)                 # frames whose record has sync_valid = 0: their products are NaN throughout
ZERO = 5                          # an all-zero frame
HALF_BAD = 6                      # 38 rows with a NaN: the reference is infinite, the frame is skipped


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return M.build_host_model(tmp_path_factory.mktemp("sym_profile_host_model"))


@pytest.fixture(scope="module")
def frames():
    """67 frames of products: unit steps at an amplitude per carrier and frame under noise, with a burst of k % 7 symbols at a place and a
    power that move from frame to frame; records with two refused frames (stale products: NaN), an all-zero frame, NaN and infinity in
    single products of frames 2 and 3, 38 bad rows in frame 6.  Shared and read only."""
    import dabgpu
    rng = np.random.default_rng(9500)
    d = np.zeros((N, 75, 1536), np.complex64)
    c = np.arange(1536)
    for k in range(N):
        amp = (2.0e5 * (1 + k % 5) * (1.0 + 0.5 * np.cos(2 * np.pi * c / 311.0 + k))).astype(F32)
        sigma = np.full(76, np.sqrt(amp.mean()) * 0.15)
        s0 = (k * 11) % 70
        sigma[s0:s0 + k % 7] *= 1.0 + (k % 4) * 3.0
        phase = np.cumsum(rng.integers(0, 4, (76, 1536)) * 0.5 + 0.25, axis=0) * np.pi
        X = np.sqrt(amp)[None, :] * np.exp(1j * phase) + sigma[:, None] * (rng.standard_normal((76, 1536)) + 1j * rng.standard_normal((76, 1536)))
        d[k] = (X[:-1] * np.conj(X[1:])).astype(np.complex64)
    st = np.zeros(N, np.dtype(dabgpu.SYNC_STATE_DTYPE))
    st["sync_valid"] = 1
    for k in REFUSED:
        st["sync_valid"][k] = 0
        d[k] = complex(np.nan, np.nan)
    d[ZERO] = 0
    d[2, 10, 100] = complex(np.nan, 1.0)
    d[2, 74, 1535] = complex(0.0, np.nan)
    d[3, 20, 200] = complex(np.inf, 0.0)
    d[3, 0, 0] = complex(1.0, -np.inf)
    d[3, 33, 767] = complex(3.0e38, 3.0e38)
    d[HALF_BAD, 20:58, 5] = np.nan
    d[7, 20:57, 5] = np.nan                                                              # 37 bad rows: still valid
    for a in (d, st):
        a.setflags(write=False)
    return d, st


@pytest.fixture(scope="module")
def device_frames(frames):
    """the products on the device once, 16 bytes behind an allocation's start: aligned to 16 bytes and to no more"""
    import torch
    d = frames[0]
    buf = torch.zeros(d.size * 2 + 4, dtype=torch.float32, device="cuda")
    view = buf[4:]
    view.copy_(torch.from_numpy(d.view(F32).reshape(-1).copy()))
    assert view.data_ptr() % 32 == 16
    return view


def expected(host, d, st=None):
    """the host model's outputs of the frames d: dict of arrays as the device writes them"""
    n = d.shape[0]
    out = {k: np.zeros((n, SIZE[k]), np.uint32 if k == "valid" else F32) for k in NAMES}
    for k in range(n):
        ok = st is None or bool(st["sync_valid"][k])
        r = M.host_frame(host, d[k] if ok else None, ok)
        for name in NAMES:
            out[name][k] = r[name]
    return out


def run(ctx, d_dq, n, want, st=None, names=NAMES, stream=None):
    """one call over the first n frames of d_dq with the outputs `names` between guard bands; asserts them equal to `want` as bit patterns,
    the bands untouched"""
    import torch
    d_st = None if st is None else torch.from_numpy(np.array(st[:n]).view(np.uint8)).cuda()
    bufs, kw = {}, {}
    for name in names:
        size = n * SIZE[name]
        bufs[name] = torch.full((GUARD + size + GUARD,), -286331154, dtype=torch.int32, device="cuda")          # 0xEEEEEEEE
        kw[name] = bufs[name][GUARD:GUARD + size]
    ctx.sym_profile(d_dq, n, sync=d_st, stream=stream, **kw)
    torch.cuda.synchronize()
    seen = {}
    for name in names:
        b = bufs[name].cpu().numpy().view(np.uint32)
        assert (b[:GUARD] == 0xEEEEEEEE).all() and (b[-GUARD:] == 0xEEEEEEEE).all(), f"{name}: guard band written"
        got, exp = b[GUARD:-GUARD], want[name][:n].reshape(-1).view(np.uint32)
        assert np.array_equal(got, exp), (name, names, np.nonzero(got != exp)[0][:8], got.view(F32)[:4], want[name].reshape(-1)[:4])
        seen[name] = got
    return seen


@pytest.fixture(scope="module")
def want(host, frames):
    d, st = frames
    w = expected(host, d, st)
    for a in w.values():
        a.setflags(write=False)
    return w


def test_equals_host_model(ctx, host, frames, device_frames, want):
    d, st = frames
    valid = want["valid"][:, 0] == 1
    assert valid.sum() == N - len(REFUSED) - 2 and ((want["symbol_weight"][valid] == 1).sum(axis=1) >= 38).all()
    # NaN behind the refused records, and nothing of it arrives: zeros.  That the products are not even read is established by reading
    # sym_profile.hip, where the return for a refused record stands in front of the first load.
    for k in REFUSED + (ZERO, HALF_BAD):
        assert not want["symbol_weight"][k].any() and not want["symbol_noise"][k].any() and want["ref_noise"][k] == 0 and want["valid"][k] == 0
    assert not want["symbol_weight"][2, [10, 74]].any() and np.isinf(want["symbol_noise"][2, [10, 74]]).all() and want["symbol_weight"][2, 11] > 0
    assert not want["symbol_weight"][3, [0, 20, 33]].any() and want["valid"][7] == 1 and not want["symbol_weight"][7, 20:57].any()
    for k in (0, 2):                                                                     # the neighbours of the refused frame: untouched by it
        alone = expected(host, d[k:k + 1])
        assert np.array_equal(alone["symbol_weight"][0].view(np.uint32), want["symbol_weight"][k].view(np.uint32))
    # a frame with a burst: its rows are weighed down, the rest is not
    k = 17                                                                               # burst of 3 symbols from symbol 47, ten times the noise power
    assert (want["symbol_weight"][k, 47:49] < 0.2).all() and (np.delete(want["symbol_weight"][k], np.arange(46, 50)) > 0.5).all()
    for n in (1, 3, N):
        seen = run(ctx, device_frames, n, want, st)
    print(f"device weights of frame 17 {seen['symbol_weight'].view(F32)[17 * 75 + 45:17 * 75 + 51]}, reference noise {seen['ref_noise'].view(F32)[:3]}, "
          f"{int(seen['valid'].sum())} of {N} frames valid")


def test_aligned_products_and_no_records(ctx, host, frames):
    """an allocation's own start (aligned to 256 bytes and more), no records: frames 3 .. 6, the last two skipped by their own figures"""
    import torch
    d, st = frames
    d_dq = torch.from_numpy(d[3:7].view(F32).copy()).cuda()
    exp = expected(host, d[3:7])
    assert exp["valid"][:, 0].tolist() == [1, 1, 0, 0] and not exp["symbol_weight"][2:].any()
    run(ctx, d_dq, 4, exp)


def test_every_subset_of_outputs(ctx, frames, device_frames, want):
    import dabgpu
    d, st = frames
    for r in range(1, len(NAMES) + 1):
        for names in itertools.combinations(NAMES, r):
            run(ctx, device_frames, 3, want, st, names=names)
    with pytest.raises(dabgpu.DabGpuError, match="no output"):
        ctx.sym_profile(device_frames, 1)
    import torch
    d_v = torch.zeros(75, device="cuda")
    with pytest.raises(dabgpu.DabGpuError, match="16-byte"):
        ctx.sym_profile(device_frames[2:], 1, symbol_weight=d_v)
    with pytest.raises(dabgpu.DabGpuError, match="n_frames"):
        ctx.sym_profile(device_frames, 0, symbol_weight=d_v)


def test_captured_call_replayed_twice(ctx, host, frames, device_frames):
    """three receivers, one captured call, two replays on new products: the call keeps no state"""
    import torch
    d, st = frames
    per_frame = 75 * 1536 * 2
    d_dq = torch.zeros(3 * per_frame, dtype=torch.float32, device="cuda")
    d_v = torch.zeros((3, 75), dtype=torch.float32, device="cuda")
    d_q = torch.zeros((3, 75), dtype=torch.float32, device="cuda")
    d_r = torch.zeros(3, dtype=torch.float32, device="cuda")
    d_ok = torch.zeros(3, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctx.sym_profile(d_dq, 3, symbol_weight=d_v, symbol_noise=d_q, ref_noise=d_r, valid=d_ok, stream=side.cuda_stream)
    for lo in (8, 16):
        d_dq.copy_(device_frames[lo * per_frame:(lo + 3) * per_frame])
        g.replay()
        torch.cuda.synchronize()
        exp = expected(host, d[lo:lo + 3])
        assert exp["valid"].all() and d_ok.cpu().numpy().tolist() == [1, 1, 1]
        assert np.array_equal(d_v.cpu().numpy().view(np.uint32), exp["symbol_weight"].view(np.uint32)), lo
        assert np.array_equal(d_q.cpu().numpy().view(np.uint32), exp["symbol_noise"].view(np.uint32)), lo
        assert np.array_equal(d_r.cpu().numpy().view(np.uint32), exp["ref_noise"].reshape(-1).view(np.uint32)), lo


def test_host_form(ctx, host, frames):
    import dabgpu
    d, st = frames
    for k in (0, 2, 3, 7, 17):
        v, q, ref, ok = ctx.sym_profile_host(d[k])
        r = M.host_frame(host, d[k])
        assert ok == 1 and np.array_equal(v.view(np.uint32), r["symbol_weight"].view(np.uint32)) and F32(ref).view(np.uint32) == r["ref_noise"].view(np.uint32)
        assert np.array_equal(q.view(np.uint32), r["symbol_noise"].view(np.uint32))
        hv, hq, href, hok = dabgpu.sym_profile_rows_host(d[k])                           # the host form of the ABI is the same definition
        assert hok == 1 and np.array_equal(hv.view(np.uint32), v.view(np.uint32)) and np.array_equal(hq.view(np.uint32), q.view(np.uint32))
        assert F32(href).view(np.uint32) == F32(ref).view(np.uint32)
    for k in (ZERO, HALF_BAD):
        v, q, ref, ok = ctx.sym_profile_host(d[k])
        assert ok == 0 and not v.any() and not q.any() and ref == 0
