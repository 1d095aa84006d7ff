"""-m gpu: the decision-directed noise profile on the device (include/dabgpu.h, "Decision-directed noise profile") against the float32 host
model of tests/dd_profile_model.py (csrc/dd_profile_core.h and noise_profile_core.h compiled by g++), bit for bit on every output: batch
sizes 1, 3 and 67, products aligned to 16 bytes and no more, a refused frame between valid ones whose stale products are NaN, an
all-zero frame, NaN and infinity in single products, the exclusion table with one band fully excluded, both alphas in place over three
calls, every subset of outputs between guard bands, a captured call replayed with the state carried, the host form."""
import itertools

import numpy as np
import pytest

import dd_profile_model as M
import noise_profile_model as PM

pytestmark = pytest.mark.gpu

F32 = np.float32
N = 67                            # more frames than one pass of any grid rule would take, a multiple of nothing
GUARD = 1024                      # floats: 4 KB on either side of every output
NAMES = ("profile_out", "band_weight", "mean_noise", "carrier_noise", "carrier_amplitude", "valid")
SIZE = dict(profile_out=128, band_weight=128, mean_noise=1, carrier_noise=1536, carrier_amplitude=1536, valid=1)
REFUSED = (1, 40)                 # frames whose record has sync_valid = 0: their products are NaN throughout
ZERO = 5                          # an all-zero frame


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return M.build_host_model(tmp_path_factory.mktemp("dd_profile_host_model"))


@pytest.fixture(scope="module")
def frames():
    """67 frames of products: unit steps at an amplitude per carrier and frame under noise whose level rises over a stretch of carriers
    that moves from frame to frame; records with two refused frames (stale products: NaN), an all-zero frame, single products NaN and
    infinite in frames 2 and 3; previous profiles of every kind.  Shared and read only."""
    import dabgpu
    rng = np.random.default_rng(9400)
    d = np.zeros((N, 75, 1536), np.complex64)
    c = np.arange(1536)
    for k in range(N):
        amp = (2.0e5 * (1 + k % 5) * (1.0 + 0.5 * np.cos(2 * np.pi * c / 311.0 + k))).astype(F32)
        sigma = amp.mean() * 0.1 * (1.0 + 9.0 * (np.abs(c - (k * 97) % 1536) < 60))
        step = np.exp(1j * np.pi * (rng.integers(0, 4, (75, 1536)) * 0.5 + 0.25))
        z = rng.standard_normal((75, 1536), dtype=F32) + 1j * rng.standard_normal((75, 1536), dtype=F32)
        d[k] = (amp[None, :] * step + sigma[None, :] * z).astype(np.complex64)
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
    prev = (rng.exponential(1.0, (N, 128)) * 3.0e4).astype(F32)
    prev[0] = 0.0
    prev[3] = np.nan
    prev[4, ::3], prev[4, 1::5], prev[4, 2::7], prev[4, 5::11] = 0.0, np.nan, np.inf, -1.0
    prev[1] = 7.0                                                                        # refused: must survive
    for a in (d, st, prev):
        a.setflags(write=False)
    return d, st, prev


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


def expected(host, d, st=None, exclude=None, prev=None, alpha=1.0):
    """the host model's outputs of the frames d: dict of arrays as the device writes them"""
    n = d.shape[0]
    out = {k: np.zeros((n, SIZE[k]), np.uint32 if k == "valid" else F32) for k in NAMES}
    for k in range(n):
        ok = st is None or bool(st["sync_valid"][k])
        r = M.host_frame(host, d[k] if ok else None, ok, exclude, None if prev is None else prev[k], alpha)
        out["profile_out"][k], out["band_weight"][k], out["mean_noise"][k] = r["profile"], r["band_weight"], r["mean_noise"]
        out["carrier_noise"][k], out["carrier_amplitude"][k], out["valid"][k] = r["carrier_noise"], r["carrier_amplitude"], r["valid"]
    return out


def run(ctx, d_dq, n, want, st=None, exclude=None, prev=None, alpha=1.0, names=NAMES, in_place=False, stream=None):
    """one call over the first n frames of d_dq with the outputs `names` between guard bands; asserts them equal to `want` as bit patterns,
    the bands untouched"""
    import torch
    d_st = None if st is None else torch.from_numpy(np.array(st[:n]).view(np.uint8)).cuda()
    d_ex = None if exclude is None else torch.from_numpy(np.array(exclude).view(np.int32)).cuda()
    bufs, kw = {}, {}
    for name in names:
        size = n * SIZE[name]
        bufs[name] = torch.full((GUARD + size + GUARD,), -286331154, dtype=torch.int32, device="cuda")          # 0xEEEEEEEE
        kw[name] = bufs[name][GUARD:GUARD + size]
    d_prev = None
    if prev is not None:
        d_prev = torch.from_numpy(np.array(prev[:n]).view(np.int32)).cuda()
        if in_place:
            assert "profile_out" in names
            kw["profile_out"].copy_(d_prev.view(-1))
            d_prev = kw["profile_out"]
    ctx.dd_profile(d_dq, n, sync=d_st, exclude=d_ex, profile_in=d_prev, alpha=alpha, stream=stream, **kw)
    torch.cuda.synchronize()
    seen = {}
    for name in names:
        b = bufs[name].cpu().numpy().view(np.uint32)
        assert (b[:GUARD] == 0xEEEEEEEE).all() and (b[-GUARD:] == 0xEEEEEEEE).all(), f"{name}: guard band written"
        got, exp = b[GUARD:-GUARD], want[name][:n].reshape(-1).view(np.uint32)
        assert np.array_equal(got, exp), (name, names, np.nonzero(got != exp)[0][:8], got.view(F32)[:4], want[name].reshape(-1)[:4])
        seen[name] = got
    if prev is not None and not in_place:
        assert np.array_equal(d_prev.cpu().numpy().view(np.uint32).reshape(-1), np.array(prev[:n]).view(np.uint32).reshape(-1))      # read only
    return seen


@pytest.fixture(scope="module")
def want(host, frames):
    """records, previous profiles, alpha 0.25: the expectation most tests share"""
    d, st, prev = frames
    w = expected(host, d, st, None, prev, 0.25)
    for a in w.values():
        a.setflags(write=False)
    return w


def test_equals_host_model(ctx, host, frames, device_frames, want):
    d, st, prev = frames
    assert want["valid"].sum() == N - len(REFUSED) and (want["band_weight"][want["valid"][:, 0] == 1] > 0).all()
    # NaN behind the refused records, and nothing of it arrives: zeros, and the previous profile as it was.  That the products are not even
    # read is established by reading dd_profile.hip, where the return for a refused record stands in front of the first load.
    for k in REFUSED:
        assert not want["band_weight"][k].any() and not want["carrier_noise"][k].any() and np.array_equal(want["profile_out"][k], prev[k])
    # an all-zero frame measures 0 in every band: with a state the state decays (valid), without one the frame is skipped (below)
    assert want["valid"][ZERO] == 1 and np.array_equal(want["profile_out"][ZERO], (F32(0.75) * prev[ZERO]).astype(F32))
    assert want["valid"][2] == 1 and want["carrier_noise"][2, 100] == 0 and np.isnan(want["carrier_amplitude"][2, 100])
    assert want["valid"][3] == 1 and want["carrier_noise"][3, 200] == 0 and want["carrier_noise"][3, 0] == 0
    for k in (0, 2):                                                                     # the neighbours of the refused frame: untouched by it
        alone = expected(host, d[k:k + 1], None, None, prev[k:k + 1], 0.25)
        assert np.array_equal(alone["band_weight"][0].view(np.uint32), want["band_weight"][k].view(np.uint32))
    for n in (1, 3, N):
        seen = run(ctx, device_frames, n, want, st, None, prev, 0.25)
    run(ctx, device_frames, N, want, st, None, prev, 0.25, in_place=True)
    print(f"device weights {seen['band_weight'].view(F32)[:4]}, mean noise {seen['mean_noise'].view(F32)[:3]}, {int(seen['valid'].sum())} of {N} frames valid")
    # the profile follows the louder stretch of carriers: a hundred times the noise power there, of which the estimate, with the noise
    # as large as the steps themselves and the decisions failing, still reads more than a tenth
    fresh = M.host_frame(host, d[0])["profile"]
    assert fresh.max() > 10.0 * np.median(fresh)


def test_aligned_products_and_no_records(ctx, host, frames):
    """an allocation's own start (aligned to 256 bytes and more), no records, no state: frames 3 .. 5, the last all zero and so skipped"""
    import torch
    d, st, prev = frames
    d_dq = torch.from_numpy(d[3:6].view(F32).copy()).cuda()
    exp = expected(host, d[3:6])
    assert exp["valid"][:, 0].tolist() == [1, 1, 0] and not exp["profile_out"][2].any() and not exp["band_weight"][2].any()
    run(ctx, d_dq, 3, exp)


@pytest.mark.parametrize("alpha", [1.0, 0.25])
def test_state_in_place_over_three_calls(ctx, host, frames, device_frames, alpha):
    """four receivers (a refused one among them), three calls on the same buffers with the state updated in place"""
    import torch
    d, st, prev = frames
    n = 4
    d_state = torch.zeros((n, 128), dtype=torch.float32, device="cuda")
    d_w = torch.zeros((n, 128), dtype=torch.float32, device="cuda")
    d_v = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_st = torch.from_numpy(np.array(st[:n]).view(np.uint8)).cuda()
    state = np.zeros((n, 128), F32)
    per_frame = 75 * 1536 * 2
    for lo in (0, 8, 16):
        rec = st[:n].copy()
        d_dq = device_frames[lo * per_frame:]
        ctx.dd_profile(d_dq, n, sync=d_st, profile_in=d_state, alpha=alpha, profile_out=d_state, band_weight=d_w, valid=d_v)
        torch.cuda.synchronize()
        exp = expected(host, d[lo:lo + n], rec, None, state, alpha)
        assert exp["valid"][:, 0].tolist() == [1, 0, 1, 1]
        assert np.array_equal(d_state.cpu().numpy().view(np.uint32), exp["profile_out"].view(np.uint32)), lo
        assert np.array_equal(d_w.cpu().numpy().view(np.uint32), exp["band_weight"].view(np.uint32)), lo
        assert d_v.cpu().numpy().tolist() == [1, 0, 1, 1]
        state = exp["profile_out"]
    assert not state[1].any() and state[0].all()


def test_masks(ctx, host, frames, device_frames):
    """no mask, scattered carriers, one band fully excluded (its mask is ignored), everything excluded (= no mask)"""
    d, st, prev = frames
    scattered = PM.exclude_words(np.random.default_rng(9401).choice(1536, 200, replace=False))
    band9 = PM.exclude_words(np.arange(108, 120))
    both = scattered | band9
    everything = np.full(48, 0xFFFFFFFF, np.uint32)
    plain = expected(host, d[:3], st[:3], None, prev, 0.25)
    for mask in (scattered, band9, both, everything):
        exp = expected(host, d[:3], st[:3], mask, prev, 0.25)
        run(ctx, device_frames, 3, exp, st, mask, prev, 0.25)
        same = np.array_equal(exp["profile_out"], plain["profile_out"])
        assert same == (mask is band9 or mask is everything)
        assert np.array_equal(exp["carrier_noise"], plain["carrier_noise"])             # carrier values are what they are under any mask


def test_every_subset_of_outputs(ctx, frames, device_frames, want):
    import dabgpu
    import torch
    d, st, prev = frames
    for r in range(1, len(NAMES) + 1):
        for names in itertools.combinations(NAMES, r):
            run(ctx, device_frames, 3, want, st, None, prev, 0.25, names=names)
    with pytest.raises(dabgpu.DabGpuError, match="no output"):
        ctx.dd_profile(device_frames, 1)
    d_w = torch.zeros(128, device="cuda")
    for alpha in (0.0, 1.5, float("nan")):
        with pytest.raises(dabgpu.DabGpuError, match="alpha"):
            ctx.dd_profile(device_frames, 1, band_weight=d_w, alpha=alpha)
    with pytest.raises(dabgpu.DabGpuError, match="16-byte"):
        ctx.dd_profile(device_frames[2:], 1, band_weight=d_w)


def test_captured_call_replayed_with_the_state_carried(ctx, host, frames, device_frames):
    """three receivers, one captured call, two replays on new products: the state is updated in place from replay to replay"""
    import torch
    d, st, prev = frames
    per_frame = 75 * 1536 * 2
    d_dq = torch.zeros(3 * per_frame, dtype=torch.float32, device="cuda")
    d_state = torch.zeros((3, 128), dtype=torch.float32, device="cuda")
    d_w = torch.zeros((3, 128), dtype=torch.float32, device="cuda")
    d_m = torch.zeros(3, dtype=torch.float32, device="cuda")
    d_q = torch.zeros((3, 1536), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctx.dd_profile(d_dq, 3, profile_in=d_state, alpha=0.25, profile_out=d_state, band_weight=d_w, mean_noise=d_m, carrier_noise=d_q,
                       stream=side.cuda_stream)
    state = np.zeros((3, 128), F32)
    d_state.zero_()
    for lo in (8, 16):
        d_dq.copy_(device_frames[lo * per_frame:(lo + 3) * per_frame])
        g.replay()
        torch.cuda.synchronize()
        exp = expected(host, d[lo:lo + 3], None, None, state, 0.25)
        assert exp["valid"].all()
        assert np.array_equal(d_state.cpu().numpy().view(np.uint32), exp["profile_out"].view(np.uint32)), lo
        assert np.array_equal(d_w.cpu().numpy().view(np.uint32), exp["band_weight"].view(np.uint32)), lo
        assert np.array_equal(d_m.cpu().numpy().view(np.uint32), exp["mean_noise"].reshape(-1).view(np.uint32)), lo
        assert np.array_equal(d_q.cpu().numpy().view(np.uint32), exp["carrier_noise"].view(np.uint32)), lo
        state = exp["profile_out"]


def test_host_form(ctx, host, frames):
    import dabgpu
    d, st, prev = frames
    mask = PM.exclude_words(np.arange(108, 125))
    for k, ex, alpha in ((0, None, 1.0), (2, mask, 0.25), (3, None, 0.25), (9, mask, 1.0)):
        state = prev[k].copy()
        bw, mean, ok, q, a = ctx.dd_profile_host(d[k], exclude=ex, profile=state, alpha=alpha, carriers=True)
        r = M.host_frame(host, d[k], True, ex, prev[k], alpha)
        assert ok == 1 and np.array_equal(bw.view(np.uint32), r["band_weight"].view(np.uint32)) and F32(mean).view(np.uint32) == r["mean_noise"].view(np.uint32)
        assert np.array_equal(state.view(np.uint32), r["profile"].view(np.uint32))
        assert np.array_equal(q.view(np.uint32), r["carrier_noise"].view(np.uint32)) and np.array_equal(a.view(np.uint32), r["carrier_amplitude"].view(np.uint32))
        # the two host forms of the ABI together are the same definition
        hq, ha = dabgpu.dd_profile_carriers_host(d[k])
        assert np.array_equal(hq.view(np.uint32), q.view(np.uint32)) and np.array_equal(ha.view(np.uint32), a.view(np.uint32))
        prof, hbw, hmean, hok = dabgpu.noise_profile_bands_host(hq, ex, prev[k], alpha)
        assert hok == 1 and np.array_equal(hbw.view(np.uint32), bw.view(np.uint32)) and np.array_equal(prof.view(np.uint32), state.view(np.uint32))
    bw, mean, ok = ctx.dd_profile_host(d[ZERO])
    assert ok == 0 and not bw.any() and mean == 0
    with pytest.raises(dabgpu.DabGpuError, match="alpha"):
        ctx.dd_profile_host(d[0], alpha=0.0)
