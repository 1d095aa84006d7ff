"""-m gpu: the noise profile on the device (include/dabgpu.h, "Noise profile") against the float32 host model of
tests/noise_profile_model.py (oracle PLL and transform around csrc/noise_profile_core.h), bit for bit on every output: batch sizes, both
loader paths, the synchroniser's offsets at their edges, refused and skipped frames, every kind of previous state in place and out of
place, both alphas, the masks, every subset of outputs between guard bands, a captured call replayed with the state carried, the host
form."""
import itertools

import numpy as np
import pytest

import noise_profile_model as M

pytestmark = pytest.mark.gpu

F32 = np.float32
NULL = 2656
STRIDE = 5000                     # >= 701 + 2656 + 1543, even: the parity of a window is that of null offset + fine time offset
GUARD = 1024                      # floats: 4 KB on either side of every output
NAMES = ("profile_out", "band_weight", "mean_noise", "carrier_power", "valid")
SIZE = dict(profile_out=128, band_weight=128, mean_noise=1, carrier_power=1536, valid=1)
FTO = [0, -504, 1543, 37, -120, 1500, 64, -1]
REFUSED = {2: (0, 0), 5: (1, -505), 6: (1, 1544), 40: (0, 99), 41: (1, 3000), 42: (1, -3000)}      # frame: (sync_valid, fine_time_offset)
TXS = [(11, 5), (40, 17), (0, 0), (69, 23)]


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def model(oracle, tmp_path_factory):
    return M.HostModel(M.build_host_model(tmp_path_factory.mktemp("noise_profile_host_model")), oracle)


@pytest.fixture(scope="module")
def frames():
    """65 slices of noise of a level of their own, coloured across the block (a louder stretch of carriers), loud samples everywhere
    behind the refused records; records as a synchroniser would leave them; a caller's offsets, NaN (none) for most; previous profiles of
    every kind: valid, zero, NaN, mixed per band.  Shared and read only."""
    import dabgpu
    rng = np.random.default_rng(9300)
    n = 65
    x = np.zeros((n, STRIDE), np.complex64)
    st = np.zeros(n, np.dtype(dabgpu.SYNC_STATE_DTYPE))
    t = np.arange(STRIDE)
    for k in range(n):
        sigma = 0.05 * (1 + k % 7)
        s = sigma * (rng.standard_normal(STRIDE) + 1j * rng.standard_normal(STRIDE))
        jam = rng.standard_normal(STRIDE) + 1j * rng.standard_normal(STRIDE)
        jam = np.convolve(jam, np.ones(24) / 24.0, mode="same") * np.exp(2j * np.pi * ((k * 37) % 1400 - 700) / 2048.0 * t)
        x[k] = s + 4.0 * sigma * jam
        st["sync_valid"][k], st["fine_time_offset"][k] = 1, FTO[k % len(FTO)]
        st["freq_coarse"][k] = F32((k % 9 - 4) / 2048.0)
        st["freq_fine"][k] = F32(0.013 * (k % 11 - 5) / 2048.0)
    for k, (valid, fto) in REFUSED.items():
        st["sync_valid"][k], st["fine_time_offset"][k] = valid, fto
        x[k] *= 1.0e6
    caller = np.full(n, np.nan, F32)
    caller[[1, 4, 33, 64]] = F32([0.0, 2.5 / 2048, -0.3 / 2048, 1e-3])
    prev = (rng.exponential(1.0, (n, 128)) * 0.01).astype(F32)
    prev[1] = 0.0
    prev[3] = np.nan
    prev[4, ::3], prev[4, 1::5], prev[4, 2::7], prev[4, 5::11] = 0.0, np.nan, np.inf, -1.0
    prev[2] = 7.0                                                                        # refused: must survive
    for a in (x, st, caller, prev):
        a.setflags(write=False)
    return x, st, caller, prev


def expected(model, x, off, st=None, caller=None, exclude=None, prev=None, alpha=1.0):
    """the host model's outputs of the frames x: dict of arrays as the device writes them"""
    n = x.shape[0]
    out = {k: np.zeros((n, SIZE[k]), np.uint32 if k == "valid" else F32) for k in NAMES}
    if prev is not None:
        out["profile_out"][:] = prev[:n]
    for k in range(n):
        fto, f = 0, F32(0.0)
        if st is not None:
            fto = int(st["fine_time_offset"][k])
            if not st["sync_valid"][k] or not -504 <= fto <= 1543 or off + fto < 0:
                continue
            f = F32(st["freq_coarse"][k]) + F32(st["freq_fine"][k])
        if caller is not None and caller[k] == caller[k]:
            f = caller[k]
        r = model.profile(x[k], off + fto, f, exclude, None if prev is None else prev[k], alpha)
        out["profile_out"][k], out["band_weight"][k], out["mean_noise"][k] = r["profile"], r["band_weight"], r["mean_noise"]
        out["carrier_power"][k], out["valid"][k] = r["carrier_power"], r["valid"]
    return out


def run(ctx, x, off, want, st=None, caller=None, exclude=None, prev=None, alpha=1.0, names=NAMES, in_place=False, stream=None):
    """one call with the outputs `names` between guard bands; asserts them equal to `want` as bit patterns, the bands untouched"""
    import torch
    n = x.shape[0]
    d_iq = torch.from_numpy(np.array(x).view(np.float32)).cuda()
    d_st = None if st is None else torch.from_numpy(np.array(st).view(np.uint8)).cuda()
    d_fq = None if caller is None else torch.from_numpy(np.array(caller)).cuda()
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
    ctx.noise_profile(d_iq, n, x.shape[1], off, states=d_st, freq_offset=d_fq, exclude=d_ex, profile_in=d_prev, alpha=alpha, stream=stream, **kw)
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


@pytest.mark.parametrize("off", [700, 701])
def test_equals_host_model(ctx, model, frames, off):
    """n_frames 1, 3, 65 with records, caller offsets and previous profiles at alpha 0.25; null offsets 700 / 701 put the same fine time
    offsets on even and on odd samples"""
    x, st, caller, prev = frames
    want = expected(model, x, off, st, caller, None, prev, 0.25)
    assert want["valid"].sum() == 65 - len(REFUSED) and (want["band_weight"][want["valid"][:, 0] == 1] > 0).all()
    # Loud samples behind the refused records, and nothing of them arrives: zeros, and the previous profile as it was.  That they are not
    # even READ is established by reading noise_profile.hip, where the return for a refused record stands in front of the first access
    # to the frame's samples (a test must not make a read fault on purpose).
    for k in REFUSED:
        assert not want["band_weight"][k].any() and not want["carrier_power"][k].any() and np.array_equal(want["profile_out"][k], prev[k])
    for n in (1, 3, 65):
        seen = run(ctx, x[:n], off, want, st[:n], caller[:n], None, prev, 0.25)
    run(ctx, x, off, want, st, caller, None, prev, 0.25, in_place=True)
    print(f"null offset {off}: device weights {seen['band_weight'].view(F32)[:4]}, mean noise {seen['mean_noise'].view(F32)[:3]}, "
          f"{int(seen['valid'].sum())} of 65 frames valid")
    # the profile itself is not flat: the convolution puts the interferer into about 2048 / 24 bins at 16 times the noise there
    fresh = model.profile(x[0], off, F32(st["freq_coarse"][0]) + F32(st["freq_fine"][0]))["profile"]
    assert fresh.max() > 4.0 * np.median(fresh)


def test_without_records_and_offsets(ctx, model, frames):
    x, st, caller, prev = frames
    run(ctx, x[:3], 701, expected(model, x[:3], 701))
    run(ctx, x[:3], 700, expected(model, x[:3], 700, None, caller[:3]), None, caller[:3])
    want = expected(model, x[:3], 0, st[:3])                                             # offset -504 at null offset 0: in front of the slice
    assert want["valid"][:, 0].tolist() == [1, 0, 0]
    run(ctx, x[:3], 0, want, st[:3])


@pytest.mark.parametrize("alpha", [1.0, 0.25])
def test_previous_state_of_every_kind(ctx, model, frames, alpha):
    """frames 0 .. 4: a valid state, a zeroed one, a refused frame, NaN, mixed per band -- out of place and in place; without a state"""
    x, st, caller, prev = frames
    want = expected(model, x[:5], 700, st[:5], None, None, prev, alpha)
    assert want["valid"][:, 0].tolist() == [1, 1, 0, 1, 1]
    fresh = expected(model, x[:5], 700, st[:5])
    assert np.array_equal(want["profile_out"][1], fresh["profile_out"][1]) and np.array_equal(want["profile_out"][3], fresh["profile_out"][3])
    mixed_ok = np.isfinite(prev[4]) & (prev[4] > 0)
    assert np.array_equal(want["profile_out"][4][~mixed_ok], fresh["profile_out"][4][~mixed_ok])
    if alpha == 1.0:
        assert np.allclose(want["profile_out"][0], fresh["profile_out"][0], rtol=1e-5)
    else:
        assert not np.array_equal(want["profile_out"][0], fresh["profile_out"][0])
    run(ctx, x[:5], 700, want, st[:5], None, None, prev, alpha)
    run(ctx, x[:5], 700, want, st[:5], None, None, prev, alpha, in_place=True)
    run(ctx, x[:5], 700, fresh, st[:5], alpha=alpha)


def test_masks(ctx, model, frames):
    """no mask, the TII carriers of four transmitters, one band fully excluded (its mask is ignored), everything excluded (= no mask)"""
    import dabgpu
    x, st, caller, prev = frames
    tii = dabgpu.noise_profile_exclude(TXS)
    band9 = M.exclude_words(np.arange(108, 120))
    everything = np.full(48, 0xFFFFFFFF, np.uint32)
    plain = expected(model, x[:3], 700, st[:3], None, None, prev, 0.25)
    for mask in (tii, band9, everything):
        want = expected(model, x[:3], 700, st[:3], None, mask, prev, 0.25)
        run(ctx, x[:3], 700, want, st[:3], None, mask, prev, 0.25)
        same = np.array_equal(want["profile_out"], plain["profile_out"])
        assert same == (mask is not tii)
    # (carrier powers are what they are under any mask)
    assert np.array_equal(expected(model, x[:3], 700, st[:3], None, tii)["carrier_power"], plain["carrier_power"])


def test_every_subset_of_outputs(ctx, model, frames):
    import dabgpu
    import torch
    x, st, caller, prev = frames
    want = expected(model, x[:3], 700, st[:3], caller[:3], None, prev, 0.25)
    for r in range(1, len(NAMES) + 1):
        for names in itertools.combinations(NAMES, r):
            run(ctx, x[:3], 700, want, st[:3], caller[:3], None, prev, 0.25, names=names)
    d_iq = torch.zeros((STRIDE, 2), device="cuda")
    with pytest.raises(dabgpu.DabGpuError, match="no output"):
        ctx.noise_profile(d_iq, 1, STRIDE, 700)
    d_w = torch.zeros(128, device="cuda")
    for alpha in (0.0, 1.5, float("nan")):
        with pytest.raises(dabgpu.DabGpuError, match="alpha"):
            ctx.noise_profile(d_iq, 1, STRIDE, 700, band_weight=d_w, alpha=alpha)


def test_skipped_frames(ctx, model, frames):
    """a NaN in the NULL window, an infinity, an all-zero NULL without a state (skipped) and with one (the state decays), an ordinary one"""
    x, st, caller, prev = frames
    y = x[7:12].copy()
    y[0, 700 + 608 + 1000] = np.nan
    y[1, 700 + 608 + 2047] = np.inf
    y[2, 700:700 + NULL] = 0
    y[3, 700:700 + NULL] = 0
    p = prev[7:12].copy()
    p[2] = 0.0
    want = expected(model, y, 700, None, None, None, p, 0.25)
    assert want["valid"][:, 0].tolist() == [0, 0, 0, 1, 1]
    for k in range(3):
        assert np.array_equal(want["profile_out"][k], p[k]) and not want["band_weight"][k].any() and want["mean_noise"][k] == 0
    assert np.array_equal(want["profile_out"][3], (F32(0.75) * p[3]).astype(F32))
    run(ctx, y, 700, want, None, None, None, p, 0.25)
    run(ctx, y, 700, want, None, None, None, p, 0.25, in_place=True)
    none = expected(model, y, 700)
    assert none["valid"][:, 0].tolist() == [0, 0, 0, 0, 1] and not none["profile_out"][:4].any()
    run(ctx, y, 700, none)


def test_captured_call_replayed_with_the_state_carried(ctx, model, frames):
    """three receivers, one captured call, three replays on new samples: the state is updated in place from replay to replay"""
    import torch
    x, st, caller, prev = frames
    d_iq = torch.from_numpy(x[:3].view(np.float32).copy()).cuda()
    d_st = torch.from_numpy(st[8:11].view(np.uint8).copy()).cuda()
    d_state = torch.zeros((3, 128), dtype=torch.float32, device="cuda")
    d_w = torch.zeros((3, 128), dtype=torch.float32, device="cuda")
    d_m = torch.zeros(3, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctx.noise_profile(d_iq, 3, STRIDE, 700, states=d_st, profile_in=d_state, alpha=0.25, profile_out=d_state, band_weight=d_w, mean_noise=d_m,
                          stream=side.cuda_stream)
    state = np.zeros((3, 128), F32)
    d_state.zero_()
    for lo in (8, 16, 24):
        d_iq.copy_(torch.from_numpy(x[lo:lo + 3].view(np.float32).copy()))
        g.replay()
        torch.cuda.synchronize()
        want = expected(model, x[lo:lo + 3], 700, st[8:11], None, None, state, 0.25)
        assert want["valid"].all()
        assert np.array_equal(d_state.cpu().numpy().view(np.uint32), want["profile_out"].view(np.uint32)), lo
        assert np.array_equal(d_w.cpu().numpy().view(np.uint32), want["band_weight"].view(np.uint32)), lo
        assert np.array_equal(d_m.cpu().numpy().view(np.uint32), want["mean_noise"].reshape(-1).view(np.uint32)), lo
        state = want["profile_out"]


def test_host_form(ctx, model, frames):
    import dabgpu
    x, st, caller, prev = frames
    tii = dabgpu.noise_profile_exclude(TXS)
    for k, fto, f, mask, alpha in ((0, 0, 0.0, None, 1.0), (3, 37, 1.5 / 2048, tii, 0.25), (9, -504, -1e-3, None, 0.25), (10, 1543, 0.0, tii, 1.0)):
        state = prev[k].copy()
        bw, mean, ok, cp = ctx.noise_profile_host(x[k], 700, freq_offset=f, fine_time_offset=fto, exclude=mask, profile=state, alpha=alpha,
                                                  carrier_power=True)
        r = model.profile(x[k], 700 + fto, F32(f), mask, prev[k], alpha)
        assert ok == 1 and np.array_equal(bw.view(np.uint32), r["band_weight"].view(np.uint32)) and F32(mean).view(np.uint32) == r["mean_noise"].view(np.uint32)
        assert np.array_equal(state.view(np.uint32), r["profile"].view(np.uint32)) and np.array_equal(cp.view(np.uint32), r["carrier_power"].view(np.uint32))
    bw, mean, ok = ctx.noise_profile_host(x[0], 700)
    assert ok == 1 and np.array_equal(bw.view(np.uint32), model.profile(x[0], 700)["band_weight"].view(np.uint32))
    with pytest.raises(dabgpu.DabGpuError):
        ctx.noise_profile_host(x[0][:700 + NULL - 1], 700)                                 # the NULL leaves the samples
    with pytest.raises(dabgpu.DabGpuError):
        ctx.noise_profile_host(x[0], 0, fine_time_offset=-1)
    for fto in (-505, 1544):
        with pytest.raises(dabgpu.DabGpuError, match="fine_time_offset"):
            ctx.noise_profile_host(x[0], 700, fine_time_offset=fto)
    with pytest.raises(dabgpu.DabGpuError, match="alpha"):
        ctx.noise_profile_host(x[0], 700, alpha=0.0)
    assert ctx.noise_profile_host(x[0][:700 + NULL], 700)[2] == 1
