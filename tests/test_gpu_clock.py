"""-m gpu: the sampling-clock tracker on the device (include/dabgpu.h, "Sampling-clock tracker") against the float32 host model of
tests/clock_model.py (csrc/clock_core.h compiled by g++), bit for bit: slopes, residuals, sums and valid words of the estimator, every
float of the de-rotator.  Batches of 1, 2 (one frame refused through its record, its stale products NaN) and 5 frames -- a frame is one
workgroup's whole job, nothing larger shows more; products aligned to 16 bytes and no more; priors, gains, the state in place; an
all-zero frame, NaN products, every output absent in turn between guard bands; the de-rotator at every run length 1 .. 75 and the
planner's own, in place and out of place, a slope-0 frame, a skipped frame's bytes; a captured graph of both calls over an in-place
state replayed three times; the host form."""
import numpy as np
import pytest

import clock_model as M

pytestmark = pytest.mark.gpu

F32 = np.float32
N = 5
GUARD = 4096                      # bytes on either side of every output
NAMES = ("slope_out", "residual", "corr", "valid")
BYTES = dict(slope_out=8, residual=8, corr=8, valid=4)
ZERO = 2                          # an all-zero frame: skipped by its own sum
PPM = (200.0, -150.0, 0.0, 35.0, 900.0)
PRIOR_PPM = (0.0, -140.0, 77.0, 0.0, 999.0)
PER_FRAME = 75 * 1536 * 2         # floats


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return M.build_host_model(tmp_path_factory.mktemp("clock_host_model"))


@pytest.fixture(scope="module")
def frames():
    """five frames of products under noise with different ramps; frame 1 has NaN and infinite products, frame 2 is all zero.  Shared and
    read only."""
    rng = np.random.default_rng(9700)
    d = np.zeros((N, 75, 1536), np.complex64)
    for k in range(N):
        d[k] = M.products(rng, PPM[k], snr_db=(20.0, 18.0, 20.0, None, 20.0)[k], amplitude=300.0 * (1 + k))
    d[ZERO] = 0
    d[1, 10] = np.nan                                       # a NaN row
    d[1, 40, 100] = complex(1.0, np.inf)
    d[1, 74, 1535] = complex(np.nan, 0.0)
    d[4, 0, 0] = complex(-np.inf, 1.0)
    d.setflags(write=False)
    return d


def on_device(d, offset_floats=4):
    """the products on the device, 16 bytes behind an allocation's start: aligned to 16 bytes and to no more"""
    import torch
    buf = torch.zeros(d.size * 2 + offset_floats, dtype=torch.float32, device="cuda")
    view = buf[offset_floats:]
    view.copy_(torch.from_numpy(d.view(F32).reshape(-1).copy()))
    assert offset_floats != 4 or view.data_ptr() % 32 == 16
    return view


@pytest.fixture(scope="module")
def device_frames(frames):
    return on_device(frames)


def sync_records(valid):
    import dabgpu
    st = np.zeros(len(valid), np.dtype(dabgpu.SYNC_STATE_DTYPE))
    st["sync_valid"] = valid
    return st


def expected(host, d, slope_in, gain, valid=None):
    n = d.shape[0]
    out = dict(slope_out=np.zeros(n, np.int64), residual=np.zeros(n, np.int64), corr=np.zeros((n, 2), F32), valid=np.zeros(n, np.uint32))
    for k in range(n):
        ok = valid is None or bool(valid[k])
        e = M.host_estimate(host, d[k] if ok else None, 0 if slope_in is None else int(slope_in[k]), gain, ok)
        out["slope_out"][k], out["residual"][k], out["corr"][k], out["valid"][k] = e["slope"], e["residual"], e["corr"], e["valid"]
    return out


def run_estimate(ctx, d_dq, n, want, slope_in=None, gain=1.0, valid=None, names=NAMES, in_place=False, stream=None):
    """one call over the first n frames with the outputs `names` between guard bands; asserts them equal to `want` as bytes, the bands
    untouched"""
    import torch
    d_st = None if valid is None else torch.from_numpy(sync_records(valid).view(np.uint8)).cuda()
    d_in = None if slope_in is None else torch.from_numpy(np.asarray(slope_in[:n], np.int64)).cuda()
    bufs, kw = {}, {}
    for name in names:
        size = n * BYTES[name]
        bufs[name] = torch.full((GUARD + size + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        kw[name] = bufs[name][GUARD:GUARD + size]
    if in_place:
        kw["slope_out"] = d_in
    ctx.clock_estimate(d_dq, n, sync=d_st, slope_in=d_in, gain=gain, stream=stream, **kw)
    torch.cuda.synchronize()
    for name in names:
        b = bufs[name].cpu().numpy()
        if in_place and name == "slope_out":
            assert (b == 0xEE).all()
            got = d_in.cpu().numpy().view(np.uint8)
        else:
            assert (b[:GUARD] == 0xEE).all() and (b[-GUARD:] == 0xEE).all(), f"{name}: guard band written"
            got = b[GUARD:-GUARD]
        exp = np.ascontiguousarray(want[name][:n]).view(np.uint8).reshape(-1)
        assert np.array_equal(got, exp), (name, names, got[:16], exp[:16])


def test_estimator_equals_host_model(ctx, host, frames, device_frames):
    prior = [M.slope_q64(p) for p in PRIOR_PPM]
    plain = expected(host, frames, None, 1.0)
    assert plain["valid"].tolist() == [1, 1, 0, 1, 1] and plain["slope_out"][ZERO] == 0 and not plain["corr"][ZERO].any()
    for k in (0, 1, 3, 4):                                                               # one frame from a zero state, under noise
        assert abs(M.ppm_of(plain["slope_out"][k]) - PPM[k]) < 0.1 * abs(PPM[k]) + 1.0, (k, M.ppm_of(plain["slope_out"][k]))
    for n in (1, 2, N):
        run_estimate(ctx, device_frames, n, plain)
        run_estimate(ctx, device_frames, n, expected(host, frames[:n], prior, 1.0), slope_in=prior)
        run_estimate(ctx, device_frames, n, expected(host, frames[:n], prior, 0.375), slope_in=prior, gain=0.375, in_place=True)
    # two frames, the first refused through its record: its products are stale (NaN here) and none of them arrives
    stale = frames[:2].copy()
    stale[0] = complex(np.nan, np.nan)
    want = expected(host, stale, prior, 1.0, valid=[0, 1])
    assert want["valid"].tolist() == [0, 1] and want["slope_out"][0] == prior[0] and want["residual"][0] == 0 and not want["corr"][0].any()
    run_estimate(ctx, on_device(stale), 2, want, slope_in=prior, valid=[0, 1])
    run_estimate(ctx, on_device(stale), 2, want, slope_in=prior, valid=[0, 1], in_place=True)
    print("tracked from zero:", [round(M.ppm_of(s), 2) for s in plain["slope_out"]], "ppm for", PPM)


def test_every_output_absent_in_turn(ctx, host, frames, device_frames):
    import dabgpu
    import torch
    prior = [M.slope_q64(p) for p in PRIOR_PPM]
    want = expected(host, frames, prior, 1.0)
    for absent in NAMES:
        run_estimate(ctx, device_frames, N, want, slope_in=prior, names=tuple(x for x in NAMES if x != absent))
    for only in NAMES:
        run_estimate(ctx, device_frames, 2, want, slope_in=prior, names=(only,))
    d_s = torch.zeros(N, dtype=torch.int64, device="cuda")
    with pytest.raises(dabgpu.DabGpuError, match="no output"):
        ctx.clock_estimate(device_frames, 1)
    with pytest.raises(dabgpu.DabGpuError, match="16-byte"):
        ctx.clock_estimate(device_frames[2:], 1, slope_out=d_s)
    with pytest.raises(dabgpu.DabGpuError, match="gain"):
        ctx.clock_estimate(device_frames, 1, slope_out=d_s, gain=0.0)
    with pytest.raises(dabgpu.DabGpuError, match="overlap"):
        ctx.clock_derotate(device_frames, device_frames[PER_FRAME:], 2, d_s)


def test_derotator_equals_host_model_at_every_split(ctx, host, frames, device_frames):
    import dabgpu
    import torch
    slopes = np.array([M.slope_q64(200.0), 0, -M.MAX_SLOPE, 1, M.slope_q64(-3.3)], np.int64)      # frame 1 (NaN rows) is a copy, frame 3 the smallest ramp
    want = np.stack([M.host_derotate(host, frames[k], slopes[k]) for k in range(N)])
    assert want[1].tobytes() == frames[1].tobytes() and want[3].tobytes() != frames[3].tobytes()
    d_want = torch.from_numpy(want.view(np.int32).reshape(-1).copy()).cuda()
    d_slope = torch.from_numpy(slopes).cuda()
    d_out = torch.zeros(N * PER_FRAME + 4, dtype=torch.float32, device="cuda")[4:]
    auto = {dabgpu.clock_derotate_plan(device_frames, d_out, n, d_slope).symbols_per_block for n in (1, 2, N)}
    assert auto and all(1 <= s <= 75 for s in auto)
    for n in (1, 2, N):
        for spb in [0] + (list(range(1, 76)) if n == 2 else sorted(auto | {1, 4, 5, 7, 75})):
            d_out.fill_(float("nan"))
            ctx.clock_derotate(device_frames, d_out, n, d_slope, symbols_per_block=spb)
            assert torch.equal(d_out[:n * PER_FRAME].view(torch.int32), d_want[:n * PER_FRAME]), (n, spb)
            assert torch.isnan(d_out[n * PER_FRAME:]).all()
    # in place equals out of place
    for spb in (0, 75, 13):
        d_io = device_frames.clone()
        ctx.clock_derotate(d_io, d_io, N, d_slope, symbols_per_block=spb)
        assert torch.equal(d_io.view(torch.int32), d_want), spb
    torch.cuda.synchronize()


def test_skipped_and_slope_zero_frames_are_left_alone(ctx, host, frames, device_frames):
    import torch
    slopes = np.array([M.slope_q64(200.0), M.slope_q64(50.0), 0, M.slope_q64(-20.0), 0], np.int64)
    valid = [1, 0, 1, 0, 1]
    d_slope = torch.from_numpy(slopes).cuda()
    d_st = torch.from_numpy(sync_records(valid).view(np.uint8)).cuda()
    pattern = -286331154                                                                 # 0xEEEEEEEE
    d_out = torch.full((N * PER_FRAME,), pattern, dtype=torch.int32, device="cuda")
    ctx.clock_derotate(device_frames, d_out.view(torch.float32), N, d_slope, sync=d_st)
    got = d_out.cpu().numpy().reshape(N, PER_FRAME)
    assert (got[1] == pattern).all() and (got[3] == pattern).all()                       # skipped through the record: not written
    assert got[0].tobytes() == M.host_derotate(host, frames[0], slopes[0]).tobytes()
    assert got[2].tobytes() == frames[2].tobytes() and got[4].tobytes() == frames[4].tobytes()      # slope 0 out of place: a copy
    # in place: the skipped frames and the slope-0 frames keep their bytes, NaN payloads included
    src = frames.copy().view(np.uint32).reshape(N, PER_FRAME)
    src[:, :4] = [0x7FC01234, 0xFFC00001, 0x80000000, 0x00000001]
    d_io = torch.from_numpy(src.view(np.int32).copy()).cuda()
    ctx.clock_derotate(d_io.view(torch.float32), d_io.view(torch.float32), N, d_slope, sync=d_st)
    back = d_io.cpu().numpy().view(np.uint32)
    for k in (1, 2, 3, 4):
        assert np.array_equal(back[k], src[k]), k
    assert back[0].tobytes() == M.host_derotate(host, src[0].view(np.complex64), slopes[0]).tobytes()


def test_captured_graph_tracks_over_an_in_place_state(ctx, host, frames, device_frames):
    """estimate and de-rotate in one captured graph, the state array in place: three replays are three steps of the host model"""
    import torch
    n = 2
    d_state = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_ok = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(n * PER_FRAME, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctx.clock_estimate(device_frames, n, slope_in=d_state, gain=0.75, slope_out=d_state, residual=d_res, valid=d_ok, stream=side.cuda_stream)
        ctx.clock_derotate(device_frames, d_out, n, d_state, stream=side.cuda_stream)
    d_state.zero_()
    state, left = [0] * n, [abs(PPM[0])]
    for step in range(3):
        g.replay()
        torch.cuda.synchronize()
        for k in range(n):
            e = M.host_estimate(host, frames[k], state[k], 0.75)
            state[k] = e["slope"]
            assert d_state[k].item() == e["slope"] and d_res[k].item() == e["residual"] and d_ok[k].item() == 1, (step, k)
            assert d_out[k * PER_FRAME:(k + 1) * PER_FRAME].cpu().numpy().tobytes() == M.host_derotate(host, frames[k], state[k]).tobytes(), (step, k)
        left.append(abs(PPM[0] - M.ppm_of(state[0])))
    assert left[0] > left[1] > left[2] > left[3]                                         # every replay goes on tracking
    print("state after three replays:", [round(M.ppm_of(s), 2) for s in state], "ppm")


def test_host_form(ctx, host, frames):
    import dabgpu
    for k, s_in in ((0, 0), (1, M.slope_q64(-140.0)), (4, M.slope_q64(999.0))):
        out, s, corr, ok = ctx.clock_track_host(frames[k], s_in, 1.0)
        e = M.host_estimate(host, frames[k], s_in, 1.0)
        assert ok == 1 and s == e["slope"] and corr.tobytes() == e["corr"].tobytes()
        assert out.tobytes() == M.host_derotate(host, frames[k], s).tobytes()
        hs, hcorr, hok = dabgpu.clock_estimate_host(frames[k], s_in)                     # the host form of the ABI is the same definition
        assert (hs, hok) == (s, 1) and hcorr.tobytes() == corr.tobytes()
        assert dabgpu.clock_derotate_host(frames[k], s).tobytes() == out.tobytes()
    out, s, corr, ok = ctx.clock_track_host(frames[ZERO], 4242, 0.5)
    assert ok == 0 and s == 4242 and not corr.any() and out.tobytes() == M.host_derotate(host, frames[ZERO], 4242).tobytes()
    none, s, corr, ok = ctx.clock_track_host(frames[0], 0, 1.0, derotate=False)
    assert none is None and ok == 1 and s == M.host_estimate(host, frames[0], 0, 1.0)["slope"]
