"""-m gpu: the noise estimator on the device (include/dabgpu.h, "Noise estimate") against the float32 host model of tests/noise_model.py
(oracle PLL and transform around csrc/noise_core.h), bit for bit on every output: batch sizes, both loader paths, the synchroniser's
offsets at their edges, refused and skipped frames, caller offsets, every subset of outputs between guard bands, TII on the air, the
TII bank's accumulator, a captured call replayed, the host form."""
import itertools

import numpy as np
import pytest

import noise_model as M

pytestmark = pytest.mark.gpu

NULL, REACH = 2656, 2656 + 2552
STRIDE = 7600                     # >= 701 + REACH + 1543, even: the parity of a window is that of null offset + fine time offset
GUARD = 1024                      # floats: 4 KB on either side of every output
NAMES = ("noise_power", "signal_power", "weight", "snr", "group_energy", "valid")
FTO = [0, -504, 1543, 37, -120, 1500, 64, -1]
REFUSED = {2: (0, 0), 5: (1, -505), 6: (1, 1544), 40: (0, 99), 41: (1, 3000), 42: (1, -3000)}      # frame: (sync_valid, fine_time_offset)


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return M.build_host_model(tmp_path_factory.mktemp("noise_host_model"))


@pytest.fixture(scope="module")
def frames():
    """65 slices: noise of a level of their own everywhere, a louder symbol from the expected PRS position on; records as a synchroniser
    would leave them, some refused; a caller's offsets, NaN (none) for most.  Shared and read only."""
    import dabgpu
    rng = np.random.default_rng(9100)
    n = 65
    x = np.zeros((n, STRIDE), np.complex64)
    st = np.zeros(n, np.dtype(dabgpu.SYNC_STATE_DTYPE))
    for k in range(n):
        sigma, amp = 0.05 * (1 + k % 7), 3.0 + (k % 5)
        s = sigma * (rng.standard_normal(STRIDE) + 1j * rng.standard_normal(STRIDE))
        a = 700 + FTO[k % len(FTO)] + NULL + 8          # (8: the NULL window of null offset 701 stays in the noise as well)
        s[a:] += amp * (rng.standard_normal(STRIDE - a) + 1j * rng.standard_normal(STRIDE - a))
        x[k] = s
        st["sync_valid"][k], st["fine_time_offset"][k] = 1, FTO[k % len(FTO)]
        st["freq_coarse"][k] = np.float32((k % 9 - 4) / 2048.0)
        st["freq_fine"][k] = np.float32(0.013 * (k % 11 - 5) / 2048.0)
    for k, (valid, fto) in REFUSED.items():
        st["sync_valid"][k], st["fine_time_offset"][k] = valid, fto
    caller = np.full(n, np.nan, np.float32)
    caller[[1, 4, 33, 64]] = np.float32([0.0, 2.5 / 2048, -0.3 / 2048, 1e-3])
    for a in (x, st, caller):
        a.setflags(write=False)
    return x, st, caller


def expected(model, x, off, st=None, caller=None):
    """the host model's outputs of the frames x: dict of arrays as the device writes them"""
    n = x.shape[0]
    out = {k: np.zeros(n, np.float32) for k in NAMES[:4]}
    out["group_energy"] = np.zeros((n, 192), np.float32)
    out["valid"] = np.zeros(n, np.uint32)
    for k in range(n):
        fto, f = 0, np.float32(0.0)
        if st is not None:
            fto = int(st["fine_time_offset"][k])
            if not st["sync_valid"][k] or not -504 <= fto <= 1543 or off + fto < 0:
                continue
            f = np.float32(st["freq_coarse"][k]) + np.float32(st["freq_fine"][k])
        if caller is not None and caller[k] == caller[k]:
            f = caller[k]
        rec, E = model.estimate(x[k], off + fto, f)
        for name in NAMES[:4]:
            out[name][k] = rec[name]
        out["group_energy"][k], out["valid"][k] = E, rec["valid"]
    return out


def run(ctx, x, off, want, st=None, caller=None, names=NAMES, stream=None):
    """one call with the outputs `names` between guard bands; asserts them equal to `want` as bit patterns, the bands untouched"""
    import torch
    n = x.shape[0]
    d_iq = torch.from_numpy(np.array(x).view(np.float32)).cuda()
    d_st = None if st is None else torch.from_numpy(np.array(st).view(np.uint8)).cuda()
    d_fq = None if caller is None else torch.from_numpy(np.array(caller)).cuda()
    bufs, kw = {}, {}
    for name in names:
        size = n * (192 if name == "group_energy" else 1)
        bufs[name] = torch.full((GUARD + size + GUARD,), -286331154, dtype=torch.int32, device="cuda")          # 0xEEEEEEEE
        kw[name] = bufs[name][GUARD:GUARD + size]
    ctx.noise_estimate(d_iq, n, x.shape[1], off, states=d_st, freq_offset=d_fq, stream=stream, **kw)
    torch.cuda.synchronize()
    seen = {}
    for name in names:
        b = bufs[name].cpu().numpy().view(np.uint32)
        assert (b[:GUARD] == 0xEEEEEEEE).all() and (b[-GUARD:] == 0xEEEEEEEE).all(), f"{name}: guard band written"
        got, exp = b[GUARD:-GUARD], want[name].reshape(-1).view(np.uint32)
        assert np.array_equal(got, exp), (name, names, np.nonzero(got != exp)[0][:8], got.view(np.float32)[:4], want[name].reshape(-1)[:4])
        seen[name] = got
    return seen


@pytest.mark.parametrize("off", [700, 701])
def test_equals_host_model(ctx, oracle, host, frames, off):
    """n_frames 1, 3, 65 with records and caller offsets; null offsets 700 / 701 put the same fine time offsets on even and on odd samples"""
    x, st, caller = frames
    model = M.HostModel(host, oracle)
    want = expected(model, x, off, st, caller)
    assert want["valid"].sum() == 65 - len(REFUSED) and (want["weight"][want["valid"] == 1] > 0).all()
    # Loud samples behind the refused records, and nothing of them arrives.  That they are not even READ is not something this test can
    # see (the kernel writes zeros for such a frame either way, and a test must not make a read fault on purpose): it is established by
    # reading noise.hip, where the return for a refused record stands in front of the first access to the frame's samples.
    for k in REFUSED:
        assert not want["weight"][k] and not want["group_energy"][k].any()
    for n in (1, 3, 65):
        seen = run(ctx, x[:n], off, {k: v[:n] for k, v in want.items()}, st[:n], caller[:n])
    print(f"null offset {off}: device weights {seen['weight'].view(np.float32)[:4]} model {want['weight'][:4]}, snr {seen['snr'].view(np.float32)[:2]}, "
          f"{int(seen['valid'].sum())} of 65 frames valid")
    # the estimate itself: N within five of the model's deviations of the noise that was put in
    for k in np.nonzero(want["valid"])[0]:
        s2 = 2.0 * (0.05 * (1 + k % 7)) ** 2
        assert abs(want["noise_power"][k] / s2 - 1.0) < 5.0 * M.relative_deviation(), k


def test_without_records_and_offsets(ctx, oracle, host, frames):
    x, st, caller = frames
    model = M.HostModel(host, oracle)
    run(ctx, x[:3], 701, expected(model, x[:3], 701))
    run(ctx, x[:3], 700, expected(model, x[:3], 700, None, caller[:3]), None, caller[:3])
    run(ctx, x[:3], 0, expected(model, x[:3], 0, st[:3]), st[:3])                         # offset -504 at null offset 0: in front of the slice
    assert expected(model, x[:3], 0, st[:3])["valid"].tolist() == [1, 0, 0]


def test_every_subset_of_outputs(ctx, oracle, host, frames):
    x, st, caller = frames
    model = M.HostModel(host, oracle)
    want = expected(model, x[:3], 700, st[:3], caller[:3])
    for r in range(1, 6):
        for names in itertools.combinations(NAMES, r):
            run(ctx, x[:3], 700, want, st[:3], caller[:3], names=names)
    import dabgpu
    import torch
    with pytest.raises(dabgpu.DabGpuError) as err:
        ctx.noise_estimate(torch.zeros((STRIDE, 2), device="cuda"), 1, STRIDE, 700)
    assert "no output" in str(err.value)


def test_skipped_frames(ctx, oracle, host, frames):
    """a NaN in the NULL window, a NaN in the PRS, an infinity, an all-zero NULL (the cap: finite), an all-zero frame (skipped)"""
    x, st, caller = frames
    y = x[:6].copy()
    y[0, 700 + 608 + 1000] = np.nan
    y[1, 700 + NULL + 504 + 77] = complex(0.0, np.nan)
    y[2, 700 + NULL + 504 + 2047] = np.inf
    y[3, 700:700 + NULL] = 0
    y[4] = 0
    model = M.HostModel(host, oracle)
    want = expected(model, y, 700)
    assert want["valid"].tolist() == [0, 0, 0, 1, 0, 1]
    P = want["signal_power"][3]
    assert want["noise_power"][3] == 0 and np.isfinite(want["weight"][3]) and abs(want["weight"][3] * P * 2.0 ** -40 - 1.0) < 2.0 ** -22
    run(ctx, y, 700, want)


def test_tii_on_the_air_and_the_bank(ctx, oracle, host):
    """four transmitters from the modulator's TII symbol under noise: the host model bit for bit, N inside the derived factor, and the
    group energies equal to a freshly reset TII bank's accumulator after one process of the same buffer"""
    import dabgpu
    import torch
    S = 196608
    rng = np.random.default_rng(9200)
    payload = torch.from_numpy(rng.integers(0, 256, (3, 75 * 384), dtype=np.uint8)).cuda()
    txs = [(11, 5, 1.0), (40, 17, 0.5), (0, 0, 1.0), (69, 23, 2.0)]
    lists, counts = dabgpu.tii_lists([txs] * 3)
    d_tx = torch.zeros((3 * S, 2), dtype=torch.float32, device="cuda")
    ctx.ofdm_modulate_frames_tii(1, payload, 3, d_tx, torch.from_numpy(lists.view(np.uint8)).cuda(), torch.from_numpy(counts).cuda())
    torch.cuda.synchronize()
    tx = d_tx.cpu().numpy().view(np.complex64).reshape(3, S)[:, :STRIDE]
    sigma = 0.5
    x = (tx + sigma * (rng.standard_normal(tx.shape) + 1j * rng.standard_normal(tx.shape))).astype(np.complex64)
    model = M.HostModel(host, oracle)
    want = expected(model, x, 0)
    run(ctx, x, 0, want)
    ratio = want["noise_power"] / (2.0 * sigma * sigma)
    assert (np.abs(ratio - M.tii_factor(4)) < 5.0 * M.relative_deviation(4)).all(), ratio
    bank = dabgpu.TiiBank(ctx, 3)
    bank.reset()
    bank.process(torch.from_numpy(x.view(np.float32)).cuda(), STRIDE, 0)
    acc, n = bank.read()
    bank.close()
    assert (n == 1).all() and np.array_equal(acc.reshape(3, 192).view(np.uint32), want["group_energy"].view(np.uint32))


def test_captured_call_replayed_on_new_samples(ctx, oracle, host, frames):
    import torch
    x, st, caller = frames
    model = M.HostModel(host, oracle)
    d_iq = torch.from_numpy(x[:3].view(np.float32).copy()).cuda()
    d_st = torch.from_numpy(st[:3].view(np.uint8).copy()).cuda()
    d_w = torch.zeros(3, dtype=torch.float32, device="cuda")
    d_n = torch.zeros(3, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctx.noise_estimate(d_iq, 3, STRIDE, 700, states=d_st, weight=d_w, noise_power=d_n, stream=side.cuda_stream)
    for lo in (0, 8):
        d_iq.copy_(torch.from_numpy(x[lo:lo + 3].view(np.float32).copy()))
        g.replay()
        torch.cuda.synchronize()
        want = expected(model, x[lo:lo + 3], 700, st[:3])
        assert np.array_equal(d_w.cpu().numpy().view(np.uint32), want["weight"].view(np.uint32)), lo
        assert np.array_equal(d_n.cpu().numpy().view(np.uint32), want["noise_power"].view(np.uint32)), lo


def test_host_form(ctx, oracle, host, frames):
    import dabgpu
    x, st, caller = frames
    model = M.HostModel(host, oracle)
    for k, fto, f in ((0, 0, 0.0), (3, 37, 1.5 / 2048), (9, -504, -1e-3), (10, 1543, 0.0)):
        rec = ctx.noise_estimate_host(x[k], 700, freq_offset=f, fine_time_offset=fto)
        exp, _ = model.estimate(x[k], 700 + fto, np.float32(f))
        assert rec.tobytes() == exp.tobytes(), (k, rec, exp)
    with pytest.raises(dabgpu.DabGpuError):
        ctx.noise_estimate_host(x[0][:700 + REACH - 1], 700)                                # the PRS leaves the samples
    with pytest.raises(dabgpu.DabGpuError):
        ctx.noise_estimate_host(x[0], 0, fine_time_offset=-1)
    for fto in (-505, 1544):                                                                # inside the samples, outside the synchroniser's range
        with pytest.raises(dabgpu.DabGpuError, match="fine_time_offset"):
            ctx.noise_estimate_host(x[0], 700, fine_time_offset=fto)
    assert ctx.noise_estimate_host(x[0][:700 + REACH], 700)["valid"] == 1
