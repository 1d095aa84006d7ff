"""-m gpu: TII on the device (include/dabgpu.h, "TII").  The modulator's TII symbol against the host composition as bit patterns, with
everything outside the NULL periods equal to the entry point without TII; the detector against the float32 host model of
tests/tii_model.py (oracle PLL and transform around csrc/tii_core.h) bit for bit; every (main id, sub id) detected; the whole chain
modulator -> channel -> synchroniser and demodulator -> detector on the device; a captured call replayed.

A noise floor everywhere: the decision compares a comb with the floor N of the spectrum, and a signal without noise has none but the
float32 rounding of the transforms, which is not flat (on the CPU the host model reports the combs 8 and 16 sub ids away from a
transmitter on such input).  "Clean" below therefore means one transmitter, no echo, no offset, white noise 30 dB under the signal.  An
empty group of an active comb reaches threshold * N with probability 3e-3 after 2 frames (it is one Gamma(16) draw against 2.16 x 12.9),
which would add a fifth bit to about 1 % of 1680 masks; after 6 frames the level is 6.5 standard deviations above such a group."""
import numpy as np
import pytest

import signal_bank_cases as SB
import tii_model as M

pytestmark = pytest.mark.gpu

S, NULL, PERIOD = 196608, 2656, 2552
PAYLOAD = 75 * 384


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return M.build_host_model(tmp_path_factory.mktemp("tii_host_model"))


def f32_null_period(oracle, prs, txs):
    """the host composition of the NULL period in the modulator's arithmetic: float32 sums in list order, the oracle's inverse transform"""
    z = np.zeros(2048, np.complex64)
    for p, c, amp in txs:
        ks = M.carriers(p, c)
        for q, k in enumerate(ks):
            ph = prs[ks[q & ~1] % 2048]
            re = np.float32(z[k % 2048].real) + np.float32(amp) * np.float32(ph.real)
            im = np.float32(z[k % 2048].imag) + np.float32(amp) * np.float32(ph.imag)
            z[k % 2048] = np.complex64(complex(re, im))
    x = oracle.fft_n(z, inverse=True)
    return np.concatenate([x[-608:], x])


def u8_pairs(x, scale):
    def q(v):
        v = (v.astype(np.float32) * np.float32(scale)).astype(np.float32) + np.float32(127.5)
        return np.clip(v, np.float32(0.0), np.float32(255.0)).astype(np.uint8)
    return np.stack([q(x.real), q(x.imag)], axis=-1).reshape(-1)


TXS = [[], [(11, 5, 1.0)], [(0, 0, 1.0), (69, 23, 0.5), (40, 17, 2.0), (33, 17, -0.75)]]


@pytest.mark.parametrize("fmt_name", ["raw_f32l", "raw_u8"])
@pytest.mark.parametrize("freq", [0.0, 3.05 / 2048])
def test_modulator_null_symbol(ctx, oracle, fmt_name, freq):
    import dabgpu
    import torch
    fmt = dabgpu.IQ_FORMATS.index(fmt_name)
    sb = 8 if fmt_name == "raw_f32l" else 2
    rng = np.random.default_rng(4100)
    payload = torch.from_numpy(rng.integers(0, 256, (3, PAYLOAD), dtype=np.uint8)).cuda()
    lists, counts = dabgpu.tii_lists(TXS)
    d_l, d_c = torch.from_numpy(lists.view(np.uint8)).cuda(), torch.from_numpy(counts).cuda()
    G = 4096
    bufs = []
    for tii in (False, True):
        buf = torch.full((G + 3 * S * sb + G,), 0xA5, dtype=torch.uint8, device="cuda")
        out = buf[G:G + 3 * S * sb]
        if tii:
            ctx.ofdm_modulate_frames_tii(1, payload, 3, out, d_l, d_c, out_format=fmt, freq_norm=freq)
        else:
            ctx.ofdm_modulate_frames(1, payload, 3, out, out_format=fmt, freq_norm=freq)
        torch.cuda.synchronize()
        b = buf.cpu().numpy()
        assert (b[:G] == 0xA5).all() and (b[-G:] == 0xA5).all(), "guard bytes written"
        bufs.append(b[G:-G].reshape(3, S * sb))
    old, new = bufs
    assert np.array_equal(old[0], new[0]), "a frame without transmitters differs from dabgpu_ofdm_modulate_frames"
    assert np.array_equal(old[:, NULL * sb:], new[:, NULL * sb:]), "samples outside the NULL periods differ"
    prs = oracle.prs_fft()
    scale = np.float32(np.float32(np.float32(1.0) / np.float32(1536.0)) * np.float32(4.0)) * np.float32(127.5)
    for f in (1, 2):
        x = f32_null_period(oracle, prs, TXS[f])
        if freq != 0.0:
            x = oracle.apply_pll(x, np.float32(freq), 0.0)
        exp = x.view(np.uint8) if sb == 8 else u8_pairs(x, scale)
        assert np.array_equal(new[f, :NULL * sb], exp), f"frame {f}: NULL period differs from the host composition"
        assert not np.array_equal(new[f, :NULL * sb], old[f, :NULL * sb])
    # all counts 0: the old entry point's output bit for bit
    buf = torch.zeros(3 * S * sb, dtype=torch.uint8, device="cuda")
    ctx.ofdm_modulate_frames_tii(1, payload, 3, buf, d_l, torch.zeros(3, dtype=torch.uint8, device="cuda"), out_format=fmt, freq_norm=freq)
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().reshape(3, -1), old)


def test_modulator_refusals(ctx, oracle):
    import dabgpu
    payload = np.zeros((1, PAYLOAD), np.uint8)
    for bad, text in (([[(70, 0, 1.0)]], "main id 70"), ([[(0, 24, 1.0)]], "sub id 24"), ([[(1, 1, 1.0)] * 5], "5 transmitters"),
                      ([[(1, 1, float("inf"))]], "not finite")):
        with pytest.raises(dabgpu.DabGpuError) as err:
            ctx.ofdm_modulate_frames_tii_host(1, payload, 1, bad)
        assert text in str(err.value)
    for mode in (2, 3, 4):
        n = dabgpu.ofdm_params(mode)
        pl = np.zeros((1, (n["nb_frame_symbols"] - 1) * n["nb_data_carriers"] // 4), np.uint8)
        with pytest.raises(dabgpu.DabGpuError) as err:
            ctx.ofdm_modulate_frames_tii_host(mode, pl, 1, [[(1, 1, 1.0)]])
        assert "mode I only" in str(err.value)
    # the host form with a valid list: the NULL period is the host composition as bit patterns, the rest the form's without TII
    out = ctx.ofdm_modulate_frames_tii_host(1, payload, 1, [[(11, 5, 1.0)]])
    assert out.shape == (1, S) and out.dtype == np.complex64
    exp = f32_null_period(oracle, oracle.prs_fft(), [(11, 5, 1.0)])
    assert np.array_equal(out[0, :NULL].view(np.uint32), exp.view(np.uint32))
    plain = ctx.ofdm_modulate_frames_host(1, payload, 1)
    assert np.array_equal(out[0, NULL:].view(np.uint32), plain[0, NULL:].view(np.uint32)) and not plain[0, :NULL].any()


def test_detector_every_pair(ctx, oracle):
    """1680 receivers in one call, one (p, c) each, no echo and no offset, white noise 30 dB under the signal, 6 frames"""
    import dabgpu
    import torch
    prs = oracle.prs_fft()
    Z = np.zeros((1680, 2048), np.complex128)
    for p in range(70):
        for c in range(24):
            Z[24 * p + c] = M.null_spectrum(prs, [(p, c, 1.0)])
    X = np.fft.ifft(Z, axis=1) * 2048
    X = np.concatenate([X[:, -608:], X], axis=1).astype(np.complex64)
    d_x = torch.from_numpy(X.view(np.float32)).cuda()
    sigma = float(np.sqrt(32.0 / 1000.0 / 2.0))                 # 32 carriers of power 1 per sample, 30 dB, per component
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1680)
    bank = dabgpu.TiiBank(ctx, 1680)
    rdt = np.dtype(dabgpu.TII_RECORD_DTYPE)
    res = torch.zeros(1680 * 24 * rdt.itemsize, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1680, dtype=torch.int32, device="cuda")
    for f in range(6):
        rx = d_x + sigma * torch.randn(d_x.shape, generator=gen, device="cuda", dtype=torch.float32)
        bank.process(rx, NULL, 0, decide=(f == 5), results=res, counts=cnt)
    torch.cuda.synchronize()
    acc, frames = bank.read()
    assert (frames == 6).all()
    assert (cnt.cpu().numpy() == 1).all(), np.nonzero(cnt.cpu().numpy() != 1)[0][:20]
    rec = res.cpu().numpy().view(rdt).reshape(1680, 24)[:, 0]
    k = np.arange(1680)
    assert np.array_equal(rec["sub_id"], k % 24) and np.array_equal(rec["main_id"], k // 24)
    assert np.array_equal(rec["mask"], np.array(M.TABLE, np.uint32)[k // 24])
    bank.close()


def loop_slices(oracle, n_frames, seed):
    """5 receivers x n_frames slices: three transmitters (two on comb 17 with different main ids) behind two paths, an offset of 3.05
    carrier spacings, a timing offset and noise, TII in every frame; the receivers' records as a synchroniser would leave them"""
    prs = oracle.prs_fft()
    txs = [(11, 5, 1.0), (40, 17, 0.5), (33, 17, 0.7)]
    x = M.null_period(prs, txs)
    rng = np.random.default_rng(seed)
    stride, off = 6000, 700
    fto = [37, -120, 0, 1500, 64]
    cfo = 3.05 / 2048
    slices = np.zeros((n_frames, 5, stride), np.complex64)
    for f in range(n_frames):
        for k in range(5):
            s = np.zeros(stride, np.complex128)
            a = off + fto[k]
            s[a:a + NULL] += x
            s[a + 200:a + 200 + NULL] += 0.5 * x
            s *= np.exp(2j * np.pi * cfo * np.arange(stride))
            s += 1.5 * (rng.standard_normal(stride) + 1j * rng.standard_normal(stride))
            slices[f, k] = s
    return slices, stride, off, fto, cfo, txs


def test_detector_equals_host_model(ctx, oracle, host):
    import dabgpu
    import torch
    F = 3
    slices, stride, off, fto, cfo, txs = loop_slices(oracle, F, 5100)
    sdt = np.dtype(dabgpu.SYNC_STATE_DTYPE)
    st = np.zeros(5, sdt)
    st["freq_coarse"] = np.float32(-3.0 / 2048)
    st["freq_fine"] = np.float32(-0.05 / 2048)
    st["fine_time_offset"] = fto
    st["sync_valid"] = [1, 1, 0, 1, 1]
    caller = np.full(5, np.nan, np.float32)
    caller[4] = np.float32(-3.04 / 2048)                          # receiver 4: a caller's offset instead of its record's
    d_st = torch.from_numpy(st.view(np.uint8)).cuda()
    d_fq = torch.from_numpy(caller).cuda()
    bank = dabgpu.TiiBank(ctx, 5)
    rdt = np.dtype(dabgpu.TII_RECORD_DTYPE)
    res = torch.full((5 * 24 * rdt.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")
    cnt = torch.full((5,), -7, dtype=torch.int32, device="cuda")
    models = [M.HostModel(host, oracle, bank.threshold) for _ in range(5)]
    for f in range(F):
        d_iq = torch.from_numpy(slices[f].view(np.float32)).cuda()
        bank.process(d_iq, stride, off, states=d_st, freq_offset=d_fq, decide=True, results=res, counts=cnt)
        acc, frames = bank.read()
        got = res.cpu().numpy().view(rdt).reshape(5, 24)
        n = cnt.cpu().numpy()
        for k in range(5):
            if k == 2:                                          # sync_valid = 0: nothing of it is touched
                assert frames[k] == 0 and not acc[k].any() and n[k] == -7 and (got[k].view(np.uint8) == 0xEE).all()
                continue
            freq = caller[k] if k == 4 else np.float32(st["freq_coarse"][k]) + np.float32(st["freq_fine"][k])
            models[k].process(slices[f, k], off + fto[k], freq)
            assert frames[k] == f + 1
            assert np.array_equal(acc[k].reshape(-1).view(np.uint32), models[k].acc.view(np.uint32)), (f, k)
            exp = models[k].decide()
            assert n[k] == len(exp) and np.array_equal(got[k, :n[k]].view(np.uint8), exp.view(np.uint8)), (f, k, got[k, :n[k]], exp)
    # after three frames: the two clean records and the union of the two main ids on comb 17
    union = M.TABLE[40] | M.TABLE[33]
    for k in (0, 1, 3, 4):
        assert M.records_as_tuples(got[k, :n[k]]) == [(5, 11, M.TABLE[11]), (17, -1, union)], (k, got[k, :n[k]])
    bank.reset()
    acc, frames = bank.read()
    assert not acc.any() and not frames.any()
    bank.close()


def test_host_form_and_checks(ctx, oracle, host):
    import dabgpu
    slices, stride, off, fto, cfo, txs = loop_slices(oracle, 2, 5200)
    bank = dabgpu.TiiBank(ctx, 1)
    m = M.HostModel(host, oracle, bank.threshold)
    f = np.float32(-3.05 / 2048)
    for j in range(2):
        rec = bank.process_host(slices[j, 0], off, freq_offset=f, fine_time_offset=fto[0], decide=(j == 1))
        m.process(slices[j, 0], off + fto[0], f)
    assert np.array_equal(rec.view(np.uint8), m.decide().view(np.uint8))
    acc, frames = bank.read()
    assert frames[0] == 2 and np.array_equal(acc.reshape(-1).view(np.uint32), m.acc.view(np.uint32))
    with pytest.raises(dabgpu.DabGpuError):
        bank.process_host(slices[0, 0][:off + 608 + 2047], off)             # the window leaves the samples
    with pytest.raises(dabgpu.DabGpuError):
        bank.process_host(slices[0, 0], 0, fine_time_offset=-609)
    import torch
    d = torch.zeros((stride, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(dabgpu.DabGpuError):
        bank.process(d, stride, stride - NULL + 1)                          # the NULL period leaves the slice
    with pytest.raises(dabgpu.DabGpuError):
        bank.process(d, stride, 0, decide=True)                             # a decision without results
    with pytest.raises(dabgpu.DabGpuError):
        dabgpu.TiiBank(ctx, 0)
    with pytest.raises(dabgpu.DabGpuError):
        dabgpu.TiiBank(ctx, 1, threshold=0.5)
    bank.close()


def test_handle_closes_twice_and_goes_with_its_last_reference(ctx):
    import dabgpu
    SB.handle_lifecycle(lambda: dabgpu.TiiBank(ctx, 2))


def test_whole_chain_on_the_device(ctx):
    """modulator with TII -> channel (offset of 3.05 carrier spacings, 20 samples early, noise) -> synchroniser + demodulator -> detector
    with the records the synchroniser left.  Early, not late: a late signal puts the end of the NULL period into the 2048 samples the
    synchroniser correlates, and what it reads there is then no longer the same with and without TII.

    The detector is fed from DABGPU_TII_SETTLE_FRAMES frames after the acquisition on: the record of the first frame is 0.45 carrier
    spacings off (tests/test_tii_closed_loop.py shows it on the CPU: -2.60 for -3.05), which is what put (4, 11), (6, 11) and (18, 40)
    beside the transmitters when every frame was fed."""
    import dabgpu
    import torch
    import channel_model as CM
    F, P = 6, 3200
    stride = P + 1544 + 76 * PERIOD
    rng = np.random.default_rng(6100)
    payload = torch.from_numpy(rng.integers(0, 256, (F, PAYLOAD), dtype=np.uint8)).cuda()
    txs = [(11, 5, 1.0), (40, 17, 0.5)]
    lists, counts = dabgpu.tii_lists([txs] * F)
    d_l, d_c = torch.from_numpy(lists.view(np.uint8)).cuda(), torch.from_numpy(counts).cuda()
    n_out = F * S + 4096
    sdt = np.dtype(dabgpu.SYNC_STATE_DTYPE)
    rdt = np.dtype(dabgpu.TII_RECORD_DTYPE)
    bits = {}
    for tii in (False, True):
        d_tx = torch.zeros((F * S, 2), dtype=torch.float32, device="cuda")
        if tii:
            ctx.ofdm_modulate_frames_tii(1, payload, F, d_tx, d_l, d_c)
        else:
            ctx.ofdm_modulate_frames(1, payload, F, d_tx)
        # power of a frame: 1536 carriers of power 1 through an unnormalised transform of 2048 points = 1536 per sample; 20 dB
        prm = CM.params_dict(taps=[(0, 1.0, 0.0)], freq_q64=int(round(3.05 / 2048 * 2 ** 64)), start=-20, seed=0x711,
                             noise_sigma=float(np.sqrt(1536.0 / 100.0 / 2.0)))
        ch = dabgpu.Channel(ctx, [CM.to_struct(prm, dabgpu.ChannelStream)])
        d_rx = torch.zeros((n_out, 2), dtype=torch.float32, device="cuda")
        ch.apply(d_tx, F * S, n_out, d_rx)
        d_st = torch.zeros(sdt.itemsize, dtype=torch.uint8, device="cuda")
        d_bits = torch.zeros((F - 1, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
        bank = dabgpu.TiiBank(ctx, 1)
        res = torch.zeros(24 * rdt.itemsize, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        nets = []
        for j in range(1, F):                                   # frame j's PRS is expected P samples into its slice
            a = NULL + j * S - P
            sl = d_rx[a:a + stride]
            ctx.ofdm_sync_demod_frames(sl, 1, stride, P, d_st, d_bits[j - 1])
            st = d_st.cpu().numpy().view(sdt)[0]
            nets.append((float(st["freq_coarse"]) + float(st["freq_fine"])) * 2048)
            if j - 1 >= dabgpu.TII_SETTLE_FRAMES:
                bank.process(sl, stride, P - NULL, states=d_st, decide=(j == F - 1), results=res, counts=cnt)
        torch.cuda.synchronize()
        st = d_st.cpu().numpy().view(sdt)[0]
        assert st["sync_valid"] == 1 and st["fine_time_offset"] == -20
        bits[tii] = d_bits.cpu().numpy()
        got = res.cpu().numpy().view(rdt)[:int(cnt.cpu().numpy()[0])]
        print("whole chain, TII", tii, "net offsets (carrier spacings):", nets, "records:", got)
        assert 0.2 < abs(nets[0] + 3.05) <= 0.52 and all(abs(n + 3.05) < 0.06 for n in nets[1:]), nets
        assert M.records_as_tuples(got) == ([(5, 11, M.TABLE[11]), (17, 40, M.TABLE[40])] if tii else []), got
        acc, frames = bank.read()
        assert frames[0] == F - 1 - dabgpu.TII_SETTLE_FRAMES
        bank.close(); ch.close()
    assert np.array_equal(bits[False], bits[True]), "the NULL symbol's content changed the soft bits"


def test_captured_call_continues_the_accumulator(ctx, oracle, host):
    import dabgpu
    import torch
    slices, stride, off, fto, cfo, txs = loop_slices(oracle, 2, 5300)
    bank = dabgpu.TiiBank(ctx, 5)
    rdt = np.dtype(dabgpu.TII_RECORD_DTYPE)
    res = torch.zeros(5 * 24 * rdt.itemsize, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(5, dtype=torch.int32, device="cuda")
    fq = torch.full((5,), float(np.float32(-3.05 / 2048)), dtype=torch.float32, device="cuda")
    d_iq = torch.from_numpy(slices[0].view(np.float32)).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        bank.process(d_iq, stride, off + 37, freq_offset=fq, decide=True, results=res, counts=cnt, stream=side.cuda_stream)
    g.replay()                                                  # (capturing enqueued nothing)
    d_iq.copy_(torch.from_numpy(slices[1].view(np.float32)))
    g.replay()
    torch.cuda.synchronize()
    acc, frames = bank.read()
    assert (frames == 2).all()
    for k in range(5):
        m = M.HostModel(host, oracle, bank.threshold)
        for f in range(2):
            m.process(slices[f, k], off + 37, np.float32(-3.05 / 2048))
        assert np.array_equal(acc[k].reshape(-1).view(np.uint32), m.acc.view(np.uint32)), k
        n = int(cnt.cpu().numpy()[k])
        assert np.array_equal(res.cpu().numpy().view(rdt).reshape(5, 24)[k, :n].view(np.uint8), m.decide().view(np.uint8))
    bank.close()
