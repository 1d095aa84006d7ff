"""-m gpu: the channel-state weighted soft bits on the device (dabgpu_ofdm_demod_frames_soft, DABGPU_SOFT_CSI) against the arithmetic
contract.  For every loader the scale the kernel reports equals the numpy model of csrc/softbit_csi_core.h over the frame's phase
reference window bit for bit, and the soft bits equal that model applied to the DQPSK view of the normalised call on the same input
(a view tests/test_gpu_ofdm.py pins to the oracle) -- in both layouts, with and without the display views, for every run length, into
a ring slot, and from a captured graph.  Frames whose power vanishes, overflows or is NaN are erased.  The normalised policy through
the new entry point is the old entry points byte for byte."""
import numpy as np
import pytest

import softbit_cases as SC
import softbit_model as SM

pytestmark = pytest.mark.gpu
NB = SC.NB_FRAME_BITS


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rx(oracle, tmp_path_factory):
    return SC.received(oracle, tmp_path_factory.mktemp("softbits_channel"))[0]


@pytest.fixture(scope="module", params=SC.FORMATS)
def case(request, ctx, rx, oracle):
    """per loader: the input on the device, the normalised call's soft bits and DQPSK view, and the model's expectation at level 64"""
    import dabgpu
    import torch
    fmt_name = request.param
    raw, dec = SC.capture_frames(rx, fmt_name)
    n = len(raw)
    d_raw = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
    fmt = dabgpu.IQ_FORMATS.index(fmt_name)
    bits = torch.zeros((n, NB), dtype=torch.int8, device="cuda")
    dq = torch.zeros((n, 75, 1536, 2), dtype=torch.float32, device="cuda")
    ctx.ofdm_demod_frames_raw(d_raw, fmt, n, bits, dqpsk=dq)
    torch.cuda.synchronize()
    dq = dq.cpu().numpy().view(np.complex64).reshape(n, 75, 1536)
    scales = SC.expected_scale(dec, 64.0)
    return dict(fmt=fmt, fmt_name=fmt_name, n=n, d_raw=d_raw, dec=dec, norm_bits=bits.cpu().numpy(), dq=dq, scales=scales,
                exp=SC.expected_bits(dq, scales, oracle.mapper()))


def run_soft(ctx, case, soft, layout=0, spb=0, views=False, stride=0, out=None):
    import torch
    n = case["n"]
    bits = out if out is not None else torch.full((n, NB), 55, dtype=torch.int8, device="cuda")
    scale = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    corr = torch.zeros((n, 76, 2), dtype=torch.float32, device="cuda")
    fft = torch.zeros((n, 77, 2048, 2), dtype=torch.float32, device="cuda") if views else None
    dq = torch.zeros((n, 75, 1536, 2), dtype=torch.float32, device="cuda") if views else None
    ctx.ofdm_demod_frames_soft(case["d_raw"], case["fmt"], n, bits, soft, cp_corr=corr, fft=fft, dqpsk=dq, symbols_per_block=spb,
                               bits_frame_stride=stride, bits_layout=layout, soft_scale=scale)
    torch.cuda.synchronize()
    return bits.cpu().numpy(), scale.cpu().numpy(), (None if dq is None else dq.cpu().numpy().view(np.complex64).reshape(n, 75, 1536))


def test_scale_and_soft_bits_equal_the_model(ctx, case):
    import dabgpu
    got, scale, _ = run_soft(ctx, case, dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0))
    assert np.array_equal(scale.view(np.uint32), case["scales"].view(np.uint32)), (scale, case["scales"])
    assert np.array_equal(scale.view(np.uint32), np.array([np.float32(dabgpu.soft_scale(f[504:2552], 64.0)) for f in case["dec"]]).view(np.uint32))
    assert np.array_equal(got, case["exp"])
    assert got.min() >= -127
    # the plain frames carry weights: not the normalised bits, yet the same signs wherever both are non-zero
    plain = got[0].astype(int) * case["norm_bits"][0].astype(int)
    assert (plain >= 0).all() and not np.array_equal(got[0], case["norm_bits"][0]) and len(np.unique(got[0])) > 100
    if case["fmt_name"] == "raw_f32l":
        # overflowing power, NaN inside the window, vanishing power: erased.  2^-70: a scale beyond 2^120 on products 2^-140 times
        # the plain frame's, still soft bits with the signs of the normalised ones.  NaN outside the window: the two symbols that see it
        assert case["scales"][0] > 0 and case["scales"][1] > 2.0 ** 120 and not case["scales"][[2, 3, 5]].any() and case["scales"][4] > 0
        assert not got[[2, 3, 5]].any()
        assert got[1].any() and (got[1].astype(int) * case["norm_bits"][1].astype(int) >= 0).all()
        sym = got[4].reshape(75, 3072)
        assert not sym[38:40].any() and all(sym[s].any() for s in range(75) if s not in (38, 39))
    elif case["fmt_name"] != "raw_u8":
        assert case["scales"][3] == 0 and not got[3].any()                 # a frame of zeros: zero power


def test_another_level_scales_the_same_products(ctx, case, oracle):
    import dabgpu
    level = 21.5
    got, scale, _ = run_soft(ctx, case, dabgpu.SoftCfg(dabgpu.SOFT_CSI, level))
    exp_scale = SC.expected_scale(case["dec"], level)
    assert np.array_equal(scale.view(np.uint32), exp_scale.view(np.uint32))
    assert np.array_equal(got[0], SM.frame_bits(case["dq"][0], oracle.mapper(), exp_scale[0]))


def test_class_order_and_views(ctx, case):
    import dabgpu
    soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0)
    P = dabgpu.classed_to_natural_index()
    got, scale, _ = run_soft(ctx, case, soft, layout=dabgpu.BITS_MSC_CLASSED)
    assert np.array_equal(got[:, P], case["exp"]) and np.array_equal(scale.view(np.uint32), case["scales"].view(np.uint32))
    got, scale, dq = run_soft(ctx, case, soft, views=True)
    assert np.array_equal(got, case["exp"]) and np.array_equal(scale.view(np.uint32), case["scales"].view(np.uint32))
    assert np.array_equal(dq.view(np.uint32), case["dq"].view(np.uint32))   # the view is the normalised call's
    with pytest.raises(dabgpu.DabGpuError):
        run_soft(ctx, case, soft, layout=dabgpu.BITS_MSC_CLASSED, views=True)


@pytest.mark.parametrize("layout", [0, 1])
def test_every_run_length_gives_identical_bytes(ctx, case, layout):
    import dabgpu
    soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0)
    ref, ref_scale, _ = run_soft(ctx, case, soft, layout=layout, spb=25)
    for spb in (1, 3, 38, 75, 0):
        got, scale, _ = run_soft(ctx, case, soft, layout=layout, spb=spb)
        assert np.array_equal(got, ref) and np.array_equal(scale.view(np.uint32), ref_scale.view(np.uint32)), spb


def test_policy_normalised_is_the_old_entry_points(ctx, case):
    import dabgpu
    import torch
    soft = dabgpu.SoftCfg()
    assert soft.policy == dabgpu.SOFT_NORMALISED and soft.level == 64.0 and dabgpu.soft_cfg_default().level == 64.0
    got, scale, dq = run_soft(ctx, case, soft, views=True)
    assert np.array_equal(got, case["norm_bits"]) and np.array_equal(dq.view(np.uint32), case["dq"].view(np.uint32))
    assert (scale == -1.0).all()                                            # not written
    n = case["n"]
    old = torch.zeros((n, NB), dtype=torch.int8, device="cuda")
    ctx.ofdm_demod_frames_history(case["d_raw"], case["fmt"], n, old, bits_layout=dabgpu.BITS_MSC_CLASSED)
    got, _, _ = run_soft(ctx, case, soft, layout=dabgpu.BITS_MSC_CLASSED)
    assert np.array_equal(got, old.cpu().numpy())


def test_refusals(ctx, case):
    import dabgpu
    for bad in (dabgpu.SoftCfg(dabgpu.SOFT_CSI, 0.5), dabgpu.SoftCfg(dabgpu.SOFT_CSI, 128.0), dabgpu.SoftCfg(dabgpu.SOFT_CSI, float("nan")),
                dabgpu.SoftCfg(2, 64.0), dabgpu.SoftCfg(dabgpu.SOFT_NORMALISED, 0.0)):
        with pytest.raises(dabgpu.DabGpuError):
            run_soft(ctx, case, bad)


def test_ring_slot_stride(ctx, case):
    import dabgpu
    import torch
    n, H, slot = case["n"], 3, 2
    ring = torch.full((n, H, NB), 77, dtype=torch.int8, device="cuda")
    got, _, _ = run_soft(ctx, case, dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0), stride=H * NB, out=ring[:, slot])
    ring = ring.cpu().numpy()
    assert np.array_equal(ring[:, slot], case["exp"]) and (ring[:, :slot] == 77).all()


def test_graph_capture_and_two_replays(ctx, case):
    import dabgpu
    import torch
    n = case["n"]
    soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0)
    bits = torch.zeros((n, NB), dtype=torch.int8, device="cuda")
    scale = torch.zeros((n,), dtype=torch.float32, device="cuda")
    corr = torch.zeros((n, 76, 2), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctx.ofdm_demod_frames_soft(case["d_raw"], case["fmt"], n, bits, soft, cp_corr=corr, symbols_per_block=25, soft_scale=scale)
    torch.cuda.synchronize()
    for _ in range(2):
        bits.fill_(9); scale.fill_(-3.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits.cpu().numpy(), case["exp"])
        assert np.array_equal(scale.cpu().numpy().view(np.uint32), case["scales"].view(np.uint32))
