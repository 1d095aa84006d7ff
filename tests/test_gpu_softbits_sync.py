"""-m gpu: dabgpu_ofdm_sync_demod_frames_soft -- synchronisation, positioned demodulation with the weighted soft bits, fine-frequency
update in one call -- on four receivers with different timing offsets and one that hears noise only.  It equals the synchroniser
followed by the batch call (dabgpu_ofdm_demod_frames_soft) on the frames shifted to where the records put them, the scale included:
the window of the frame power moves with the frame.  The records themselves are those of dabgpu_ofdm_sync_demod_frames (the policy
does not enter the frequency loop), and a receiver whose impulse-peak test fails keeps its rows and its scale."""
import numpy as np
import pytest

import softbit_cases as SC
import softbit_model as SM

pytestmark = pytest.mark.gpu
P = 700
STRIDE = P + 1544 + 196608
TOFFS = [0, 37, -81, 201]
NB = SC.NB_FRAME_BITS


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


def make_slices(rx):
    """receiver k hears frame k of the transmission with its first PRS sample at P + TOFFS[k] of the slice; the last receiver noise"""
    rng = np.random.default_rng(9310)
    s = np.zeros((len(TOFFS) + 1, STRIDE), np.complex64)
    for k, toff in enumerate(TOFFS):
        a = 2656 + k * 196608 + SC.CL.TIMING - (P + toff)
        s[k] = rx[a:a + STRIDE]
    s[-1] = (rng.standard_normal(STRIDE) + 1j * rng.standard_normal(STRIDE)).astype(np.complex64)
    return s


@pytest.mark.parametrize("layout,spb", [(0, 25), (0, 75), (1, 0), (1, 3)])
def test_sync_demod_soft_equals_sync_then_the_batch_call(ctx, oracle, tmp_path_factory, layout, spb):
    import dabgpu
    import torch
    rx = SC.received(oracle, tmp_path_factory.mktemp("softbits_sync_channel"))[0]
    slices = make_slices(rx)
    n = len(slices)
    soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0)
    sdt = np.dtype(dabgpu.SYNC_STATE_DTYPE)
    d_iq = torch.from_numpy(slices.view(np.float32).reshape(n, STRIDE, 2)).cuda()
    # the one call
    d_st = torch.from_numpy(np.zeros(n, sdt).view(np.uint8)).cuda()
    bits = torch.full((n, NB), 55, dtype=torch.int8, device="cuda")
    scale = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    total = torch.full((n,), -3.0, dtype=torch.float32, device="cuda")
    ctx.ofdm_sync_demod_frames_soft(d_iq, n, STRIDE, P, d_st, bits, soft, symbols_per_block=spb, bits_layout=layout, total_phase=total, soft_scale=scale)
    # the records of the call without a policy
    d_st0 = torch.from_numpy(np.zeros(n, sdt).view(np.uint8)).cuda()
    bits0 = torch.zeros((n, NB), dtype=torch.int8, device="cuda")
    ctx.ofdm_sync_demod_frames(d_iq, n, STRIDE, P, d_st0, bits0, symbols_per_block=spb, bits_layout=layout)
    # the synchroniser alone, then the batch call on the shifted frames
    d_st1 = torch.from_numpy(np.zeros(n, sdt).view(np.uint8)).cuda()
    ctx.ofdm_sync(d_iq[:, P:], n, STRIDE, d_st1)
    torch.cuda.synchronize()
    st, st0, st1 = (t.cpu().numpy().view(sdt) for t in (d_st, d_st0, d_st1))
    assert np.array_equal(d_st.cpu().numpy(), d_st0.cpu().numpy())
    assert st1["sync_valid"].tolist() == [1, 1, 1, 1, 0] and st1["fine_time_offset"][:4].tolist() == TOFFS
    assert np.array_equal(st["fine_time_offset"], st1["fine_time_offset"]) and np.array_equal(st["sync_valid"], st1["sync_valid"])
    valid = [k for k in range(n) if st1[k]["sync_valid"]]
    frames = np.stack([slices[k, P + st1[k]["fine_time_offset"]:P + st1[k]["fine_time_offset"] + 196608] for k in valid])
    freq = (st1["freq_coarse"] + st1["freq_fine"]).astype(np.float32)[valid]
    b1 = torch.zeros((len(valid), NB), dtype=torch.int8, device="cuda")
    s1 = torch.zeros((len(valid),), dtype=torch.float32, device="cuda")
    ctx.ofdm_demod_frames_soft(torch.from_numpy(frames.view(np.float32)).cuda(), dabgpu.IQ_FORMATS.index("raw_f32l"), len(valid), b1, soft,
                               freq_offset=torch.from_numpy(freq).cuda(), bits_layout=layout, soft_scale=s1)
    torch.cuda.synchronize()
    gb, gs, gt = bits.cpu().numpy(), scale.cpu().numpy(), total.cpu().numpy()
    assert np.array_equal(gb[valid], b1.cpu().numpy())
    assert np.array_equal(gs[valid].view(np.uint32), s1.cpu().numpy().view(np.uint32))
    # the scale is the model's over the window the record points at, not over the expected position
    exp_scale = SC.expected_scale(frames, 64.0)
    assert np.array_equal(gs[valid].view(np.uint32), exp_scale.view(np.uint32)) and (exp_scale > 0).all()
    at_expected = SC.expected_scale(np.stack([slices[k, P:P + 196608] for k in valid]), 64.0)
    assert not np.array_equal(at_expected.view(np.uint32)[1:], exp_scale.view(np.uint32)[1:])
    # weights, not the normalised bits; the same signs
    g0 = bits0.cpu().numpy()
    assert not np.array_equal(gb[0], g0[0]) and (gb[0].astype(int) * g0[0].astype(int) >= 0).all()
    # the receiver without a signal: rows and scale untouched
    assert (gb[4] == 55).all() and gs[4] == -1.0 and gt[4] == -3.0 and (gt[:4] != -3.0).all()
