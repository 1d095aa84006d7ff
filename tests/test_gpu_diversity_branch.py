"""-m gpu: dabgpu_ofdm_sync_demod_frames_branch -- a synchronised diversity branch: dabgpu_ofdm_sync_demod_frames_soft in the natural
layout that also writes the receivers' DQPSK products.  Two streams, one with a timing offset and one that hears noise only.  Bits,
records, scale, total phase and cyclic-prefix correlations equal dabgpu_ofdm_sync_demod_frames_soft; the products equal
dabgpu_ofdm_demod_frames_soft (display views) on the frame shifted to where the record puts it; the receiver whose impulse-peak test
fails keeps every row, its products included, so that its branch is dead through d_sync and nothing stale is combined."""
import numpy as np
import pytest

import diversity_model as DM
import softbit_cases as SC

pytestmark = pytest.mark.gpu
P = 700
STRIDE = P + 1544 + 196608
TOFF = 37
NB = SC.NB_FRAME_BITS


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("spb", [0, 25, 75])
def test_branch_call_equals_the_soft_call_and_writes_the_products(ctx, oracle, tmp_path_factory, spb):
    import dabgpu
    import torch
    rx = SC.received(oracle, tmp_path_factory.mktemp("diversity_branch_channel"))[0]
    rng = np.random.default_rng(9610)
    slices = np.zeros((2, STRIDE), np.complex64)
    a = 2656 + 196608 + SC.CL.TIMING - (P + TOFF)
    slices[0] = rx[a:a + STRIDE]
    slices[1] = (rng.standard_normal(STRIDE) + 1j * rng.standard_normal(STRIDE)).astype(np.complex64)
    n = 2
    soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0)
    sdt = np.dtype(dabgpu.SYNC_STATE_DTYPE)
    d_iq = torch.from_numpy(slices.view(np.float32).reshape(n, STRIDE, 2)).cuda()

    def outputs():
        return dict(st=torch.from_numpy(np.zeros(n, sdt).view(np.uint8)).cuda(), bits=torch.full((n, NB), 55, dtype=torch.int8, device="cuda"),
                    scale=torch.full((n,), -1.0, dtype=torch.float32, device="cuda"), total=torch.full((n,), -3.0, dtype=torch.float32, device="cuda"),
                    corr=torch.full((n, 76, 2), -5.0, dtype=torch.float32, device="cuda"))

    A, B = outputs(), outputs()
    dq = torch.full((n, 75, 1536, 2), -7.0, dtype=torch.float32, device="cuda")
    ctx.ofdm_sync_demod_frames_branch(d_iq, n, STRIDE, P, A["st"], A["bits"], soft, dq, cp_corr=A["corr"], symbols_per_block=spb, total_phase=A["total"],
                                      soft_scale=A["scale"])
    ctx.ofdm_sync_demod_frames_soft(d_iq, n, STRIDE, P, B["st"], B["bits"], soft, cp_corr=B["corr"], symbols_per_block=spb, total_phase=B["total"],
                                    soft_scale=B["scale"])
    d_st1 = torch.from_numpy(np.zeros(n, sdt).view(np.uint8)).cuda()
    ctx.ofdm_sync(d_iq[:, P:], n, STRIDE, d_st1)
    torch.cuda.synchronize()
    for name in ("st", "bits", "scale", "total", "corr"):
        assert np.array_equal(A[name].cpu().numpy().view(np.uint8), B[name].cpu().numpy().view(np.uint8)), name
    st, st1 = A["st"].cpu().numpy().view(sdt), d_st1.cpu().numpy().view(sdt)
    assert st["sync_valid"].tolist() == [1, 0] and st["fine_time_offset"][0] == TOFF
    # the products: the batch call with the display views on the shifted frame, at the offset the synchroniser found
    frame = slices[0, P + TOFF:P + TOFF + 196608][None]
    freq = np.array([st1["freq_coarse"][0] + st1["freq_fine"][0]], np.float32)
    b1 = torch.zeros((1, NB), dtype=torch.int8, device="cuda")
    dq1 = torch.zeros((1, 75, 1536, 2), dtype=torch.float32, device="cuda")
    ctx.ofdm_demod_frames_soft(torch.from_numpy(frame.view(np.float32)).cuda(), dabgpu.IQ_FORMATS.index("raw_f32l"), 1, b1, soft,
                               freq_offset=torch.from_numpy(freq).cuda(), dqpsk=dq1)
    torch.cuda.synchronize()
    got_dq = dq.cpu().numpy()
    assert np.array_equal(got_dq[0].view(np.uint32), dq1.cpu().numpy()[0].view(np.uint32)) and np.array_equal(A["bits"].cpu().numpy()[0], b1.cpu().numpy()[0])
    # the receiver without a signal: every row untouched, the products too
    assert (got_dq[1] == -7.0).all() and (A["bits"].cpu().numpy()[1] == 55).all() and A["scale"].cpu().numpy()[1] == -1.0
    assert A["total"].cpu().numpy()[1] == -3.0 and A["total"].cpu().numpy()[0] != -3.0
    if spb == 0:
        # ... and the pair is what the combiner takes: branch 0 alone gives the call's own bits, the dead receiver an erased frame
        out = torch.full((n, NB), 9, dtype=torch.int8, device="cuda")
        mask = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        ctx.diversity_combine([(dq, A["scale"], None, A["st"])], n, out, live_mask=mask)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy()[0], b1.cpu().numpy()[0]) and not out.cpu().numpy()[1].any() and mask.cpu().numpy().tolist() == [1, 0]
    with pytest.raises(dabgpu.DabGpuError, match="d_dqpsk"):
        ctx.ofdm_sync_demod_frames_branch(d_iq, n, STRIDE, P, A["st"], A["bits"], soft, None)
    assert DM.NB_FRAME_BITS == NB
