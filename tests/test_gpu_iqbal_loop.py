"""-m gpu: the closed loop of tests/iqbal_loop.py through the device banks: the 8.192 MS/s capture of the host combiner (the wanted block at
+856 kHz, one neighbour 30 dB up at -856 kHz) -> dabgpu.IqBalance with the FIXED stream of dabgpu.iqbal_impairment (the front end) ->
dabgpu.IqBalance with the library's default TRACK stream, primed (MEASURE over the capture's whole tiles, seek back, APPLY in place) ->
dabgpu.Channeliser split -> dabgpu_ofdm_sync_demod_frames -> dabgpu_decode_frames_layout.  The impaired and the corrected capture and the
record equal the host model's bit for bit; the receive outputs equal the CPU oracle chain's byte for byte; every FIB CRC, FIB body and
sub-channel byte arrives with fine time offset 37 in every frame, where the uncorrected capture loses the block.  The operating point was
chosen on the CPU: tests/test_iqbal_closed_loop.py."""
import numpy as np
import pytest

import channel_loop as CL
import channel_model as CHM
import channelise_model as CM
import iqbal_loop as QL
import iqbal_model as IM
from test_gpu_channelise_loop import receive_on_device

pytestmark = pytest.mark.gpu


def test_front_end_then_corrector_through_the_device_banks(oracle, tmp_path):
    import dabgpu
    import torch
    hosts = CHM.build_host_model(tmp_path), CM.build_host_model(tmp_path), IM.build_host_model(tmp_path)
    ctx = dabgpu.Context(0)
    fib, pay, nb, rows = QL.block_rows(oracle, hosts[0], CL.SNR_DB)
    Fh = CM.host_design(hosts[1], QL.D)
    wide = CM.host_combine(hosts[1], QL.channels(QL.ADJACENT_DB), 1, Fh, rows, 0, 0, QL.N_WIDE, False)[0]
    n = wide.size
    tiles = n // IM.TILE * IM.TILE
    # the front end: the simulator's impairment
    S = dabgpu.iqbal_impairment(QL.GAIN_DB, QL.PHASE_DEG, QL.DC)
    assert bytes(S)[8:32] == bytes(IM.to_struct(QL.impairment()))[8:32]       # the six coefficients are the model's
    tuner = dabgpu.IqBalance(ctx, [S], IM.TILE)
    d_wide = torch.from_numpy(wide.view(np.float32).reshape(n, 2).copy()).cuda()
    tuner.apply(d_wide, n, d_wide)
    torch.cuda.synchronize()
    impaired = d_wide.cpu().numpy().view(np.complex64).reshape(-1)
    want = QL.front_end(hosts[2], wide, True)
    assert np.array_equal(impaired.view(np.uint32), want.view(np.uint32)), "impaired capture != host model"
    # uncorrected, the block is lost: the split finds the neighbour's image on it
    cb = dabgpu.Channeliser(ctx, [CM.to_struct(c, dabgpu.ChanneliserChannel) for c in QL.wanted_channel()], 1, dabgpu.channeliser_design(QL.D))
    d_back = torch.zeros((1, CL.N_OUT, 2), dtype=torch.float32, device="cuda")
    cb.split(d_wide, n, CL.N_OUT, d_back, out_stride_bytes=CL.N_OUT * 8)
    torch.cuda.synchronize()
    raw = d_back.cpu().numpy().view(np.complex64).reshape(-1)
    with pytest.raises(AssertionError):
        receive_on_device(oracle, ctx, raw, fib[0], pay[0], nb, against_oracle=False)
    # prime + correct, in place
    bal = dabgpu.IqBalance(ctx, [dabgpu.iqbal_stream()], tiles)
    bal.apply(d_wide, tiles, flags=dabgpu.IQBAL_MEASURE)
    bal.seek(0)
    bal.apply(d_wide, n, d_wide)
    torch.cuda.synchronize()
    corrected = d_wide.cpu().numpy().view(np.complex64).reshape(-1)
    want, rec = QL.correct(hosts[2], impaired)
    assert np.array_equal(corrected.view(np.uint32), want.view(np.uint32)), "corrected capture != host model"
    state = bal.read_state()
    assert state.tobytes() == rec.tobytes() and state["valid"][0] == 1 and state["tiles_used"][0] == tiles // IM.TILE
    cb.seek(0)
    cb.split(d_wide, n, CL.N_OUT, d_back, out_stride_bytes=CL.N_OUT * 8)
    torch.cuda.synchronize()
    back = d_back.cpu().numpy().view(np.complex64).reshape(-1)
    assert np.array_equal(back.view(np.uint32), CM.host_split(hosts[1], QL.wanted_channel(), Fh, corrected, 0, 0, CL.N_OUT, False)[0].view(np.uint32))
    receive_on_device(oracle, ctx, back, fib[0], pay[0], nb, against_oracle=True)
    for b in (cb, bal, tuner):
        b.close()
    ctx.close()
