"""-m gpu: the closed loop of tests/test_stream_soft_closed_loop.py on the device.  The received samples of its two operating points
(`tu6`, six Rayleigh taps at 10 Hz, 10 dB, fading seeds 1 and 7) behind their lead-in, as two streams of one bank, in blocks of 65536
through dabgpu_stream_bank_process_ring (natural layout and class order) -> dabgpu_fic_decode_ring / dabgpu_msc_decode_ring[_layout];
one bank under the normalised policy, one under the weighted one (level 64).

The samples are the host model's, uploaded as they are, not the output of TxBank -> Channel on the device: what is asserted here is
equality with the CPU counts -- FIB CRCs of 60 and wrong bytes of the EEP 3-A sub-channel's five delivered logical frames, for both
policies -- and with the same samples that equality is a property of the bank and the decoders alone (the device chain's counts at these
operating points differ from the CPU's by a CRC here and there, tests/test_gpu_softbits_loop.py tabulates both).  The weighted policy must
be strictly better at both points."""
import numpy as np
import pytest

import channel_fading_model as FM
import channel_loop as CL
import softbit_loop as SL
import softbit_model as SM
import stream_soft_model as SSM
import tx_encode_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def loop(oracle, tmp_path_factory):
    host = FM.build_host_model(tmp_path_factory.mktemp("stream_soft_loop_gpu_host_model"))
    fib, pay, nb = CL.inputs(oracle)
    iq = CL.oracle_iq(oracle, fib, pay)
    points = [SSM.loop_cpu_point(oracle, host, iq, fib, pay, nb, snr, seed) for snr, seed in SSM.LOOP_POINTS]
    return fib, pay, nb, points


@pytest.mark.parametrize("layout", [0, 1], ids=["natural", "classed"])
def test_counts_equal_the_cpu_loop_and_the_weighted_policy_is_better(oracle, loop, layout):
    import dabgpu
    import torch
    fib, pay, nb, points = loop
    E, H, F = len(points), 8, CL.N_FRAMES
    n = min(p[0].size for p in points)
    streams = np.stack([p[0][:n] for p in points])
    fmt = dabgpu.IQ_FORMATS.index("raw_f32l")
    gsubs = [T.g_sub(dabgpu, d) for d in CL.SUBS]
    n0 = oracle.subchannel_plan(T.o_sub(oracle, CL.SUBS[0]))[2]
    cifs = pay.reshape(4 * F, nb)[:, :n0]
    ctx = dabgpu.Context(0)
    d_raw = torch.view_as_real(torch.from_numpy(streams).cuda()).contiguous()
    rdt = np.dtype(dabgpu.RESULT_DTYPE)
    got = {}
    for policy in (dabgpu.SOFT_NORMALISED, dabgpu.SOFT_CSI):
        bank = dabgpu.StreamBank(ctx, E)
        scale = torch.zeros(E * H, dtype=torch.float32, device="cuda")
        bank.set_soft(dabgpu.SoftCfg(policy, SL.LEVEL), scale)
        hist = torch.zeros((E, H, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
        slot = torch.full((E,), -7, dtype=torch.int32, device="cuda")
        d_fib = torch.zeros((E, 4, 96), dtype=torch.uint8, device="cuda"); fres = torch.zeros((E * 4, 16), dtype=torch.uint8, device="cuda")
        msc = torch.zeros((E, 4, nb), dtype=torch.uint8, device="cuda"); mres = torch.zeros((E * 4 * len(gsubs), 16), dtype=torch.uint8, device="cuda")
        crc, wrong, frames = [0] * E, [0] * E, [0] * E
        for k in range(0, n, SSM.LOOP_BLOCK):
            m = min(SSM.LOOP_BLOCK, n - k)
            bank.process_ring(d_raw[:, k:].data_ptr(), fmt, n, m, hist, H, slot, bits_layout=layout)
            ctx.fic_decode_ring(hist, E, H * dabgpu.NB_FRAME_BITS, slot, d_fib, fres)
            ctx.msc_decode_ring(hist, E, H * dabgpu.NB_FRAME_BITS, H, slot, gsubs, msc, 4 * nb, mres, bits_layout=layout)
            torch.cuda.synchronize()
            sl = slot.cpu().numpy()
            masks = fres.cpu().numpy().view(rdt)["crc_ok_mask"].reshape(E, 4)
            out = msc.cpu().numpy()
            for e in range(E):
                if sl[e] < 0:
                    continue
                j = frames[e]
                assert sl[e] == j % H
                crc[e] += int(sum(bin(int(x)).count("1") for x in masks[e]))
                for c in range(4):
                    if 4 * j + c >= 15:
                        wrong[e] += int((out[e, c, :n0] != cifs[4 * j + c - 15]).sum())
                frames[e] += 1
        assert frames == [F] * E and int(bank.status()["total_frames_desync"].sum()) == 0
        got[policy] = [(crc[e], wrong[e]) for e in range(E)]
        bank.close()
    ctx.close()
    for e, (snr, seed) in enumerate(SSM.LOOP_POINTS):
        cpu = points[e][2]
        norm, csi = got[dabgpu.SOFT_NORMALISED][e], got[dabgpu.SOFT_CSI][e]
        print(f"{snr} dB, fading seed {seed}: normalised {norm}, weighted {csi} (FIB CRCs of 60, wrong bytes); CPU {cpu[SM.SOFT_NORMALISED]}, {cpu[SM.SOFT_CSI]}")
        assert norm == cpu[SM.SOFT_NORMALISED] and csi == cpu[SM.SOFT_CSI]
        assert csi[0] > norm[0] and csi[1] < norm[1]
