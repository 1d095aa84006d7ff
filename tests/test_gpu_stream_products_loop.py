"""-m gpu: the closed loop of tests/test_stream_products_closed_loop.py on the device.  The CPU loop's three streams -- (12 dB, +200 ppm),
(12 dB, -200 ppm), (15 dB, no clock error), each behind its lead-in -- are one stream bank with products
(dabgpu_stream_bank_set_products), fed in blocks of 65536 with 2 bits slots.  After every call, for every slot whose record is valid:
dabgpu_clock_estimate_frames over (products, records) with the stream's state word in place, gain 1 -> dabgpu_clock_derotate_frames
by that word -> dabgpu_diversity_combine_frames over the one branch (products, the bank's scale words, records), once on the products as
they came and once on the de-rotated ones.  The bits are fetched and counted by the oracle's decoders as the CPU loop counts them.
Counts of both paths and the five tracked slope words of every stream equal the CPU test's; no stream desyncs."""
import numpy as np
import pytest

import clock_loop as L
import clock_model as CK
import stream_products_model as SPM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def loop(oracle, tmp_path_factory):
    return L.Loop(oracle, tmp_path_factory.mktemp("stream_products_loop"))


def test_tracker_and_combiner_behind_the_bank_equal_the_cpu_loop(oracle, loop):
    import dabgpu
    import torch
    cpu = [SPM.cpu_point(oracle, loop, snr_db, ppm) for snr_db, ppm in SPM.POINTS]
    streams = np.stack([p["stream"] for p in cpu])
    E, n = streams.shape
    slots, block, NB = 2, SPM.BLOCK, dabgpu.NB_FRAME_BITS
    ctx = dabgpu.Context(0)
    bank = dabgpu.StreamBank(ctx, E)
    scale = torch.zeros(E * slots, dtype=torch.float32, device="cuda")
    dq = torch.zeros((E * slots, 75, 1536, 2), dtype=torch.float32, device="cuda")
    dv = torch.zeros_like(dq)
    rec = torch.zeros((E * slots, 6), dtype=torch.int32, device="cuda")
    bank.set_soft(dabgpu.SoftCfg(dabgpu.SOFT_CSI, L.PL.LEVEL), scale)
    bank.set_products(dq, rec)
    bits = torch.zeros((E, slots, NB), dtype=torch.int8, device="cuda")
    out = {p: torch.zeros((E * slots, NB), dtype=torch.int8, device="cuda") for p in SPM.PATHS}
    nf = torch.zeros(E, dtype=torch.int32, device="cuda")
    state = torch.zeros(E, dtype=torch.int64, device="cuda")                  # the tracker's word of every stream, updated in place
    ok = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = {p: [[] for _ in range(E)] for p in SPM.PATHS}
    slopes = [[] for _ in range(E)]
    sdt = np.dtype(dabgpu.SYNC_STATE_DTYPE)
    for k in range(0, n, block):
        m = min(block, n - k)
        d_iq = torch.view_as_real(torch.from_numpy(np.ascontiguousarray(streams[:, k:k + m])).cuda())
        bank.process(d_iq, m, m, bits, slots, nf)
        torch.cuda.synchronize()
        valid = rec.cpu().numpy().view(sdt)["sync_valid"].reshape(E, slots)
        assert np.array_equal(valid.sum(axis=1), nf.cpu().numpy())
        for e in range(E):
            for j in range(slots):
                if not valid[e, j]:
                    continue
                s = e * slots + j
                ctx.clock_estimate(dq[s], 1, sync=rec[s], slope_in=state[e:e + 1], gain=1.0, slope_out=state[e:e + 1], valid=ok)
                ctx.clock_derotate(dq[s], dv[s], 1, state[e:e + 1], sync=rec[s])
                ctx.diversity_combine([(dq[s], scale[s:s + 1], None, rec[s])], 1, out["plain"][s])
                ctx.diversity_combine([(dv[s], scale[s:s + 1], None, rec[s])], 1, out["tracked"][s])
                torch.cuda.synchronize()
                assert ok.item() == 1
                assert torch.equal(out["plain"][s], bits[e, j]), "the one-branch combination of the products is the bank's own frame"
                for p in SPM.PATHS:
                    got[p][e].append(out[p][s].cpu().numpy())
                slopes[e].append(int(state[e].item()))
    st = bank.status()
    assert (st["total_frames_desync"] == 0).all() and (st["total_frames_read"] == SPM.N_FRAMES).all()
    for e, (snr_db, ppm) in enumerate(SPM.POINTS):
        counts = {p: loop.count(got[p][e]) for p in SPM.PATHS}
        print(f"SNR {snr_db} dB, {ppm} ppm: device {counts}, CPU {cpu[e]['counts']}, tracked {[round(CK.ppm_of(s), 1) for s in slopes[e]]} ppm")
        assert len(slopes[e]) == SPM.N_FRAMES and slopes[e] == cpu[e]["slopes"], (e, slopes[e], cpu[e]["slopes"])
        assert counts == cpu[e]["counts"], (e, counts, cpu[e]["counts"])
    bank.close(); ctx.close()
