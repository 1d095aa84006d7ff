"""-m gpu: the closed loop of tests/blanker_loop.py with every stage on the device: TxBank -> the channel bank -> the interferer bank's
burst source, in place -> the blanker bank -> dabgpu_ofdm_sync_demod_frames_branch -> dabgpu_diversity_combine_frames (plain) into a
history ring -> dabgpu_decode_frames_layout (the chain of tests/test_gpu_interferer_loop.py with the blanker in it).  At SNR 12 dB with
bursts at I / S 17 and 23 dB: the blanked stream and its mask words equal the CPU chain's bit for bit, the counts its counts, every FIB
and byte delivered and no frame refused."""
import numpy as np
import pytest

import blanker_loop as BL
import blanker_model as BM
import channel_loop as CL
import channel_model as CM
import interferer_loop as IL
import interferer_model as IM
import noise_loop as NL
from test_gpu_interferer_loop import Chain

pytestmark = pytest.mark.gpu


class BlankedChain(Chain):
    def blanked_stream(self, snr_db, is_db):
        """-> (the blanked stream, its mask words)"""
        dabgpu, torch = self.dabgpu, self.torch
        p = CL.params(self.iq, snr_db)
        p["seed"] = NL.NOISE_SEED["A"]
        n = CL.N_OUT
        d_rx = torch.zeros((1, n, 2), dtype=torch.float32, device="cuda")
        d_out = torch.zeros((1, n, 2), dtype=torch.float32, device="cuda")
        d_mask = torch.zeros((1, dabgpu.blanker_mask_words(n)), dtype=torch.int32, device="cuda")
        ch = dabgpu.Channel(self.ctx, [CM.to_struct(p, dabgpu.ChannelStream)])
        ch.apply(self.d_iq, CL.N_FRAMES * dabgpu.NB_FRAME_SAMPLES, n, d_rx)
        jam = dabgpu.Interferer(self.ctx, [IM.to_struct(IL.burst_stream(self.S, is_db), dabgpu.InterfererStream)])
        jam.apply(d_rx, n, d_rx, in_stride_samples=n)                               # in place
        blanker = dabgpu.Blanker(self.ctx, [BM.to_struct(BL.PARAMS, dabgpu.BlankerStream)])
        blanker.apply(d_rx, n, n, d_out, in_stride_samples=n, d_mask=d_mask)
        torch.cuda.synchronize()
        ch.close(); jam.close(); blanker.close()
        return d_out.cpu().numpy().view(np.complex64).reshape(-1), d_mask.cpu().numpy().view(np.uint32).reshape(-1)


@pytest.fixture(scope="module")
def chain(oracle):
    c = BlankedChain(oracle)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cpu_loop(oracle, tmp_path_factory):
    return BL.Loop(oracle, tmp_path_factory.mktemp("blanker_loop"))


@pytest.mark.parametrize("is_db", [17.0, 23.0])
def test_device_loop_equals_the_cpu_loop(chain, cpu_loop, is_db):
    rx, mask = chain.blanked_stream(BL.SNR_DB, is_db)
    want, want_mask, n, total = cpu_loop.blanked_stream(BL.SNR_DB, is_db, "burst")
    assert np.array_equal(mask, want_mask), "the mask words differ from the CPU chain's"
    assert np.array_equal(rx.view(np.uint32), want.view(np.uint32)), "the blanked stream differs from the CPU chain's"
    counts, lost = chain.point(rx, alphas=())
    cpu = cpu_loop.blanked(BL.SNR_DB, is_db, "burst")
    print(f"SNR {BL.SNR_DB} dB, bursts at I / S {is_db} dB: device {counts}, CPU {cpu}, {n} of {total} blocks blanked, frames without sync {lost}")
    assert lost == 0 and counts["plain"] == cpu == BL.DELIVERED
