"""-m gpu: dabgpu_radio_cli --ber on the closed-loop capture of tests/channel_loop.py (two paths, offset, 15 dB).  The capture's soft bits
(dabgpu_ofdm_sync_demod_frames, as tests/test_gpu_ber_loop.py produces them) go in as the bit file of --configuration dab; the figures the
tool prints per frame -- FIC, then one per sub-channel, errors / bits -- equal the model's (tests/ber_model.py) on those soft bits with
the oracle's decoded bytes.  Without --ber the tool prints nothing and writes the same files."""
import os
import re
import subprocess

import numpy as np
import pytest

import ber_model as M
import channel_loop as CL
import channel_model as CM
import tx_encode_cases as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dab-radio_amd", "host", "apps", "dabgpu_radio_cli")


def test_printed_figures_equal_the_model(oracle, tmp_path):
    import dabgpu
    import torch
    ctx = dabgpu.Context(0)
    fib, pay, nb = CL.inputs(oracle)
    gsubs = [T.g_sub(dabgpu, d) for d in CL.SUBS]
    osubs = [T.o_sub(oracle, d) for d in CL.SUBS]
    F, S = CL.N_FRAMES, dabgpu.NB_FRAME_SAMPLES
    bank = dabgpu.TxBank(ctx, 1, gsubs)
    iq = bank.transmit_frames_host(fib, pay, F).reshape(-1)
    ch = dabgpu.Channel(ctx, [CM.to_struct(CL.params(iq), dabgpu.ChannelStream)])
    rx = ch.apply_host(iq, CL.N_OUT).reshape(-1)
    slices = CL.slices_of(rx)
    d_st = torch.zeros(np.dtype(dabgpu.SYNC_STATE_DTYPE).itemsize, dtype=torch.uint8, device="cuda")
    d_bits = torch.zeros((F, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
    for j in range(F):
        d_slice = torch.from_numpy(np.ascontiguousarray(slices[j:j + 1]).view(np.float32)).cuda()
        ctx.ofdm_sync_demod_frames(d_slice, 1, CL.STRIDE, CL.P, d_st, d_bits[j])
    torch.cuda.synchronize()
    ring = d_bits.cpu().numpy()
    ch.close(); bank.close(); ctx.close()
    ring.tofile(tmp_path / "bits.bin")
    sub_args = ["--radio-subchannel", "0,48,3,A", "--radio-subchannel", "200,52,uep,20"]
    env = dict(os.environ, DABGPU_VITERBI_CORE="scalar")           # the oracle's decoders below model the scalar core
    base = [CLI, "-i", str(tmp_path / "bits.bin"), "--configuration", "dab", *sub_args]
    res = subprocess.run(base + ["--radio-fib-output", str(tmp_path / "fib_b.bin"), "--radio-msc-output", str(tmp_path / "b_"), "--ber"],
                         capture_output=True, timeout=300, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    plain = subprocess.run(base + ["--radio-fib-output", str(tmp_path / "fib_p.bin"), "--radio-msc-output", str(tmp_path / "p_")],
                           capture_output=True, timeout=300, env=env)
    assert plain.returncode == 0 and plain.stdout == b""
    for a, b in (("fib_b.bin", "fib_p.bin"), ("b_0.bin", "p_0.bin"), ("b_1.bin", "p_1.bin")):
        assert (tmp_path / a).read_bytes() == (tmp_path / b).read_bytes()
    lines = res.stdout.decode().strip().splitlines()
    assert len(lines) == F
    total = 0
    for j, line in enumerate(lines):
        m = re.fullmatch(r"ber frame=(\d+) fic=(\d+)/(\d+) sub0=(\d+)/(\d+) sub1=(\d+)/(\d+)", line)
        assert m, line
        got = [int(x) for x in m.groups()]
        fibb = np.stack([oracle.fic_decode_group(ring[j, 2304 * g:2304 * (g + 1)])[0] for g in range(4)])
        first = min(max(0, 15 - 4 * j), 4)
        msc = np.zeros((4, nb), np.uint8)
        for q in range(first, 4):
            off = 0
            for sc in osubs:
                bits = np.zeros(64 * sc.length, np.int8)
                K = M.kept_bits(oracle, sc)
                bits[:K] = M.consumed(ring, j, q, sc.start_address, K)
                out = oracle.msc_decode_logical(sc, bits)[0]
                msc[q, off:off + out.size] = out
                off += out.size
        fic_r, msc_r = M.ber_frames(oracle, ring, j, osubs, fibb, msc)
        exp = [j, int(fic_r["n_errors"].sum()), int(fic_r["n_bits"].sum())]
        for s in range(len(osubs)):
            exp += [int(msc_r[first:, s]["n_errors"].sum()), int(msc_r[first:, s]["n_bits"].sum())]
        assert got == exp, (j, line)
        total += exp[1] + exp[3] + exp[5]
    assert total > 0
    bad = subprocess.run([CLI, "--configuration", "ofdm", "--ber"], capture_output=True, timeout=60)
    assert bad.returncode != 0 and b"--ber needs the channel decode stage" in bad.stderr
