"""-m gpu: OFDM_Demod::SetSoftDecision through tests/cpp/softbit_class_harness.cpp.  The capture is the transmission of
tests/channel_loop.py through the two-path host model at 15 dB.  The class's soft bits with DABGPU_SOFT_CSI equal the batch call's
(dabgpu_ofdm_demod_frames_soft) for the same frames: where each frame lies in the capture and with which offset the class corrected it
is pinned first with the NORMALISED policy -- the class's normalised bits must equal the batch call's at that position and offset --
and the weighted bits are then compared at exactly those (every delivered frame but the first after the acquisition, whose loop state
the class does not publish).  A receiver that the default rule makes a member of the receiver bank leaves
the bank when the policy is chosen before its first Process() call, stays private and gives the same bits; chosen after frames have
run, a member refuses; a bad level is refused."""
import os
import subprocess

import numpy as np
import pytest

import channel_loop as CL
import softbit_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "cpp", "softbit_class_harness")
NB, S = SC.NB_FRAME_BITS, SC.NB_FRAME_SAMPLES
LEAD = 2656                                  # the capture repeats its first NULL symbol in front: the run-in of the power-dip search
SEARCH = 4


def harness(capture, out, policy, level, others, when, env=None):
    os.makedirs(out, exist_ok=True)
    e = dict(os.environ)
    e.pop("DABGPU_MIRROR_BANK", None); e.pop("DABGPU_MIRROR_BANK_FROM", None)
    e.update(env or {})
    res = subprocess.run([HARNESS, str(capture), str(out), "65536", str(policy), repr(float(level)), str(others), when], capture_output=True, timeout=300, env=e)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    info = dict(kv.split("=", 1) for kv in res.stdout.decode().strip().split(" ", 4))
    bits = np.fromfile(os.path.join(out, "frame_bits.bin"), np.int8).reshape(-1, NB)
    st = np.fromfile(os.path.join(out, "states.bin"), np.float32).reshape(-1, 3)
    return info, bits, st


@pytest.fixture(scope="module")
def capture(oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("softbits_class")
    rx = SC.received(oracle, d)[0]
    stream = np.concatenate([rx[:LEAD], rx]).astype(np.complex64)
    stream.tofile(d / "iq.c32")
    return d, stream


@pytest.fixture(scope="module")
def pinned(capture):
    """the class with the normalised policy, and per delivered frame the (position, offset) at which the batch call gives the same bits"""
    import dabgpu
    import torch
    d, stream = capture
    info, bits, st = harness(d / "iq.c32", d / "norm", dabgpu.SOFT_NORMALISED, 64.0, 0, "never")
    n = len(bits)
    assert n >= CL.N_FRAMES - 1 and info["member_at_creation"] == "0"
    first = CL.N_FRAMES - n                                           # the class may spend the first frame on its acquisition
    ctx = dabgpu.Context(0)
    fmt = dabgpu.IQ_FORMATS.index("raw_f32l")
    where = []
    for j in range(n):
        # the PLL ran with coarse + the fine offset BEFORE this frame's update: the previous delivered frame's.  The first frame after an
        # acquisition is left out: what the loop held when it was demodulated is not among the values the class publishes.
        if j == 0:
            continue
        # (the coarse word the class publishes with a frame may already be the next synchronisation's: the reader runs ahead of the
        # delivery; the candidates are the coarse words around the frame, and exactly one of them must reproduce the bits)
        fine = np.float32(st[j - 1, 1])
        freqs = [np.float32(st[k, 0]) + fine for k in (j, j - 1, j + 1) if 0 <= k < n]
        base = LEAD + 2656 + (first + j) * S + CL.TIMING
        shifts = list(range(-SEARCH, SEARCH + 1))
        cand = np.stack([stream[base + o:base + o + S] for o in shifts])
        d_cand = torch.from_numpy(cand.view(np.float32)).cuda()
        hit, nearest = [], []
        for f in freqs:
            out = torch.zeros((len(cand), NB), dtype=torch.int8, device="cuda")
            ctx.ofdm_demod_frames_soft(d_cand, fmt, len(cand), out, dabgpu.SoftCfg(),
                                       freq_offset=torch.full((len(cand),), float(f), dtype=torch.float32, device="cuda"))
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            hit += [(o, f) for o, b in zip(shifts, got) if np.array_equal(b, bits[j])]
            nearest.append(min((int((b != bits[j]).sum()), o) for o, b in zip(shifts, got)))
        assert len(hit) == 1, (f"frame {j} of {n}: the class's normalised bits are the batch call's at exactly one position and offset, found {hit}; "
                               f"states {st.tolist()}, nearest (mismatches, shift) per offset {nearest}")
        where.append((j, base + hit[0][0], hit[0][1]))
    assert len(where) == n - 1
    yield ctx, where, bits
    ctx.close()


def batch_csi(ctx, stream, where, level):
    import dabgpu
    import torch
    frames = np.stack([stream[p:p + S] for _, p, _ in where])
    freq = torch.from_numpy(np.array([f for _, _, f in where], np.float32)).cuda()
    out = torch.zeros((len(where), NB), dtype=torch.int8, device="cuda")
    ctx.ofdm_demod_frames_soft(torch.from_numpy(frames.view(np.float32)).cuda(), dabgpu.IQ_FORMATS.index("raw_f32l"), len(where), out,
                               dabgpu.SoftCfg(dabgpu.SOFT_CSI, level), freq_offset=freq)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("level", [64.0, 20.0])
def test_class_bits_equal_the_batch_call(capture, pinned, level):
    import dabgpu
    d, stream = capture
    ctx, where, norm_bits = pinned
    info, bits, _ = harness(d / "iq.c32", d / f"csi_{level:g}", dabgpu.SOFT_CSI, level, 0, "before")
    assert info["refused"] == "0" and info["member_at_end"] == "0" and len(bits) == len(norm_bits)
    assert np.array_equal(bits[[j for j, _, _ in where]], batch_csi(ctx, stream, where, level))
    assert not np.array_equal(bits, norm_bits)


def test_a_receiver_that_would_join_the_bank_stays_private(capture, pinned):
    import dabgpu
    d, stream = capture
    ctx, where, norm_bits = pinned
    # the second mode I receiver of a process is a member of the bank by the default rule; as a member it gives the normalised bits
    info, member_bits, _ = harness(d / "iq.c32", d / "member", dabgpu.SOFT_NORMALISED, 64.0, 1, "never")
    assert info["member_at_creation"] == "1" and info["member_at_end"] == "1" and len(member_bits) == len(norm_bits)
    print("member's normalised bits equal the private receiver's:", np.array_equal(member_bits, norm_bits))
    # with the policy chosen before the first sample it leaves the bank, and its bits are the batch call's
    for env in (None, {"DABGPU_MIRROR_BANK": "1"}):
        info, bits, _ = harness(d / "iq.c32", d / "left", dabgpu.SOFT_CSI, 64.0, 1 if env is None else 0, "before", env)
        assert info["member_at_creation"] == "1" and info["member_at_end"] == "0" and info["refused"] == "0"
        assert len(bits) == len(norm_bits) and np.array_equal(bits[[j for j, _, _ in where]], batch_csi(ctx, stream, where, 64.0))
    # once frames have run a member refuses, and keeps its bits
    info, bits, _ = harness(d / "iq.c32", d / "late", dabgpu.SOFT_CSI, 64.0, 1, "after")
    assert info["member_at_end"] == "1" and info["refused"] == "1" and "receiver bank" in info["error"] and np.array_equal(bits, member_bits)
    # the normalised policy is no reason to leave
    info, _, _ = harness(d / "iq.c32", d / "stay", dabgpu.SOFT_NORMALISED, 64.0, 1, "before")
    assert info["member_at_end"] == "1" and info["refused"] == "0"


def test_bad_level_is_refused(capture):
    import dabgpu
    d, _ = capture
    for level, others in ((0.5, 0), (128.0, 0), (200.0, 1)):
        info, bits, _ = harness(d / "iq.c32", d / "bad", dabgpu.SOFT_CSI, level, others, "before")
        assert info["refused"] == "1" and "level" in info["error"] and len(bits) == 0
    # (a member that was refused is still a member)
    assert info["member_at_end"] == "1"
