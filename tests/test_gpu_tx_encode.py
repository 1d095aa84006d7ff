"""-m gpu: the channel encoder bank on the device (dabgpu_tx_bank_*, dab-radio_amd/csrc/dab_encode.hip).
Parity is against the ORACLE composition as whole 28800-byte frames (tests/tx_encode_cases.py: fic_encode_group per FIB group,
msc_encode_logical per sub-channel and CIF, time_interleave over the whole sequence into a zero CIF, LSB-first packing); then call
splitting, guard patterns, the closed loop through the product's own demodulator and decoders, the fused call against the two separate
ones, the host forms, and HIP-graph replay.  Every output buffer of this file sits between two 4 KiB guard patterns that are checked
after each call."""
import numpy as np
import pytest

import tx_encode_cases as T

pytestmark = pytest.mark.gpu
GUARD = 4096
N_FRAMES = 6                # CIFs 0..23: start-up zero fill (frames 0-3) and steady state (from CIF 15 on)


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


def guarded(n_bytes):
    """a device buffer of n_bytes between two guard patterns: (whole, view)"""
    import torch
    whole = torch.full((GUARD + n_bytes + GUARD,), 0xC3, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + n_bytes]


def guards_intact(whole):
    h = whole.cpu().numpy()
    return bool((h[:GUARD] == 0xC3).all() and (h[-GUARD:] == 0xC3).all())


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def encode(bank, fib, pay, n_ens, calls=None):
    """fib [n][F][4][3][30], pay [n][F][4][nb] numpy -> [n][F][28800] numpy, in one call or split as `calls` = (F1, F2, ...)"""
    import torch
    F = fib.shape[1]
    out = np.zeros((n_ens, F, 28800), np.uint8)
    at = 0
    for Fc in (calls or (F,)):
        whole, view = guarded(n_ens * Fc * 28800)
        d_fib, d_pay = dev(fib[:, at:at + Fc]), dev(pay[:, at:at + Fc])
        bank.encode_frames(d_fib, d_pay if pay.shape[-1] else None, Fc, view)
        torch.cuda.synchronize()
        assert guards_intact(whole), "the encoder wrote outside its output"
        out[:, at:at + Fc] = view.cpu().numpy().reshape(n_ens, Fc, 28800)
        at += Fc
    assert at == F
    return out


def check_against_oracle(oracle, got, subs, fib, pay, what):
    for e in range(got.shape[0]):
        exp = T.expected_frames(oracle, subs, fib[e], pay[e])
        if not np.array_equal(got[e], exp):
            bad = np.argwhere(got[e] != exp)
            raise AssertionError(f"{what}: ensemble {e}: {len(bad)} bytes differ from the oracle composition, first at frame {bad[0][0]} byte {bad[0][1]}")


def layouts():
    import dabsynth
    return {"canonical": T.layout_subs(dabsynth.canonical_layout()), "mixed": T.layout_subs(dabsynth.mixed_layout())}


@pytest.mark.parametrize("n_ens", [1, 3, 65, 257])
@pytest.mark.parametrize("name", ["canonical", "mixed"])
def test_multiplex_frames_equal_the_oracle_composition(oracle, ctx, name, n_ens):
    import dabgpu
    subs = layouts()[name]
    bank = dabgpu.TxBank(ctx, n_ens, [T.g_sub(dabgpu, d) for d in subs])
    rng = np.random.default_rng(5200 + n_ens)
    fib, pay = T.random_input(rng, n_ens, N_FRAMES, bank.cif_in_bytes)
    got = encode(bank, fib, pay, n_ens)
    check_against_oracle(oracle, got, subs, fib, pay, f"{name} x {n_ens}")
    bank.close()


def test_every_profile_at_two_starts_equals_the_oracle_composition(oracle, ctx):
    import dabgpu
    rng = np.random.default_rng(5300)
    n_done = 0
    for prof in T.profiles(dabgpu):
        room = 864 - prof["length"]
        second = room if room % 2 == 1 or room == 0 else room - 1          # an odd start where there is one
        for start in sorted({0, second}):
            d = dict(prof, start=start)
            bank = dabgpu.TxBank(ctx, 2, [T.g_sub(dabgpu, d)])
            fib, pay = T.random_input(rng, 2, N_FRAMES, bank.cif_in_bytes)
            got = encode(bank, fib, pay, 2)
            check_against_oracle(oracle, got, [d], fib, pay, str(d))
            bank.close()
            n_done += 1
    assert n_done >= 2 * (63 + 11) - 8


@pytest.mark.parametrize("name", ["canonical", "mixed"])
def test_call_splitting_and_reset(oracle, ctx, name):
    import dabgpu
    subs = layouts()[name]
    n_ens = 3
    bank = dabgpu.TxBank(ctx, n_ens, [T.g_sub(dabgpu, d) for d in subs])
    rng = np.random.default_rng(5400)
    fib, pay = T.random_input(rng, n_ens, N_FRAMES, bank.cif_in_bytes)
    one = encode(bank, fib, pay, n_ens)
    check_against_oracle(oracle, one, subs, fib, pay, name)
    for calls in ((1, 5), (2, 2, 2), (1, 1, 1, 1, 1, 1)):
        bank.reset()
        assert np.array_equal(encode(bank, fib, pay, n_ens, calls), one), calls
    # without a reset the interleaver goes on: the same input gives other frames, the continuation of a 12-frame sequence
    cont = encode(bank, fib, pay, n_ens)
    assert not np.array_equal(cont, one)
    twice = T.expected_frames(oracle, subs, np.concatenate([fib[0], fib[0]]), np.concatenate([pay[0], pay[0]]))
    assert np.array_equal(cont[0], twice[N_FRAMES:])
    bank.close()


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_extremes_fic_only_full_multiplex_constant_payload(oracle, ctx, fill):
    import dabgpu
    rng = np.random.default_rng(5500 + fill)
    # FIC only: every CIF is zero
    bank = dabgpu.TxBank(ctx, 3, [])
    assert bank.cif_in_bytes == 0
    fib = np.full((3, N_FRAMES, 4, 3, 30), fill, np.uint8)
    pay = np.zeros((3, N_FRAMES, 4, 0), np.uint8)
    got = encode(bank, fib, pay, 3)
    check_against_oracle(oracle, got, [], fib, pay, "FIC only")
    assert not got[:, :, 1152:].any()
    bank.close()
    # all 864 capacity units: one sub-channel, the canonical 18, and 64 sub-channels (63 of 12 CU and one of 108, EEP 1-A)
    full = [[dict(start=0, length=864, is_uep=0, uep_index=0, eep_level=2, eep_type=0)], layouts()["canonical"],
            [dict(start=12 * k, length=12, is_uep=0, uep_index=0, eep_level=0, eep_type=0) for k in range(63)] +
            [dict(start=756, length=108, is_uep=0, uep_index=0, eep_level=0, eep_type=0)]]
    for subs in full:
        assert sum(d["length"] for d in subs) == 864
        bank = dabgpu.TxBank(ctx, 2, [T.g_sub(dabgpu, d) for d in subs])
        fib = rng.integers(0, 256, (2, N_FRAMES, 4, 3, 30), dtype=np.uint8)
        pay = np.full((2, N_FRAMES, 4, bank.cif_in_bytes), fill, np.uint8)
        got = encode(bank, fib, pay, 2)
        check_against_oracle(oracle, got, subs, fib, pay, f"{len(subs)} sub-channels on 864 CU, payload {fill:#x}")
        bank.close()


def transmit(bank, fib, pay, n_ens, F, fmt=None, freq_norm=0.0):
    import dabgpu
    import torch
    f32 = dabgpu.IQ_FORMATS.index("raw_f32l")
    per = 196608 * (8 if fmt in (None, f32) else 2)
    whole, view = guarded(n_ens * F * per)
    bank.transmit_frames(dev(fib), dev(pay) if pay.shape[-1] else None, F, view, freq_norm=freq_norm, out_format=fmt)
    torch.cuda.synchronize()
    assert guards_intact(whole), "transmit_frames wrote outside its output"
    return view


@pytest.mark.parametrize("bits_layout", [0, 1], ids=["natural", "classed"])
def test_closed_loop_bytes_to_iq_to_bytes(ctx, bits_layout):
    """transmit_frames (complex float, no noise) -> ofdm_demod_frames_history -> decode_frames: from the frame that holds CIF 15 on,
    every sub-channel's bytes are the payload of the CIF 15 earlier and every FIB body is its input with its CRC valid"""
    import dabgpu
    import torch
    subs = layouts()["mixed"]
    gsubs = [T.g_sub(dabgpu, d) for d in subs]
    E, H = 3, 8
    bank = dabgpu.TxBank(ctx, E, gsubs)
    nb, n_sub = bank.cif_in_bytes, len(subs)
    rng = np.random.default_rng(5600)
    fib_in, pay = T.random_input(rng, E, N_FRAMES, nb)
    iq = transmit(bank, fib_in, pay, E, N_FRAMES).view(torch.float32).reshape(E, N_FRAMES, 196608, 2)
    fmt = dabgpu.IQ_FORMATS.index("raw_f32l")
    hist = torch.zeros((E, H, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
    fib = torch.zeros((E, 4, 96), dtype=torch.uint8, device="cuda"); fres = torch.zeros((E * 4, 16), dtype=torch.uint8, device="cuda")
    out = torch.zeros((E, 4, nb), dtype=torch.uint8, device="cuda"); res = torch.zeros((E * 4 * n_sub, 16), dtype=torch.uint8, device="cuda")
    cifs = pay.reshape(E, 4 * N_FRAMES, nb)
    rdt = np.dtype(dabgpu.RESULT_DTYPE)
    checked = 0
    for j in range(N_FRAMES):
        # the demodulator's frame buffer: PRS first, the NULL of the following frame last
        frame = torch.zeros((E, 196608, 2), dtype=torch.float32, device="cuda")
        frame[:, :196608 - 2656] = iq[:, j, 2656:]
        ctx.ofdm_demod_frames_history(frame, fmt, E, hist[:, j % H], bits_frame_stride=H * dabgpu.NB_FRAME_BITS, bits_layout=bits_layout)
        ctx.decode_frames(hist, E, H * dabgpu.NB_FRAME_BITS, H, j % H, gsubs, fib, fres, out, 4 * nb, res, bits_layout=bits_layout)
        torch.cuda.synchronize()
        got_fib, got = fib.cpu().numpy(), out.cpu().numpy()
        assert (fres.cpu().numpy().view(rdt)["crc_ok_mask"] == 7).all(), f"frame {j}: FIB CRCs"
        for g in range(4):
            for i in range(3):
                assert np.array_equal(got_fib[:, g, 32 * i:32 * i + 30], fib_in[:, j, g, i]), (j, g, i)
        for c in range(4):
            if 4 * j + c >= 15:
                assert np.array_equal(got[:, c], cifs[:, 4 * j + c - 15]), f"frame {j} CIF {c}"
                checked += 1
    assert checked == 4 * N_FRAMES - 15
    bank.close()


def test_fused_call_equals_encode_then_modulate(ctx):
    import dabgpu
    import torch
    f32, u8 = dabgpu.IQ_FORMATS.index("raw_f32l"), dabgpu.IQ_FORMATS.index("raw_u8")
    subs = layouts()["mixed"]
    gsubs = [T.g_sub(dabgpu, d) for d in subs]
    E, F = 5, 3
    rng = np.random.default_rng(5700)
    for fmt, freq in ((f32, 0.0), (u8, 1.25e-3)):
        a, b = dabgpu.TxBank(ctx, E, gsubs), dabgpu.TxBank(ctx, E, gsubs)
        fib, pay = T.random_input(rng, E, F, a.cif_in_bytes)
        fused = transmit(a, fib, pay, E, F, fmt=fmt, freq_norm=freq).cpu().numpy()
        bits = encode(b, fib, pay, E)
        per = 196608 * (8 if fmt == f32 else 2)
        whole, view = guarded(E * F * per)
        ctx.ofdm_modulate_frames(1, dev(bits), E * F, view, layout=dabgpu.TX_PAYLOAD_FRAME_BITS, out_format=fmt, freq_norm=freq)
        torch.cuda.synchronize()
        assert guards_intact(whole)
        assert np.array_equal(fused, view.cpu().numpy()), dabgpu.IQ_FORMATS[fmt]
        # the host forms, one ensemble: the same bytes as the batch call's ensemble 0 on a fresh bank
        one = dabgpu.TxBank(ctx, 1, gsubs)
        assert np.array_equal(one.encode_frames_host(fib[:1], pay[:1], F)[0], bits[0])
        one.reset()
        h = one.transmit_frames_host(fib[:1], pay[:1], F, freq_norm=freq, out_format=fmt)
        assert np.array_equal(np.ascontiguousarray(h).view(np.uint8).reshape(-1), fused[:F * per])
        for k in (a, b, one):
            k.close()


def test_captured_encode_step_replays_onto_the_following_frames(oracle, ctx):
    import dabgpu
    import torch
    subs = layouts()["mixed"]
    gsubs = [T.g_sub(dabgpu, d) for d in subs]
    E = 4
    eager, graphed = dabgpu.TxBank(ctx, E, gsubs), dabgpu.TxBank(ctx, E, gsubs)
    rng = np.random.default_rng(5800)
    fib, pay = T.random_input(rng, E, N_FRAMES, eager.cif_in_bytes)
    exp = encode(eager, fib, pay, E)
    check_against_oracle(oracle, exp, subs, fib, pay, "eager")
    side = torch.cuda.Stream()
    whole, view = guarded(E * 28800)
    s_fib, s_pay = dev(fib[:, :1]), dev(pay[:, :1])
    with torch.cuda.stream(side):
        graphed.encode_frames(s_fib, s_pay, 1, view, stream=side.cuda_stream)           # frame 0, eagerly
    side.synchronize()
    assert np.array_equal(view.cpu().numpy().reshape(E, 28800), exp[:, 0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        graphed.encode_frames(s_fib, s_pay, 1, view, stream=side.cuda_stream)
    # (capturing enqueues nothing: the bank still stands after frame 0)
    for j in range(1, N_FRAMES):
        s_fib.copy_(dev(fib[:, j:j + 1])); s_pay.copy_(dev(pay[:, j:j + 1]))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(view.cpu().numpy().reshape(E, 28800), exp[:, j]), f"replay {j}"
    assert guards_intact(whole)
    # growing the bank's frame-bit scratch inside a capture is refused, not done
    g2 = torch.cuda.CUDAGraph()
    iq_whole, iq_view = guarded(E * 2 * 196608 * 8)
    two_fib, two_pay = dev(fib[:, :2]), dev(pay[:, :2])
    torch.cuda.synchronize()
    with pytest.raises(Exception) as err:
        with torch.cuda.graph(g2, stream=side):
            graphed.transmit_frames(two_fib, two_pay, 2, iq_view, stream=side.cuda_stream)
    assert "before capturing" in str(err.value)
    torch.cuda.synchronize()
    eager.close(); graphed.close()
