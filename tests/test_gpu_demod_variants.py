"""-m gpu: the demodulator instantiations that no other test launches (profiles/demod_launch/coverage.md), each through the stream bank --
the only caller that hands the launcher frame descriptors -- and each against the oracle state machine (tests/stream_model.py) fed the
same blocks: every completed frame's soft bits bit for bit, and after every call the status of every stream with its floats as bit
patterns.  The bank does not hand out the cyclic-prefix correlations of a round; the fine-frequency word it reports is the IIR over their
angles summed in symbol order, so a correlation that differed in one bit would show there.

dabgpu_launch_demod picks a kernel out of a table by the planner's variant index (1 + loader with descriptors) and, for the wave kernels,
by a row per mode (mode III under DABGPU_MODE3_SINGLE: the one-symbol row): a table entry in the wrong place reads the block in another
capture format or another mode's geometry, and no frame would equal the oracle's.

  mode I     ofdm_demod_kernel<s8, bank, class order>
  modes II-IV  u8 and s8 blocks: ofdm_demod_wave_kernel<2 | 4, u8 | s8, bank>, ofdm_demod_wave3_kernel<u8 | s8, bank>
  mode III, DABGPU_MODE3_SINGLE: ofdm_demod_wave_kernel<3, every loader, bank>
  DABGPU_MODE_GENERIC: ofdm_demod_mode_kernel<every loader, bank>

Not here: ofdm_demod_kernel<*, bank, views> -- no entry point can ask a bank round for the display views."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


FORMATS = {"c32": "raw_f32l", "u8": "raw_u8", "s8": "raw_s8", "s16": "raw_s16l"}


def quantise(streams, fmt):
    """complex float streams -> raw capture bytes [E][n * sample bytes] of the format"""
    raws = []
    for s in streams:
        x = np.stack([s.real, s.imag], axis=-1).reshape(-1)
        x = x / np.abs(x).max()
        if fmt == "c32":
            raws.append(np.ascontiguousarray(s).view(np.uint8))
        elif fmt == "u8":
            raws.append(np.clip(np.rint(x * 127.0 + 127.5), 0, 255).astype(np.uint8))
        elif fmt == "s8":
            raws.append(np.clip(np.rint(x * 127.0), -128, 127).astype(np.int8).view(np.uint8))
        else:
            raws.append(np.clip(np.rint(x * 30000.0), -32768, 32767).astype("<i2").view(np.uint8))
    return np.stack(raws)


def same_status(st, models, where):
    for e, mo in enumerate(models):
        assert int(st["state"][e]) == mo.state, where + (e,)
        assert st["signal_l1_average"][e].view(np.uint32) == np.float32(mo.signal_avg).view(np.uint32), where + (e,)
        assert st["freq_coarse"][e].view(np.uint32) == np.float32(mo.sync.freq_coarse).view(np.uint32), where + (e,)
        assert st["freq_fine"][e].view(np.uint32) == np.float32(mo.sync.freq_fine).view(np.uint32), where + (e,)
        assert int(st["fine_time_offset"][e]) == mo.fine_time_offset, where + (e,)
        assert int(st["total_frames_read"][e]) == mo.frames_read and int(st["total_frames_desync"][e]) == mo.frames_desync, where + (e,)


_mode_streams = {}


def mode_streams(oracle, mode):
    """two receivers of a transmission mode, five frames each, other carrier offsets and start positions (computed once per mode)"""
    import modes_model as MM
    if mode not in _mode_streams:
        g = oracle.geometry(mode)
        out = []
        for seed, cfo_bins, pad, noise in ((1, 2.1, 77, 0.05), (2, -3.4, 311, 0.1)):
            rng = np.random.default_rng(7000 * mode + seed)
            sent = [rng.integers(0, 2, g.nb_frame_bits, dtype=np.uint8) for _ in range(5)]
            tx = oracle.apply_pll(np.concatenate([MM.make_tx_frame(oracle, mode, b, rng) for b in sent]), cfo_bins / g.nb_fft, 0.2)
            s = np.concatenate([tx[g.nb_null_period:g.nb_null_period + 6000 + pad], tx])
            out.append(((s + noise * (rng.standard_normal(s.size) + 1j * rng.standard_normal(s.size))) / 39.2).astype(np.complex64))
        n = min(s.size for s in out) // 8 * 8
        _mode_streams[mode] = [s[:n] for s in out]
    return _mode_streams[mode]


CASES = [(mode, fmt, None) for mode in (2, 3, 4) for fmt in ("u8", "s8")]
CASES += [(3, fmt, "DABGPU_MODE3_SINGLE") for fmt in ("c32", "u8", "s8", "s16")]
CASES += [(2, "c32", "DABGPU_MODE_GENERIC"), (3, "u8", "DABGPU_MODE_GENERIC"), (4, "s8", "DABGPU_MODE_GENERIC"), (2, "s16", "DABGPU_MODE_GENERIC")]


@pytest.mark.parametrize("mode,fmt,switch", CASES, ids=[f"mode{m}-{f}-{(s or 'default').lower()}" for m, f, s in CASES])
def test_bank_rounds_of_modes_2_to_4_by_loader_and_switch(ctx, oracle, mode, fmt, switch):
    import dabgpu
    import stream_model as SM
    import torch
    g = oracle.geometry(mode)
    fnum = dabgpu.IQ_FORMATS.index(FORMATS[fmt])
    sb = dabgpu.iq_format_sample_bytes(fnum)
    raw = quantise(mode_streams(oracle, mode), fmt)
    E, n = raw.shape[0], raw.shape[1] // sb
    iq = [oracle.iq_convert(raw[e], fnum).view(np.complex64) for e in range(E)]         # what the loader makes of the bytes
    d_raw = torch.from_numpy(raw).cuda()
    cfg = dabgpu.StreamCfg()
    dabgpu.lib().dabgpu_stream_cfg_default(dabgpu.C.byref(cfg))
    cfg.sync.impulse_peak_threshold_db = 8.0             # the reference's default 20 dB rarely passes with the short symbols of modes II / III
    bank = dabgpu.StreamBank(ctx, E, cfg, mode=mode)
    models = [SM.StreamModel(oracle, mode) for _ in range(E)]
    for m in models:
        m.cfg.impulse_peak_threshold_db = 8.0
    block = 40000
    max_frames = block // (g.nb_frame_samples - g.nb_null_period - g.nb_symbol_period) + 2
    d_bits = torch.zeros((E, max_frames, g.nb_frame_bits), dtype=torch.int8, device="cuda")
    d_nf = torch.zeros(E, dtype=torch.int32, device="cuda")
    frames = 0
    assert not switch or switch not in os.environ
    try:
        if switch:
            os.environ[switch] = "1"
        for k in range(0, n, block):
            m = min(block, n - k)
            d_bits.zero_()
            bank.process_raw(d_raw[:, sb * k:].data_ptr(), fnum, n, m, d_bits, max_frames, d_nf)
            torch.cuda.synchronize()
            nf = d_nf.cpu().numpy()
            for e in range(E):
                before = len(models[e].out_frames)
                models[e].process(iq[e][k:k + m])
                new = models[e].out_frames[before:]
                assert nf[e] == len(new), (mode, fmt, k, e, nf[e], len(new))
                for j, fr in enumerate(new):
                    assert np.array_equal(d_bits[e, j].cpu().numpy(), fr["bits"]), (mode, fmt, k, e, j)
                frames += len(new)
            same_status(bank.status(), models, (mode, fmt, k))
    finally:
        if switch:
            os.environ.pop(switch, None)
        bank.close()
    assert frames >= 6, frames                           # both receivers locked and delivered most of their five frames


def test_mode_1_bank_round_from_s8_blocks_in_class_order(ctx, oracle):
    """ofdm_demod_kernel<s8, bank, class order>: the ring form of the bank, soft bits of the MSC in time-interleaver class order"""
    import dabgpu
    import stream_model as SM
    import torch
    from test_gpu_stream_bank import make_stream
    fnum = dabgpu.IQ_FORMATS.index("raw_s8")
    streams = [make_stream(oracle, 31, 3, 1.1e-3, 500, 2.0), make_stream(oracle, 32, 3, -0.7e-3, 1700, 4.0)]
    n = min(s.size for s in streams) // 8 * 8
    raw = quantise([s[:n] for s in streams], "s8")
    E, H, block = 2, 5, 150000 + 2                       # at most one frame per call and stream; + 2: odd byte alignments inside the raw data
    iq = [oracle.iq_convert(raw[e], fnum).view(np.complex64) for e in range(E)]
    d_raw = torch.from_numpy(raw).cuda()
    bank = dabgpu.StreamBank(ctx, E)
    models = [SM.StreamModel(oracle) for _ in range(E)]
    d_hist = torch.zeros((E, H, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
    d_slot = torch.full((E,), -1, dtype=torch.int32, device="cuda")
    to_natural = dabgpu.classed_to_natural_index()
    frames = 0
    for k in range(0, n, block):
        m = min(block, n - k)
        bank.process_ring(d_raw[:, 2 * k:].data_ptr(), fnum, n, m, d_hist, H, d_slot, bits_layout=dabgpu.BITS_MSC_CLASSED)
        torch.cuda.synchronize()
        slot, hist = d_slot.cpu().numpy(), d_hist.cpu().numpy()
        for e in range(E):
            before = len(models[e].out_frames)
            models[e].process(iq[e][k:k + m])
            new = models[e].out_frames[before:]
            assert len(new) <= 1
            if not new:
                assert slot[e] == -1, (k, e)
                continue
            assert slot[e] == (models[e].frames_read - 1) % H, (k, e)
            assert np.array_equal(hist[e, slot[e]][to_natural], new[0]["bits"]), (k, e)
            assert not np.array_equal(hist[e, slot[e]], new[0]["bits"]), "the MSC symbols are in class order, not in natural order"
            frames += 1
        same_status(bank.status(), models, (k,))
    bank.close()
    assert frames >= 3, frames
