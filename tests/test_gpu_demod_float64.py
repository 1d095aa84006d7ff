"""-m gpu: the demodulation kernels against the float64 model of tests/demod_model.py directly -- the oracle is not in the loop, so a
mistake the oracle and a kernel share does not pass here.  Stage by stage, each with its derived bound (see the model's docstrings):
spectra against numpy's complex128 transform of the input rotated in float64; the DQPSK view and the soft bits against the device's own
float32 spectra (every bit in its interval, the norm's component exactly -+127); cyclic-prefix correlations against the float64 sum;
summed phase and fine-frequency update against the device's own correlations.  Mode I kernel at symbols_per_block 1 / 7 / 75 (run
boundaries, halo), its capture-format loaders, the size-generic kernel of modes II-IV, the bits-only wave / pair kernels, the phase
tail alone and fused.  Three frames per case (the PLL's phase restarts per frame) with different offsets; every test prints the worst
ratio to each bound."""
import numpy as np
import pytest

import demod_model as DM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


def build_case(mode):
    """three frames: no offset and one purely real symbol; tiny (1e-12), a notch of carriers whose norm is ~1e-3 of the others', and a
    residual offset of -0.4 rad per symbol left after the PLL (the phase tail then has something to sum, and a fine frequency near the
    wrap point wraps); huge (1e12) and noisier.  All clear of subnormals and overflow.  The float64 references are computed once."""
    g = DM.Geometry(mode)
    rng = np.random.default_rng(4200 + mode)
    residual = -0.4 / (2 * np.pi * g.N)
    notch = tuple(int(s) for s in rng.choice(g.NC, 6, replace=False))
    specs = [dict(f=0.0, noise=0.03, real_symbol=3), dict(f=7e-4, noise=0.05, scale=1e-12, notch=notch), dict(f=-2.3e-3, noise=0.2, scale=1e12)]
    frames = np.stack([DM.make_frame(mode, rng, **s)[0] for s in specs])
    f = np.array([0.0, 7e-4 + residual, -2.3e-3], np.float32)
    return {"mode": mode, "g": g, "frames": frames, "f": f, "scale": [s.get("scale", 1.0) for s in specs],
            "ref": [DM.demodulate(frames[k], f[k], mode) for k in range(len(specs))]}


@pytest.fixture(scope="module")
def case():
    made = {}

    def get(mode):
        if mode not in made:
            made[mode] = build_case(mode)
        return made[mode]
    return get


def launch(ctx, c, frames=None, raw=None, fmt=None, views=True, spb=0, dqpsk=False):
    """one demodulation launch of the case's frames (mode I: the register-resident kernel, or its raw loaders; else the generic entry)"""
    import torch
    g, n = c["g"], len(c["f"])
    d_f = torch.from_numpy(c["f"]).cuda()
    d_bits = torch.zeros((n, g.frame_bits), dtype=torch.int8, device="cuda")
    d_corr = torch.zeros((n, g.L, 2), dtype=torch.float32, device="cuda")
    d_fft = torch.zeros((n, g.L + 1, g.N, 2), dtype=torch.float32, device="cuda") if views else None
    d_dq = torch.zeros((n, g.L - 1, g.NC, 2), dtype=torch.float32, device="cuda") if dqpsk else None
    if raw is not None:
        d_raw = torch.from_numpy(raw).cuda()
        ctx.ofdm_demod_frames_raw(d_raw, fmt, n, d_bits, freq_offset=d_f, cp_corr=d_corr, fft=d_fft, symbols_per_block=spb, dqpsk=d_dq)
    else:
        d_iq = torch.from_numpy(np.ascontiguousarray(c["frames"] if frames is None else frames).view(np.float32)).cuda()
        if c["mode"] == 1:
            ctx.ofdm_demod_frames(d_iq, d_bits, freq_offset=d_f, cp_corr=d_corr, fft=d_fft, symbols_per_block=spb, n_frames=n, dqpsk=d_dq)
        else:
            ctx.ofdm_demod_frames_mode(c["mode"], d_iq, n, d_bits, freq_offset=d_f, cp_corr=d_corr, fft=d_fft, symbols_per_block=spb)
    torch.cuda.synchronize()
    cplx = lambda t: None if t is None else np.ascontiguousarray(t.cpu().numpy()).view(np.complex64)[..., 0]
    return {"bits": d_bits.cpu().numpy(), "corr": cplx(d_corr), "fft": cplx(d_fft), "dqpsk": cplx(d_dq), "d_corr": d_corr}


def hold_views(out, c, refs, what):
    """spectra, soft bits (and the DQPSK view) and correlations of a launch that returned its spectra; -> the intervals per frame"""
    mode, ivs = c["mode"], []
    for k, ref in enumerate(refs):
        w = (what, "frame", k)
        r_fft = DM.hold_fft(out["fft"][k], ref, mode, c["f"][k], w)
        iv = DM.soft_bit_intervals(out["fft"][k], mode)
        r_dq = DM.hold_dqpsk(out["dqpsk"][k], iv, w) if out["dqpsk"] is not None else float("nan")
        differ, ambiguous = DM.hold_soft_bits(out["bits"][k], iv, w)
        r_corr = DM.hold_cp(out["corr"][k], ref, mode, c["f"][k], w)
        print(f"{what} frame {k} f {float(c['f'][k]):+.4e}: spectrum {r_fft:.3f}, DQPSK product {r_dq:.3f}, correlation {r_corr:.3f} of their bounds; "
              f"soft bits: delta up to {iv['delta'].max():.2e} counts, {differ:.5%} differ from plain truncation, {ambiguous:.5%} ambiguous")
        ivs.append(iv)
    return ivs


@pytest.mark.parametrize("spb", [1, 7, 75])
def test_mode_1_kernel_with_all_views(ctx, case, spb):
    c = case(1)
    out = launch(ctx, c, spb=spb, dqpsk=True)
    hold_views(out, c, c["ref"], f"mode 1 symbols_per_block {spb}")


@pytest.mark.parametrize("fmt", ["raw_u8", "raw_s8", "raw_s16l"])
def test_mode_1_capture_format_loaders(ctx, case, fmt):
    """the frames quantised to the capture format; the model decodes the bytes itself (demod_model.decode_capture)"""
    import dabgpu
    c = case(1)
    raw = np.stack([DM.encode_capture(c["frames"][k].astype(np.complex128) / c["scale"][k], fmt, 5.0) for k in range(len(c["f"]))])
    refs = [DM.demodulate(DM.decode_capture(raw[k], fmt), c["f"][k], 1) for k in range(len(c["f"]))]
    out = launch(ctx, c, raw=raw, fmt=dabgpu.IQ_FORMATS.index(fmt), dqpsk=True)
    hold_views(out, c, refs, f"mode 1 {fmt}")


@pytest.mark.parametrize("mode", [2, 3, 4])
def test_generic_kernel_and_the_bits_only_kernels(ctx, case, mode):
    """with the FFT view: the size-generic kernel.  Without it: the wave kernels (modes II, IV) and the pair kernel (mode III), whose
    soft bits are held to the intervals of the spectra the view launch returned for the same input, and whose correlations to the model"""
    c = case(mode)
    ivs = hold_views(launch(ctx, c), c, c["ref"], f"mode {mode} generic")
    for spb in (0, 7):
        out = launch(ctx, c, views=False, spb=spb)
        for k, iv in enumerate(ivs):
            w = (mode, "bits only", spb, "frame", k)
            differ, _ = DM.hold_soft_bits(out["bits"][k], iv, w)
            r_corr = DM.hold_cp(out["corr"][k], c["ref"][k], mode, c["f"][k], w)
            print(f"mode {mode} bits only, symbols_per_block {spb}, frame {k}: correlation {r_corr:.3f} of its bound, {differ:.5%} of the soft bits "
                  f"differ from plain truncation")


def fine_inputs(g):
    """frame 1 carries -0.4 rad per symbol: from 0.95 of the wrap point its update crosses it (and lands 0.06 of it past zero, far from
    any wrap point: no excuse)"""
    return np.array([1e-5, 0.95 * 0.5 * 1.01 / g.N, -2e-5], np.float32)


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_phase_tail(ctx, case, mode):
    """dabgpu_ofdm_phase_update[_mode] on the correlations the demodulation left on the device"""
    import torch
    c = case(mode)
    g, n = c["g"], len(c["f"])
    out = launch(ctx, c, views=False)
    fine0 = fine_inputs(g)
    d_total = torch.zeros(n, dtype=torch.float32, device="cuda")
    d_fine = torch.from_numpy(fine0.copy()).cuda()
    if mode == 1:
        ctx.ofdm_phase_update(out["d_corr"], n, total_phase=d_total, fine_freq=d_fine, beta=0.9)
    else:
        ctx.ofdm_phase_update_mode(mode, out["d_corr"], n, total_phase=d_total, fine_freq=d_fine, beta=0.9)
    torch.cuda.synchronize()
    total, fine = d_total.cpu().numpy(), d_fine.cpu().numpy()
    hold_tail(out["corr"], total, fine0, fine, c, f"mode {mode} phase update")


def hold_tail(corr, total, fine0, fine, c, what):
    g = c["g"]
    wrapped = 0
    for k in range(len(c["f"])):
        bound = DM.angle_bounds_from_input(c["ref"][k], c["mode"], c["f"][k])
        r_angle = DM.hold_angles(np.angle(corr[k].astype(np.complex128)), c["ref"][k], bound, (what, k))      # the correlation's angle is the model's
        r_total, r_fine, near = DM.hold_phase_tail(corr[k], total[k], fine0[k], fine[k], 0.9, c["mode"], (what, "frame", k))
        assert not near, (what, k)
        wrapped += abs(float(fine0[k]) - float(np.float32(0.9)) * float(total[k]) / (g.N * g.L * 2 * np.pi)) > 0.5 * 1.01 / g.N
        print(f"{what} frame {k}: total {float(total[k]):+.4f} rad at {r_total:.4f}, fine frequency {float(fine0[k]):+.4e} -> {float(fine[k]):+.4e} at "
              f"{r_fine:.3f} of their bounds (angle of the correlation at {r_angle:.3f})")
    assert wrapped == 1, "the case must hold one update that wraps"


@pytest.mark.parametrize("spb", [75, 25])
def test_mode_1_fused_phase_tail(ctx, case, spb):
    """dabgpu_ofdm_demod_phase_frames: the tail inside the demodulation kernel (a workgroup per frame, 75) and as its own launch (25);
    soft bits against the intervals of the spectra a view launch returns for the same input"""
    import dabgpu
    import torch
    c = case(1)
    g, n = c["g"], len(c["f"])
    ivs = [DM.soft_bit_intervals(x, 1) for x in launch(ctx, c)["fft"]]
    fine0 = fine_inputs(g)
    d_raw = torch.from_numpy(np.ascontiguousarray(c["frames"]).view(np.float32)).cuda()
    d_bits = torch.zeros((n, g.frame_bits), dtype=torch.int8, device="cuda")
    d_corr = torch.zeros((n, g.L, 2), dtype=torch.float32, device="cuda")
    d_total = torch.zeros(n, dtype=torch.float32, device="cuda")
    d_fine = torch.from_numpy(fine0.copy()).cuda()
    ctx.ofdm_demod_phase_frames(d_raw, dabgpu.IQ_FORMATS.index("raw_f32l"), n, d_bits, freq_offset=torch.from_numpy(c["f"]).cuda(), cp_corr=d_corr,
                                symbols_per_block=spb, beta=0.9, total_phase=d_total, fine_freq=d_fine)
    torch.cuda.synchronize()
    corr = np.ascontiguousarray(d_corr.cpu().numpy()).view(np.complex64)[..., 0]
    bits = d_bits.cpu().numpy()
    for k in range(n):
        w = ("fused phase tail", spb, "frame", k)
        DM.hold_soft_bits(bits[k], ivs[k], w)
        print(f"fused phase tail, symbols_per_block {spb}, frame {k}: correlation {DM.hold_cp(corr[k], c['ref'][k], 1, c['f'][k], w):.3f} of its bound")
    hold_tail(corr, d_total.cpu().numpy(), fine0, d_fine.cpu().numpy(), c, f"fused phase tail, symbols_per_block {spb}")
