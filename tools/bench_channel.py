#!/usr/bin/env python3
"""Rate of the channel model (dabgpu_channel_bank_apply, dab-radio_amd/csrc/channel.hip) on one MI355X: N streams x one mode I frame,
complex float and u8 output, one tap without noise / one tap with noise / four taps with noise, the median of --reps calls timed with
HIP events; the modulator (dabgpu_ofdm_modulate_frames) on the same number of frames in the same process for comparison.  Algorithmic
bytes: 16 per sample for complex float out (8 read, 8 written), 10 for u8; shares are of 8 TB/s.  Behind them, in the same process, the
fading kernel (channel_fading.hip): the same four taps all Rayleigh, and two of the four, against the static four-tap rows just measured
(--fading-out; the ratio is against those rows, never against figures from another machine).
    python tools/bench_channel.py [--streams 4096] [--reps 30] [--out profiles/tx/bench_channel.md]
                                  [--fading-out profiles/tx/bench_channel_fading.md] [--doppler-hz 100]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "dab-radio_amd")]


def median_ms(fn, reps):
    import torch
    fn(); fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx", "bench_channel.md"))
    ap.add_argument("--fading-out", default=os.path.join(ROOT, "profiles", "tx", "bench_channel_fading.md"))
    ap.add_argument("--doppler-hz", type=float, default=100.0)
    a = ap.parse_args()
    import torch
    import dabgpu
    N, S = a.streams, dabgpu.NB_FRAME_SAMPLES
    ctx = dabgpu.Context(0)
    F32, U8 = dabgpu.IQ_FORMATS.index("raw_f32l"), dabgpu.IQ_FORMATS.index("raw_u8")
    payload = torch.randint(0, 256, (N, dabgpu.NB_FRAME_BITS // 8), dtype=torch.uint8, device="cuda")
    frames = torch.empty((N, S, 2), dtype=torch.float32, device="cuda")
    out = torch.empty((N, S, 2), dtype=torch.float32, device="cuda")
    L = dabgpu.lib()
    st = dabgpu.Context._stream(None)

    def mod(fmt, dst):
        dabgpu.check(L.dabgpu_ofdm_modulate_frames(ctx._h, 1, dabgpu._ptr(payload), dabgpu.TX_PAYLOAD_FRAME_BITS, N, None, 0.0, dabgpu._ptr(dst), fmt, st), "modulate")

    rows = []
    t_mod = {F32: median_ms(lambda: mod(F32, out), a.reps), U8: median_ms(lambda: mod(U8, out), a.reps)}
    mod(F32, frames)
    scale = (1.0 / 1536 * 4.0) * 127.5
    taps4 = [(0, 1.0, 0.0), (60, 0.5, 0.2), (200, 0.35, -0.35), (450, 0.0, 0.25)]
    cases = [("1 tap, no noise", dict(taps=[(0, 1.0, 0.0)], cycles_per_sample=1e-4)),
             ("1 tap, noise", dict(taps=[(0, 1.0, 0.0)], cycles_per_sample=1e-4, noise_sigma=0.01)),
             ("4 taps, noise", dict(taps=taps4, cycles_per_sample=1e-4, noise_sigma=0.01))]
    for name, kw in cases:
        ch = dabgpu.Channel(ctx, [dabgpu.channel_stream(seed=s + 1, **kw) for s in range(N)])
        for fmt, label, bps in ((F32, "f32", 16), (U8, "u8", 10)):
            ms = median_ms(lambda: ch.apply(frames, S, S, out, in_stride_samples=S, wrap=True, out_format=fmt, u8_scale=scale), a.reps)
            gbs = N * S * bps / ms / 1e6
            rows.append((name, label, ms, gbs, gbs / 8000 * 100, ms / t_mod[fmt]))
        ch.close()
    static4 = {l: ms for n, l, ms, _, _, _ in rows if n == "4 taps, noise"}
    frows = []
    streams = [dabgpu.channel_stream(seed=s + 1, **cases[2][1]) for s in range(N)]
    for name, kinds in (("4 taps, all static kinds, noise", [0, 0, 0, 0]), ("4 taps, 2 Rayleigh, noise", [0, 1, 0, 1]), ("4 taps, 4 Rayleigh, noise", [1, 1, 1, 1])):
        tables = dabgpu.channel_fading_plan(streams, [dabgpu.channel_fading_spec(a.doppler_hz / 2.048e6, s + 1, kinds) for s in range(N)])
        ch = dabgpu.Channel(ctx, streams, fading=tables)
        for fmt, label, bps in ((F32, "f32", 16), (U8, "u8", 10)):
            ms = median_ms(lambda: ch.apply(frames, S, S, out, in_stride_samples=S, wrap=True, out_format=fmt, u8_scale=scale), a.reps)
            frows.append((name, label, ms, N * S * bps / ms / 1e6, ms / static4[label]))
        ch.close()
    ftext = [f"# Fading channel: {N} streams x one mode I frame ({S} samples), Doppler {a.doppler_hz:g} Hz, median of {a.reps} calls (HIP events)", "",
             f"Device: {torch.cuda.get_device_properties(0).gcnArchName} ({torch.cuda.get_device_name(0)}).  The yardstick, measured in the same process on "
             f"the same card: the plain bank's \"4 taps, noise\" rows, {static4['f32']:.3f} ms (f32) and {static4['u8']:.3f} ms (u8).", "",
             "| case (fading bank) | out | ms / call | GB/s (algorithmic) | x static 4 taps |", "|---|---|---|---|---|"]
    ftext += [f"| {n} | {l} | {ms:.3f} | {g:.0f} | {r:.2f} |" for n, l, ms, g, r in frows]
    ftext = "\n".join(ftext) + "\n"
    text = [f"# Channel model: {N} streams x one mode I frame ({S} samples), median of {a.reps} calls (HIP events)", "",
            f"Device: {torch.cuda.get_device_properties(0).gcnArchName} ({torch.cuda.get_device_name(0)}).  Modulator on the same {N} frames: "
            f"{t_mod[F32]:.3f} ms (f32, {N * S * 8 / t_mod[F32] / 1e6 / 80:.1f} % of 8 TB/s written), {t_mod[U8]:.3f} ms (u8).", "",
            "| case | out | ms / call | GB/s (algorithmic) | % of 8 TB/s | x modulator |", "|---|---|---|---|---|---|"]
    text += [f"| {n} | {l} | {ms:.3f} | {g:.0f} | {p:.1f} | {r:.2f} |" for n, l, ms, g, p, r in rows]
    text = "\n".join(text) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    print(ftext)
    os.makedirs(os.path.dirname(a.fading_out), exist_ok=True)
    open(a.fading_out, "w").write(ftext)


if __name__ == "__main__":
    main()
