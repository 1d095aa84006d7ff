#!/usr/bin/env python3
"""Rate of the interferer (dabgpu_interferer_bank_apply, dab-radio_amd/csrc/interferer.hip) on one MI355X: N streams x one mode I frame,
complex float to complex float: one BAND source at L = 1, 16 and 64, four BAND sources, a white source, tones only.  Beside it, on the
same buffers and alternating with it in the same session, dabgpu_channel_bank_apply with one zero-delay tap -- without noise: the same
load and store path and nothing else; with noise: the same generator on every sample, the figure to beat.  A warm loop, then the median of
--reps calls per case timed with HIP events, the cases taken in turn within every repetition.  Algorithmic bytes: 16 per sample (8 read, 8
written); shares are of 8 TB/s.
    python tools/bench_interferer.py [--streams 4096] [--reps 15] [--out profiles/tx/bench_interferer.md]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "dab-radio_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx", "bench_interferer.md"))
    a = ap.parse_args()
    import torch
    import dabgpu
    N, S = a.streams, dabgpu.NB_FRAME_SAMPLES
    ctx = dabgpu.Context(0)
    frames = torch.randn((N, S, 2), dtype=torch.float32, device="cuda")
    out = torch.empty((N, S, 2), dtype=torch.float32, device="cuda")
    shapes = [dabgpu.interferer_design(w) for w in (0.6, 96000.0 / 2048000.0, 2.0 ** -7)]
    assert [H.interp for H in shapes] == [1, 16, 64]
    B, T = dabgpu.INTERFERER_BAND, dabgpu.INTERFERER_TONE

    def band(shape, f):
        return dabgpu.interferer_source(B, amp=1.0, shape=shape, cycles_per_sample=f)

    cases = [("one BAND source, L = 1", [band(0, 0.1)]), ("one BAND source, L = 16", [band(1, 0.146)]), ("one BAND source, L = 64", [band(2, 0.146)]),
             ("four BAND sources, L = 16", [band(1, f) for f in (0.146, -0.2, 0.3, -0.4)]),
             ("four BAND sources, L = 1, 16, 64, 64", [band(0, 0.1), band(1, -0.2), band(2, 0.3), band(2, -0.4)]),
             ("one white source", [band(-1, 0.0)]),
             ("one tone", [dabgpu.interferer_source(T, amp=1.0, cycles_per_sample=0.01)]),
             ("four tones", [dabgpu.interferer_source(T, amp=1.0, cycles_per_sample=f) for f in (0.01, -0.02, 0.3, -0.4)]),
             ("one white burst source, on 1 % of the time", [dabgpu.interferer_source(B, amp=1.0, shape=-1, gate_period=20480, gate_on=205)])]
    runs = []
    for name, sources in cases:
        bank = dabgpu.Interferer(ctx, [dabgpu.interferer_stream(sources, seed=s + 1) for s in range(N)], shapes)
        runs.append((name, bank, lambda bank=bank: bank.apply(frames, S, out, in_stride_samples=S), bank.plan["lds_bytes"]))
    for name, kw in (("channel bank, 1 zero-delay tap, no noise", dict()), ("channel bank, 1 zero-delay tap, noise", dict(noise_sigma=0.01))):
        ch = dabgpu.Channel(ctx, [dabgpu.channel_stream(seed=s + 1, taps=[(0, 1.0, 0.0)], cycles_per_sample=1e-4, **kw) for s in range(N)])
        runs.append((name, ch, lambda ch=ch: ch.apply(frames, S, S, out, in_stride_samples=S, wrap=True), 0))
    for _, _, fn, _ in runs:                                                 # the warm loop
        fn(); fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _, _ in runs}
    for _ in range(a.reps):                                                  # the cases in turn within every repetition
        for name, _, fn, _ in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
    copy, noisy = med["channel bank, 1 zero-delay tap, no noise"], med["channel bank, 1 zero-delay tap, noise"]
    text = [f"# Interferer: {N} streams x one mode I frame ({S} samples), complex float in and out, median of {a.reps} calls (HIP events)", "",
            f"Device: {torch.cuda.get_device_properties(0).gcnArchName} ({torch.cuda.get_device_name(0)}).  The cases alternate within every repetition, "
            "on the same two buffers.  Algorithmic bytes: 16 per sample.", "",
            "| case | LDS bytes / workgroup | ms / call | GB/s (algorithmic) | % of 8 TB/s | x channel bank without noise | x channel bank with noise |",
            "|---|---|---|---|---|---|---|"]
    for name, _, _, lds in runs:
        ms = med[name]
        gbs = N * S * 16 / ms / 1e6
        text.append(f"| {name} | {lds} | {ms:.3f} | {gbs:.0f} | {gbs / 80:.1f} | {ms / copy:.2f} | {ms / noisy:.2f} |")
    text = "\n".join(text) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    for _, bank, _, _ in runs:
        bank.close()
    ctx.close()


if __name__ == "__main__":
    main()
