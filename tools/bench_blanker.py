#!/usr/bin/env python3
"""Rate of the impulse blanker (dabgpu_blanker_bank_apply, dab-radio_amd/csrc/blanker.hip) on one MI355X: N streams x one mode I frame,
complex float to complex float, default parameters (reach 25 blocks): nothing flagged (Gaussian input), white bursts on 205 of every
20480 samples 17 dB above the input (the interferer bank's burst source), every block flagged (an input of NaN: the
non-finite path, a bound on what zeroing every block costs, not the threshold decision), and a disabled bank; the first two with and
without the mask.  Beside it, alternating with it in the same session, dabgpu_channel_bank_apply with one
zero-delay tap and no noise: the same load and store path and nothing else -- the copy path, the figure to compare with.  Every timed
call, the channel bank's included, is a seek to position 0 and the apply: the same count of launches on both sides of the ratio.  A warm loop,
then the median of --reps calls per case timed with HIP events, the cases taken in turn within every repetition.  Algorithmic bytes: 16 per
sample (8 read, 8 written); shares are of 8 TB/s.
    python tools/bench_blanker.py [--streams 4096] [--reps 15] [--out profiles/tx/bench_blanker.md]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "dab-radio_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx", "bench_blanker.md"))
    a = ap.parse_args()
    import torch
    import dabgpu
    N, S = a.streams, dabgpu.NB_FRAME_SAMPLES
    ctx = dabgpu.Context(0)
    clean = torch.randn((N, S, 2), dtype=torch.float32, device="cuda")       # power 2 per sample
    bursts = torch.empty_like(clean)
    amp = (2.0 * 10.0 ** 1.7) ** 0.5
    white = -1                                                               # dabgpu_interferer_source.shape: a BAND source without a shape is white noise
    src = dabgpu.interferer_source(dabgpu.INTERFERER_BAND, amp=amp, shape=white, gate_period=20480, gate_on=205, gate_offset=-1000)
    itf = dabgpu.Interferer(ctx, [dabgpu.interferer_stream([src], seed=s + 1) for s in range(N)])
    itf.apply(clean, S, bursts, in_stride_samples=S)
    nans = torch.full((N, S, 2), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.empty((N, S, 2), dtype=torch.float32, device="cuda")
    words = dabgpu.blanker_mask_words(S)
    mask = torch.zeros((N, words), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    itf.close()

    on = dabgpu.Blanker(ctx, [dabgpu.blanker_stream() for _ in range(N)])
    off = dabgpu.Blanker(ctx, [dabgpu.blanker_stream(enabled=False) for _ in range(N)])
    ch = dabgpu.Channel(ctx, [dabgpu.channel_stream(seed=s + 1, taps=[(0, 1.0, 0.0)], cycles_per_sample=1e-4) for s in range(N)])

    def blank(bank, x, m):
        bank.seek(0)
        bank.apply(x, S, S, out, in_stride_samples=S, d_mask=m)

    def copy_row():
        ch.seek(0)
        ch.apply(clean, S, S, out, in_stride_samples=S, wrap=True)

    runs = [("nothing flagged", lambda: blank(on, clean, None)), ("nothing flagged, with the mask", lambda: blank(on, clean, mask)),
            ("1 % bursts at I/S 17 dB", lambda: blank(on, bursts, None)), ("1 % bursts at I/S 17 dB, with the mask", lambda: blank(on, bursts, mask)),
            ("every block flagged (NaN input)", lambda: blank(on, nans, None)), ("a disabled bank", lambda: blank(off, clean, None)),
            ("channel bank, 1 zero-delay tap, no noise", lambda: copy_row())]
    for _, fn in runs:                                                       # the warm loop
        fn(); fn()
    torch.cuda.synchronize()
    share = {}
    for name, x in (("nothing flagged", clean), ("1 % bursts at I/S 17 dB", bursts), ("every block flagged (NaN input)", nans)):
        blank(on, x, mask)
        torch.cuda.synchronize()
        bits = int(sum(bin(int(w) & 0xFFFFFFFF).count("1") for w in mask[:8].cpu().numpy().ravel()))
        share[name] = bits / (8 * S / 32)
    times = {name: [] for name, _ in runs}
    for _ in range(a.reps):                                                  # the cases in turn within every repetition
        for name, fn in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
    copy = med["channel bank, 1 zero-delay tap, no noise"]
    text = [f"# Impulse blanker: {N} streams x one mode I frame ({S} samples), complex float in and out, median of {a.reps} calls (HIP events)", "",
            f"Device: {torch.cuda.get_device_properties(0).gcnArchName} ({torch.cuda.get_device_name(0)}).  Default parameters (threshold 3, gap 8, "
            f"window 16, guard 1: reach 25 blocks), tile {dabgpu.BLANKER_BLOCK} samples, {on.plan['lds_bytes']} bytes of LDS per workgroup.  The cases "
            "alternate within every repetition; every call, the channel bank's too, is a seek to position 0 and the apply.  Algorithmic "
            "bytes: 16 per sample.  Blanked share: blocks blanked of the first 8 streams.", "",
            "| case | blanked share | ms / call | GB/s (algorithmic) | % of 8 TB/s | x channel bank without noise |",
            "|---|---|---|---|---|---|"]
    for name, _ in runs:
        ms = med[name]
        gbs = N * S * 16 / ms / 1e6
        sh = share.get(name.replace(", with the mask", ""))
        text.append(f"| {name} | {'' if sh is None or 'channel' in name or 'disabled' in name else f'{100 * sh:.2f} %'} | {ms:.3f} | {gbs:.0f} | {gbs / 80:.1f} | {ms / copy:.2f} |")
    text = "\n".join(text) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    for bank in (on, off, ch):
        bank.close()
    ctx.close()


if __name__ == "__main__":
    main()
