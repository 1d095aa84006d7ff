#!/usr/bin/env python3
"""Rate of the IQ balance bank (dabgpu_iqbal_bank_apply, dab-radio_amd/csrc/iqbal.hip) on one MI355X: N streams x one mode I frame, complex
float to complex float: APPLY alone with TRACK streams (the map with the records' coefficients), APPLY alone with OFF streams (a copy),
MEASURE | APPLY in one pass, and MEASURE alone (no output).  Beside it, alternating with it in the same session, dabgpu_channel_bank_apply
with one zero-delay tap and no noise: the same load and store path and nothing else -- the copy path tools/bench_blanker.py compares with.
Every timed call, the channel bank's included, is a seek to position 0 and the apply.  A warm loop, then the median of --reps calls per
case timed with HIP events, the cases taken in turn within every repetition.  Algorithmic bytes: 16 per sample (8 read, 8 written) plus
32 per tile of 1024 samples with MEASURE; 8 per sample plus 32 per tile for MEASURE alone; shares are of 8 TB/s.
    python tools/bench_iqbal.py [--streams 4096] [--reps 15] [--out profiles/tx/bench_iqbal.md]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "dab-radio_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx", "bench_iqbal.md"))
    a = ap.parse_args()
    import torch
    import dabgpu
    N, S = a.streams, dabgpu.NB_FRAME_SAMPLES
    tiles = S // dabgpu.IQBAL_TILE
    ctx = dabgpu.Context(0)
    clean = torch.randn((N, S, 2), dtype=torch.float32, device="cuda")
    clean[:, :, 1] *= 1.05                                                   # a gain error for the estimator to find
    out = torch.empty((N, S, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    track = dabgpu.IqBalance(ctx, [dabgpu.iqbal_stream() for _ in range(N)], S)
    off = dabgpu.IqBalance(ctx, [dabgpu.iqbal_stream(mode=dabgpu.IQBAL_OFF) for _ in range(N)], S)
    ch = dabgpu.Channel(ctx, [dabgpu.channel_stream(seed=s + 1, taps=[(0, 1.0, 0.0)], cycles_per_sample=1e-4) for s in range(N)])

    def iq(bank, flags):
        bank.seek(0)
        bank.apply(clean, S, out if flags & dabgpu.IQBAL_APPLY else None, flags=flags, in_stride_samples=S)

    def copy_row():
        ch.seek(0)
        ch.apply(clean, S, S, out, in_stride_samples=S, wrap=True)

    A, M = dabgpu.IQBAL_APPLY, dabgpu.IQBAL_MEASURE
    per_sample = 16 * N * S
    runs = [("APPLY, TRACK streams", lambda: iq(track, A), per_sample), ("APPLY, OFF streams (copy)", lambda: iq(off, A), per_sample),
            ("MEASURE + APPLY", lambda: iq(track, A | M), per_sample + 32 * N * tiles), ("MEASURE alone", lambda: iq(track, M), per_sample // 2 + 32 * N * tiles),
            ("channel bank, 1 zero-delay tap, no noise", copy_row, per_sample)]
    for _, fn, _ in runs:                                                    # the warm loop (the MEASURE calls prime the records)
        fn(); fn()
    torch.cuda.synchronize()
    rec = track.read_state()
    times = {name: [] for name, _, _ in runs}
    for _ in range(a.reps):                                                  # the cases in turn within every repetition
        for name, fn, _ in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
    copy = med["channel bank, 1 zero-delay tap, no noise"]
    text = [f"# IQ balance bank: {N} streams x one mode I frame ({S} samples = {tiles} tiles), complex float in and out, median of {a.reps} calls (HIP events)", "",
            f"Device: {torch.cuda.get_device_properties(0).gcnArchName} ({torch.cuda.get_device_name(0)}).  Default parameters (forget "
            f"{dabgpu.iqbal_stream().forget:.8f}, min_weight 65536), tile {dabgpu.IQBAL_TILE} samples, {track.plan['scratch_bytes']} bytes of tile scratch.  "
            "The cases alternate within every repetition; every call, the channel bank's too, is a seek to position 0 and the apply.  Algorithmic "
            "bytes: 16 per sample, plus 32 per tile with MEASURE; MEASURE alone reads 8 per sample.  "
            f"After the warm loop {int((rec['valid'] == 1).sum())} of {N} records are valid, median |w| {float(sorted((rec['w_re'] ** 2 + rec['w_im'] ** 2) ** 0.5)[N // 2]):.4f}.", "",
            "| case | ms / call | GB/s (algorithmic) | % of 8 TB/s | x channel bank without noise |",
            "|---|---|---|---|---|"]
    for name, _, nbytes in runs:
        ms = med[name]
        gbs = nbytes / ms / 1e6
        text.append(f"| {name} | {ms:.3f} | {gbs:.0f} | {gbs / 80:.1f} | {ms / copy:.2f} |")
    text = "\n".join(text) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    for bank in (track, off, ch):
        bank.close()
    ctx.close()


if __name__ == "__main__":
    main()
