#!/usr/bin/env python3
"""Rate of the channeliser (dabgpu_channeliser_bank_split / _combine, dab-radio_amd/csrc/channelise.hip) on one MI355X: N wideband streams
x one mode I frame of output per channel, complex float; split at D = 4 with 1, 3 and 4 channels per stream, D = 5 with 5, D = 1 (the
mixer, one channel), combine at D = 4 with 3 channels; the median of --reps calls timed with HIP events.  Algorithmic bytes of a call: the
input once plus the outputs (split: 8 D per block-rate position of a stream + 8 per output sample of a channel; combine: 8 per block
sample of a channel + 8 per wideband sample).  fmaf of a call: split 2 x 72 D per output sample (the filter alone; the rotation is counted
apart), combine 2 x 72 per wideband sample and channel.  Shares are of 8 TB/s and of the 78.6 T fmaf/s vector peak.
    python tools/bench_channelise.py [--frames-total 256] [--reps 20] [--out profiles/tx/bench_channelise.md]"""
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
    ap.add_argument("--frames-total", type=int, default=256, help="output frames of a call, all channels together")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx", "bench_channelise.md"))
    a = ap.parse_args()
    import torch
    import dabgpu
    S = dabgpu.NB_FRAME_SAMPLES
    ctx = dabgpu.Context(0)
    cases = [("split", 4, 1), ("split", 4, 3), ("split", 4, 4), ("split", 5, 5), ("split", 1, 1), ("combine", 4, 3)]
    rows = []
    for kind, D, per in cases:
        N = max(a.frames_total // per, 1)
        rate = 2048000.0 * D
        offs = [(k - (per - 1) / 2.0) * 1712000.0 + 300000.0 for k in range(per)]
        chs = [dabgpu.channeliser_channel(dabgpu.channeliser_freq((o + rate / 2) % rate - rate / 2, rate), 0, 1.0, s) for s in range(N) for o in offs]
        cb = dabgpu.Channeliser(ctx, chs, N, D)
        if kind == "split":
            n_in = (S * D + 72 * D + 1) & ~1
            x = torch.randn((N, n_in, 2), dtype=torch.float32, device="cuda")
            out = torch.empty((N * per, S, 2), dtype=torch.float32, device="cuda")
            ms = median_ms(lambda: cb.split(x, n_in, S, out, in_stride_samples=n_in, wrap=True), a.reps)
            out_samples, nbytes = N * per * S, N * S * D * 8 + N * per * S * 8
            fmaf, lds = N * per * S * 2 * cb.plan["taps"], cb.plan["split_lds_bytes"]
        else:
            n_in = (S + 74) & ~1
            x = torch.randn((N * per, n_in, 2), dtype=torch.float32, device="cuda")
            out = torch.empty((N, S * D, 2), dtype=torch.float32, device="cuda")
            ms = median_ms(lambda: cb.combine(x, n_in, S * D, out, in_stride_samples=n_in, wrap=True), a.reps)
            out_samples, nbytes = N * S * D, N * per * S * 8 + N * S * D * 8
            fmaf, lds = N * S * D * per * 2 * (cb.plan["taps"] // D), cb.plan["combine_lds_bytes"]
        gbs, tf = nbytes / ms / 1e6, fmaf / ms / 1e9
        rows.append((f"{kind}, D = {D}, {per} channel{'s' if per > 1 else ''} per stream", N, lds, ms, out_samples / ms / 1e6, gbs, gbs / 8000 * 100, tf, tf / 78.6 * 100))
        cb.close()
        del x, out
    text = [f"# Channeliser: one mode I frame ({S} samples) per output row, {a.frames_total} output frames per split call, complex float, median of {a.reps} calls (HIP events)",
            "", f"Device: {torch.cuda.get_device_properties(0).gcnArchName} ({torch.cuda.get_device_name(0)}).  Measured on one MI355X by tools/bench_channelise.py.", "",
            "| case | wideband streams | LDS bytes / workgroup | ms / call | G output samples / s | GB/s (algorithmic) | % of 8 TB/s | T fmaf/s (filter) | % of 78.6 T fmaf/s |",
            "|---|---|---|---|---|---|---|---|---|"]
    text += [f"| {n} | {s} | {l} | {ms:.3f} | {sps:.2f} | {g:.0f} | {p:.1f} | {f:.2f} | {fp:.1f} |" for n, s, l, ms, sps, g, p, f, fp in rows]
    text = "\n".join(text) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
