#!/usr/bin/env python3
"""Frames per second of the receive-diversity combiner (dabgpu_diversity_combine_frames) beside the demodulation that feeds it: 1024
frames, 2 and 4 branches, the natural and the class-order layout.  Per shape the K branches are demodulated once from random samples
under DABGPU_SOFT_CSI with the DQPSK view (dabgpu_ofdm_demod_frames_soft: the call a branch is made with), which leaves real products
and scales on the device; both operations are warmed up (untimed launches until 60 ms of kernels have run), then ROUNDS timed rounds
ALTERNATE them -- the K demodulation launches of a batch, and the one combiner launch -- LAUNCHES repetitions each, timed with device
events; the figure is the median round, the spread its slowest and fastest round.  Run lengths are given (25) so that no tuning state
enters.  The combiner's algorithmic bytes per frame are K x 921,600 read + 230,400 written; the fraction is of 8 TB/s.

    python tools/bench_diversity.py [--out profiles/tx/bench_diversity.md] [--rounds 9] [--launches 8] [--frames 1024]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dab-radio_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
PEAK_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx", "bench_diversity.md"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--branches", default="2,4")
    a = ap.parse_args()
    import numpy as np
    import torch
    import dabgpu
    assert torch.cuda.is_available(), "bench_diversity needs the GPU: there is no CPU path to time"
    ctx = dabgpu.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(9620)
    n = a.frames
    fmt = dabgpu.IQ_FORMATS.index("raw_f32l")
    soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0)
    rows = []
    for K in [int(x) for x in a.branches.split(",")]:
        raw = [torch.randn((n, dabgpu.NB_FRAME_SAMPLES, 2), dtype=torch.float32, device="cuda", generator=gen) for _ in range(K)]
        dq = [torch.zeros((n, 75, 1536, 2), dtype=torch.float32, device="cuda") for _ in range(K)]
        scale = [torch.zeros((n,), dtype=torch.float32, device="cuda") for _ in range(K)]
        own = torch.zeros((n, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
        corr = torch.zeros((n, 76, 2), dtype=torch.float32, device="cuda")
        out = torch.zeros((n, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
        k_out = torch.zeros((n,), dtype=torch.float32, device="cuda")
        table = dabgpu.diversity_table([(dq[b], scale[b]) for b in range(K)])

        def demod():
            for b in range(K):
                ctx.ofdm_demod_frames_soft(raw[b], fmt, n, own, soft, cp_corr=corr, dqpsk=dq[b], symbols_per_block=25, soft_scale=scale[b])

        for layout, layout_name in ((dabgpu.BITS_NATURAL, "natural"), (dabgpu.BITS_MSC_CLASSED, "class order")):
            def combine():
                ctx.diversity_combine(table, n, out, bits_layout=layout, symbols_per_block=25, soft_scale=k_out)

            def timed(fn, reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)
            ops = {"demod": demod, "combine": combine}
            warm = 0.0
            while warm < 60.0:
                warm += sum(timed(f, 2) for f in ops.values())
            assert float(k_out.min()) > 0, "the branches' scales did not arrive"
            ms = {k: [] for k in ops}
            for _ in range(a.rounds):
                for k, f in ops.items():
                    ms[k].append(timed(f, a.launches) / a.launches)
            c, d = np.sort(np.array(ms["combine"])), np.sort(np.array(ms["demod"]))
            bytes_per_frame = K * 921600 + 230400
            row = dict(K=K, layout=layout_name, fps=n / np.median(c) * 1e3, fps_lo=n / c[-1] * 1e3, fps_hi=n / c[0] * 1e3, ms=float(np.median(c)),
                       frac=bytes_per_frame * n / (np.median(c) * 1e-3) / PEAK_BYTES_PER_S, demod_ms=float(np.median(d)), demod_lo=float(d[0]), demod_hi=float(d[-1]))
            rows.append(row)
            print(row, flush=True)
        del raw, dq
    ctx.close()
    name = torch.cuda.get_device_name(0)
    lines = ["# Receive diversity: combiner throughput", "",
             f"`python tools/bench_diversity.py --frames {n} --rounds {a.rounds} --launches {a.launches}` on {name}: `dabgpu_diversity_combine_frames` over K branches of {n} frames,",
             f"symbols_per_block 25, beside the K `dabgpu_ofdm_demod_frames_soft` launches (float loader, weighted policy, DQPSK view, symbols_per_block 25) that feed it, in the same run:",
             f"{a.rounds} alternating rounds of {a.launches} repetitions each after a 60 ms warm-up, device events.  Combiner: frames/s of the median round (slowest .. fastest round), the time of",
             "one launch, and its algorithmic bytes (K x 921,600 read + 230,400 written per frame) per second as a fraction of 8 TB/s -- a call rate over the HBM peak, not a",
             "profiled kernel time.  Demodulation: the time of the K launches of one batch, median (fastest .. slowest round).", "",
             "| branches | layout | combiner frames/s | combiner ms | of 8 TB/s | demodulation of the K branches, ms | combiner / demodulation |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['K']} | {r['layout']} | {r['fps']:,.0f} ({r['fps_lo']:,.0f} .. {r['fps_hi']:,.0f}) | {r['ms']:.3f} | {r['frac']:.3f} | "
                     f"{r['demod_ms']:.3f} ({r['demod_lo']:.3f} .. {r['demod_hi']:.3f}) | {r['ms'] / r['demod_ms']:.3f} |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
