#!/usr/bin/env python3
"""Call times of the noise profile and of the banded combiner beside the calls they stand next to.  (1) dabgpu_noise_profile_frames
(state in place, band weights, mean and flag; no records, frames 8192 samples apart, wide loader) against
dabgpu_noise_estimate_frames on the same buffer of white noise: the same front half, less behind it.  (2)
dabgpu_diversity_combine_frames_banded with a table on every branch against dabgpu_diversity_combine_frames with a scalar weight on
every branch, on the same products (random, scales 40): K = 1, 2, 4, symbols_per_block 25, natural layout.  Both operations of a pair
are warmed up (untimed launches until 60 ms of kernels have run), then ROUNDS timed rounds ALTERNATE them, LAUNCHES repetitions each,
timed with device events; the figure is the median round, the spread its fastest and slowest round.

    python tools/bench_noise_profile.py [--out profiles/tx/bench_noise_profile.md] [--rounds 9] [--launches 8] [--frames 1024,4096]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dab-radio_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
STRIDE = 8192


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx", "bench_noise_profile.md"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--frames", default="1024,4096")
    ap.add_argument("--branches", default="1,2,4")
    ap.add_argument("--combiner-frames", type=int, default=1024)
    a = ap.parse_args()
    import numpy as np
    import torch
    import dabgpu
    assert torch.cuda.is_available(), "bench_noise_profile needs the GPU: there is no CPU path to time"
    ctx = dabgpu.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(9720)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def pair(ops):
        """{name: sorted ms per launch over the rounds} of operations timed in alternation"""
        warm = 0.0
        while warm < 60.0:
            warm += sum(timed(f, 2) for f in ops.values())
        ms = {k: [] for k in ops}
        for _ in range(a.rounds):
            for k, f in ops.items():
                ms[k].append(timed(f, a.launches) / a.launches)
        return {k: np.sort(np.array(v)) for k, v in ms.items()}

    def fmt(v):
        return f"{np.median(v):.4f} ({v[0]:.4f} .. {v[-1]:.4f})"

    prof_rows = []
    for n in [int(x) for x in a.frames.split(",")]:
        iq = torch.randn((n, STRIDE, 2), dtype=torch.float32, device="cuda", generator=gen)                  # power 2 per complex sample
        state = torch.zeros((n, 128), dtype=torch.float32, device="cuda")
        bw = torch.zeros((n, 128), dtype=torch.float32, device="cuda")
        mean = torch.zeros((n,), dtype=torch.float32, device="cuda")
        valid = torch.zeros((n,), dtype=torch.int32, device="cuda")
        outs = [torch.zeros((n,), dtype=torch.float32, device="cuda") for _ in range(4)]
        ms = pair({"profile": lambda: ctx.noise_profile(iq, n, STRIDE, 0, profile_in=state, alpha=0.25, profile_out=state, band_weight=bw, mean_noise=mean,
                                                        valid=valid),
                   "estimate": lambda: ctx.noise_estimate(iq, n, STRIDE, 0, noise_power=outs[0], signal_power=outs[1], weight=outs[2], snr=outs[3], valid=valid)})
        torch.cuda.synchronize()
        assert int(valid.sum()) == n
        m = mean.cpu().numpy()
        row = dict(n=n, profile=ms["profile"], estimate=ms["estimate"], mean=float(m.mean()), dev=float(m.std() / m.mean()))
        prof_rows.append(row)
        print({k: (fmt(v) if hasattr(v, "shape") else v) for k, v in row.items()}, flush=True)
        del iq
    comb_rows = []
    n = a.combiner_frames
    for K in [int(x) for x in a.branches.split(",")]:
        dq = [torch.randn((n, 75, 1536, 2), dtype=torch.float32, device="cuda", generator=gen) for _ in range(K)]
        scale = [torch.full((n,), 40.0, dtype=torch.float32, device="cuda") for _ in range(K)]
        w = [torch.rand((n,), dtype=torch.float32, device="cuda", generator=gen) + 0.5 for _ in range(K)]
        bands = [torch.rand((n, 128), dtype=torch.float32, device="cuda", generator=gen) + 0.5 for _ in range(K)]
        out = torch.zeros((n, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
        k_out = torch.zeros((n,), dtype=torch.float32, device="cuda")
        scalar = dabgpu.diversity_table([(dq[b], scale[b], w[b]) for b in range(K)])
        plain = dabgpu.diversity_table([(dq[b], scale[b]) for b in range(K)])
        ms = pair({"scalar": lambda: ctx.diversity_combine(scalar, n, out, symbols_per_block=25, soft_scale=k_out),
                   "banded": lambda: ctx.diversity_combine(plain, n, out, symbols_per_block=25, soft_scale=k_out, band_weights=bands)})
        torch.cuda.synchronize()
        assert float(k_out.min()) > 0
        row = dict(K=K, scalar=ms["scalar"], banded=ms["banded"])
        comb_rows.append(row)
        print({k: (fmt(v) if hasattr(v, "shape") else v) for k, v in row.items()}, flush=True)
        del dq
    ctx.close()
    name = torch.cuda.get_device_name(0)
    lines = ["# Noise profile and banded combiner: call times", "",
             f"`python tools/bench_noise_profile.py --frames {a.frames} --rounds {a.rounds} --launches {a.launches}` on {name}.  Each pair of calls: {a.rounds} alternating rounds of",
             f"{a.launches} repetitions each after a 60 ms warm-up, device events; ms of one call, the median round (fastest .. slowest round).  Call times of a warm loop,",
             "not profiled kernel times.", "",
             "`dabgpu_noise_profile_frames` (state in place at alpha 0.25, band weights, mean, flag; no records, frames 8192 samples apart) against",
             "`dabgpu_noise_estimate_frames` (four floats and the flag) on the same buffer of white noise of power 2 per sample:", "",
             "| frames | profile ms | estimate ms | profile / estimate | mean of d_mean_noise (2 put in), relative deviation (derived 0.0255) |", "|---|---|---|---|---|"]
    for r in prof_rows:
        lines.append(f"| {r['n']} | {fmt(r['profile'])} | {fmt(r['estimate'])} | {np.median(r['profile']) / np.median(r['estimate']):.3f} | {r['mean']:.4f}, {r['dev']:.4f} |")
    lines += ["", f"`dabgpu_diversity_combine_frames_banded` (a table on every branch) against `dabgpu_diversity_combine_frames` (a scalar weight on every branch), {n} frames,",
              "symbols_per_block 25, natural layout, the same products:", "", "| branches | banded ms | scalar ms | banded / scalar |", "|---|---|---|---|"]
    for r in comb_rows:
        lines.append(f"| {r['K']} | {fmt(r['banded'])} | {fmt(r['scalar'])} | {np.median(r['banded']) / np.median(r['scalar']):.3f} |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
