#!/usr/bin/env python3
"""Call time of the decision-directed noise profile beside the call it feeds.  dabgpu_dd_profile_frames (state in place at alpha 0.25,
band weights, mean and flag; no records) against the one-branch dabgpu_diversity_combine_frames_banded call on the same products with
the band weights the profile wrote: both read the frames' 921,600 bytes of products once, the combiner writes 230,400 bytes of soft bits
per frame more.  The mark: the profile is not slower than that call.  The products are unit steps at a level per carrier under noise, so
that every frame is valid.  Both calls are warmed up (untimed launches until 60 ms of kernels have run), then ROUNDS timed rounds
ALTERNATE them, LAUNCHES repetitions each, timed with device events; the figure is the median round, the spread its fastest and slowest
round.  The fraction of the 8 TB/s peak counts the products read and the outputs written.

    python tools/bench_dd_profile.py [--out profiles/tx/bench_dd_profile.md] [--rounds 9] [--launches 8] [--frames 1024]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dab-radio_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
PEAK = 8.0e12
# hipcc -Rpass-analysis=kernel-resource-usage on csrc/dd_profile.hip with the library's flags
RESOURCES = "65 VGPRs, 0 AGPRs, 44 SGPRs, no scratch, 6152 bytes of LDS per workgroup of 256, occupancy 7 waves per SIMD"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx", "bench_dd_profile.md"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--frames", default="1024")
    a = ap.parse_args()
    import numpy as np
    import torch
    import dabgpu
    assert torch.cuda.is_available(), "bench_dd_profile needs the GPU: there is no CPU path to time"
    ctx = dabgpu.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(9730)

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

    rows = []
    for n in [int(x) for x in a.frames.split(",")]:
        # unit steps of amplitude 1 on the diagonals under noise of deviation 0.2 per component: Q about 0.04 everywhere
        dq = torch.randn((n, 75, 1536, 2), dtype=torch.float32, device="cuda", generator=gen) * 0.2
        dq += (torch.randint(0, 2, (n, 75, 1536, 2), device="cuda", generator=gen).to(torch.float32) * 2.0 - 1.0) * 0.70710678
        scale = torch.full((n,), 40.0, dtype=torch.float32, device="cuda")
        state = torch.zeros((n, 128), dtype=torch.float32, device="cuda")
        bw = torch.zeros((n, 128), dtype=torch.float32, device="cuda")
        mean = torch.zeros((n,), dtype=torch.float32, device="cuda")
        valid = torch.zeros((n,), dtype=torch.int32, device="cuda")
        out = torch.zeros((n, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
        k_out = torch.zeros((n,), dtype=torch.float32, device="cuda")
        table = dabgpu.diversity_table([(dq, scale)])
        ctx.dd_profile(dq, n, profile_in=state, alpha=0.25, profile_out=state, band_weight=bw, mean_noise=mean, valid=valid)
        ms = pair({"profile": lambda: ctx.dd_profile(dq, n, profile_in=state, alpha=0.25, profile_out=state, band_weight=bw, mean_noise=mean, valid=valid),
                   "combiner": lambda: ctx.diversity_combine(table, n, out, soft_scale=k_out, band_weights=[bw])})
        torch.cuda.synchronize()
        assert int(valid.sum()) == n and float(k_out.min()) > 0
        m = mean.cpu().numpy()
        read = n * 75 * 1536 * 8
        row = dict(n=n, profile=ms["profile"], combiner=ms["combiner"], mean=float(m.mean()),
                   frac_profile=float((read + n * (2 * 128 + 2) * 4 + n * 128 * 4) / (np.median(ms["profile"]) * 1e-3) / PEAK),
                   frac_combiner=float((read + n * 128 * 4 + n * dabgpu.NB_FRAME_BITS) / (np.median(ms["combiner"]) * 1e-3) / PEAK))
        rows.append(row)
        print({k: (fmt(v) if hasattr(v, "shape") else v) for k, v in row.items()}, flush=True)
        del dq, out
    ctx.close()
    name = torch.cuda.get_device_name(0)
    lines = ["# Decision-directed noise profile: call time", "",
             f"`python tools/bench_dd_profile.py --frames {a.frames} --rounds {a.rounds} --launches {a.launches}` on {name}.  {a.rounds} alternating rounds of",
             f"{a.launches} repetitions each after a 60 ms warm-up, device events; ms of one call, the median round (fastest .. slowest round).  Call times of a warm loop,",
             "not profiled kernel times.", "",
             "`dabgpu_dd_profile_frames` (state in place at alpha 0.25, band weights, mean, flag; no records) against the one-branch",
             "`dabgpu_diversity_combine_frames_banded` call on the same products with the weights the profile wrote (default symbols_per_block, natural layout).",
             "Both read 921,600 bytes of products per frame once; the combiner writes 230,400 bytes of soft bits per frame more.  The mark: profile / combiner <= 1.", "",
             "| frames | profile ms | combiner ms | profile / combiner | profile: of 8 TB/s | combiner: of 8 TB/s | mean of d_mean_noise |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} | {fmt(r['profile'])} | {fmt(r['combiner'])} | {np.median(r['profile']) / np.median(r['combiner']):.3f} | {r['frac_profile']:.3f} | "
                     f"{r['frac_combiner']:.3f} | {r['mean']:.3e} |")
    lines += ["", f"Resources of `dd_profile_kernel`: {RESOURCES}.  One workgroup per frame, fifteen 16-byte loads in flight per thread."]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
