#!/usr/bin/env python3
"""Call times of the sampling-clock tracker's two kernels beside the calls they stand next to.
  estimator    dabgpu_clock_estimate_frames (state in place, residual, sum, flag; no records) against dabgpu_sym_profile_frames (weights,
               noise, reference, flag) on the same products: both read the frames' 921,600 bytes of products once, in the same pattern,
               and write a few words.  The estimator loads every lag partner a second time, out of the cache.
  de-rotator   dabgpu_clock_derotate_frames out of place and in place against a device copy of the same bytes (Tensor.copy_): 921,600
               bytes read and as many written per frame.
The products are unit steps under noise with the ramp of 200 ppm on them, so that every frame is valid and rotated.  The calls of a
group are warmed up (untimed launches until 60 ms of kernels have run), then ROUNDS timed rounds ALTERNATE them, LAUNCHES repetitions
each, timed with device events; the figure is the median round, the spread its fastest and slowest round.  The fraction of the 8 TB/s
peak counts the products read once and what is written.

    python tools/bench_clock.py [--out profiles/tx/bench_clock.md] [--rounds 9] [--launches 4] [--frames 4096]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dab-radio_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
PEAK = 8.0e12
# hipcc -Rpass-analysis=kernel-resource-usage on csrc/clock.hip with the library's flags
RESOURCES = ("`clock_estimate_kernel`: 85 VGPRs, no scratch, 48 bytes of LDS per workgroup of 256, occupancy 5 waves per SIMD; one "
             "workgroup per frame, eighteen 16-byte loads in flight per thread.  `clock_derotate_kernel`: 80 VGPRs, no scratch, 12288 bytes of LDS, occupancy 6; "
             "a workgroup per run of rows, twelve 16-byte loads in flight per thread")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx", "bench_clock.md"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=4)
    ap.add_argument("--frames", default="4096")
    a = ap.parse_args()
    import numpy as np
    import torch
    import dabgpu
    assert torch.cuda.is_available(), "bench_clock needs the GPU: there is no CPU path to time"
    ctx = dabgpu.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(9733)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def group(ops):
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
    slope200 = dabgpu.clock_slope_q64(200.0)
    for n in [int(x) for x in a.frames.split(",")]:
        # unit steps on the diagonals under noise of deviation 0.1 per component, turned by the ramp of 200 ppm (de-rotating by -200)
        dq = torch.randn((n, 75, 1536, 2), dtype=torch.float32, device="cuda", generator=gen) * 0.1
        dq += (torch.randint(0, 2, (n, 75, 1536, 2), device="cuda", generator=gen).to(torch.float32) * 2.0 - 1.0) * 0.70710678
        ramp = torch.full((n,), -slope200, dtype=torch.int64, device="cuda")
        ctx.clock_derotate(dq, dq, n, ramp)
        out = torch.zeros_like(dq)
        state = torch.zeros((n,), dtype=torch.int64, device="cuda")
        res = torch.zeros((n,), dtype=torch.int64, device="cuda")
        corr = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
        ok = torch.zeros((n,), dtype=torch.int32, device="cuda")
        v = torch.zeros((n, 75), dtype=torch.float32, device="cuda")
        q = torch.zeros((n, 75), dtype=torch.float32, device="cuda")
        ref = torch.zeros((n,), dtype=torch.float32, device="cuda")
        sok = torch.zeros((n,), dtype=torch.int32, device="cuda")
        slope = torch.full((n,), slope200, dtype=torch.int64, device="cuda")
        ctx.clock_estimate(dq, n, slope_in=state, slope_out=state, residual=res, corr=corr, valid=ok)
        torch.cuda.synchronize()
        first = np.array([dabgpu.clock_ppm(int(s)) for s in state[:64].cpu().numpy()])
        assert int(ok.sum()) == n and np.abs(first - 200.0).max() < 2.0, first[:4]
        scratch = dq.clone()
        est = group({"clock": lambda: ctx.clock_estimate(dq, n, slope_in=state, slope_out=state, residual=res, corr=corr, valid=ok),
                     "sym": lambda: ctx.sym_profile(dq, n, symbol_weight=v, symbol_noise=q, ref_noise=ref, valid=sok)})
        rot = group({"derotate": lambda: ctx.clock_derotate(dq, out, n, slope),
                     "in_place": lambda: ctx.clock_derotate(scratch, scratch, n, slope),
                     "copy": lambda: out.copy_(dq)})
        torch.cuda.synchronize()
        g = dabgpu.clock_derotate_plan(dq, out, n, slope)
        read = n * 75 * 1536 * 8
        row = dict(n=n, est=est, rot=rot, spb=int(g.symbols_per_block),
                   frac_clock=float((read + n * 28) / (np.median(est["clock"]) * 1e-3) / PEAK),
                   frac_sym=float((read + n * (2 * 75 + 2) * 4) / (np.median(est["sym"]) * 1e-3) / PEAK),
                   frac_rot=float(2 * read / (np.median(rot["derotate"]) * 1e-3) / PEAK),
                   frac_in_place=float(2 * read / (np.median(rot["in_place"]) * 1e-3) / PEAK),
                   frac_copy=float(2 * read / (np.median(rot["copy"]) * 1e-3) / PEAK))
        rows.append(row)
        print({k: ({x: fmt(y) for x, y in val.items()} if isinstance(val, dict) else val) for k, val in row.items()}, flush=True)
        del dq, out, scratch
    ctx.close()
    name = torch.cuda.get_device_name(0)
    lines = ["# Sampling-clock tracker: call times", "",
             f"`python tools/bench_clock.py --frames {a.frames} --rounds {a.rounds} --launches {a.launches}` on {name}.  {a.rounds} alternating rounds of",
             f"{a.launches} repetitions each after a 60 ms warm-up, device events; ms of one call, the median round (fastest .. slowest round).  Call times of a warm loop,",
             "not profiled kernel times.  Fractions of 8 TB/s count the products once (921,600 bytes a frame) and what is written.", "",
             "Estimator: `dabgpu_clock_estimate_frames` (state in place, residual, sum, flag; no records) against `dabgpu_sym_profile_frames` (weights, noise,",
             "reference, flag) on the same products: the same bytes in the same pattern (profiles/tx/bench_sym_profile.md has that call at 1024 frames).", "",
             "| frames | clock ms | sym ms | clock / sym | frames/s | clock: of 8 TB/s | sym: of 8 TB/s |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} | {fmt(r['est']['clock'])} | {fmt(r['est']['sym'])} | {np.median(r['est']['clock']) / np.median(r['est']['sym']):.3f} | "
                     f"{r['n'] / (np.median(r['est']['clock']) * 1e-3):.3e} | {r['frac_clock']:.3f} | {r['frac_sym']:.3f} |")
    lines += ["", "De-rotator: `dabgpu_clock_derotate_frames` out of place and in place (the planner's run length) against `Tensor.copy_` of the same bytes.", "",
              "| frames | rows per workgroup | out of place ms | in place ms | copy ms | out of place / copy | frames/s | out of place: of 8 TB/s | in place: of 8 TB/s | copy: of 8 TB/s |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} | {r['spb']} | {fmt(r['rot']['derotate'])} | {fmt(r['rot']['in_place'])} | {fmt(r['rot']['copy'])} | "
                     f"{np.median(r['rot']['derotate']) / np.median(r['rot']['copy']):.3f} | {r['n'] / (np.median(r['rot']['derotate']) * 1e-3):.3e} | "
                     f"{r['frac_rot']:.3f} | {r['frac_in_place']:.3f} | {r['frac_copy']:.3f} |")
    lines += ["", "Resources.  " + RESOURCES + "."]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
