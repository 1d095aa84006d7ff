#!/usr/bin/env python3
"""Rate of the resampler (dabgpu_resample_bank_apply, dab-radio_amd/csrc/resample.hip) on one MI355X: N streams x one mode I frame of
output, complex float out, for a clock error of 20 ppm (step 1 + 2e-5: a block touches a handful of table rows) and for a 2.4 MS/s capture
brought to 2.048 MS/s (step 1.171875: every row), the identity stream (a copy) beside them; the median of --reps calls timed with HIP
events.  Algorithmic bytes per output sample: 8 written + 8 x step read; shares are of 8 TB/s.  Per output the kernel executes 3 x taps
FMAs (one for the coefficient, two for the sample).
    python tools/bench_resample.py [--streams 4096] [--reps 30] [--out profiles/tx/bench_resample.md]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx", "bench_resample.md"))
    a = ap.parse_args()
    import torch
    import dabgpu
    N, S = a.streams, dabgpu.NB_FRAME_SAMPLES
    ctx = dabgpu.Context(0)
    n_in = (int(S * 2.4 / 2.048) + 64) & ~1
    x = torch.randn((N, n_in, 2), dtype=torch.float32, device="cuda")
    out = torch.empty((N, S, 2), dtype=torch.float32, device="cuda")
    cases = [("identity (copy path)", dabgpu.resample_step()), ("2.048 MS/s + 20 ppm", dabgpu.resample_step(ppm=20.0)),
             ("2.4 -> 2.048 MS/s", dabgpu.resample_step(2.4e6, 2.048e6))]
    rows = []
    for name, step in cases:
        rs = dabgpu.Resampler(ctx, [dabgpu.resample_stream(step, offset=0.25 if step != 1 << 62 else 0.0) for _ in range(N)])
        ms = median_ms(lambda: rs.apply(x, n_in, S, out, in_stride_samples=n_in, wrap=True), a.reps)
        ratio = step * 2.0 ** -62
        gbs = N * S * (8 + 8 * ratio) / ms / 1e6
        flops = 0.0 if step == 1 << 62 else N * S * 3 * dabgpu.RESAMPLE_TAPS * 2 / ms / 1e9
        rows.append((name, rs.plan["table_rows"], rs.plan["lds_bytes"], ms, N * S / ms / 1e6, gbs, gbs / 8000 * 100, flops, rs.design.error))
        rs.close()
    text = [f"# Resampler: {N} streams x one mode I frame of output ({S} samples), complex float, median of {a.reps} calls (HIP events)", "",
            f"Device: {torch.cuda.get_device_properties(0).gcnArchName} ({torch.cuda.get_device_name(0)}).  Measured on one MI355X by tools/bench_resample.py.", "",
            "| case | table rows staged | LDS bytes | ms / call | G samples / s | GB/s (algorithmic) | % of 8 TB/s | TFLOP/s (3 x taps FMA) | design error |",
            "|---|---|---|---|---|---|---|---|---|"]
    text += [f"| {n} | {r} | {l} | {ms:.3f} | {sps:.1f} | {g:.0f} | {p:.1f} | {f:.1f} | {e:.2e} |" for n, r, l, ms, sps, g, p, f, e in rows]
    text = "\n".join(text) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
