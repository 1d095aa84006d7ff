#!/usr/bin/env python3
"""Call time of the noise estimator (dabgpu_noise_estimate_frames) beside dabgpu_tii_bank_process -- the one existing launch with the same
window and transform -- at 1024 and 4096 frames per launch, in the same run.  The frames are white noise with a louder phase reference
symbol, 8192 samples apart (windows 16-byte aligned: the wide loader), no records; the estimator writes its four floats and the flag per
frame, the bank accumulates without a decision.  Both operations are warmed up (untimed launches until 60 ms of kernels have run), then
ROUNDS timed rounds ALTERNATE them, LAUNCHES repetitions each, timed with device events; the figure is the median round, the spread its
fastest and slowest round.  Algorithmic bytes per frame: the estimator reads the window and the symbol's useful part (2 x 16,384) and
writes 20; the bank reads the window (16,384) and reads and writes its 768-byte accumulator.

    python tools/bench_noise.py [--out profiles/tx/bench_noise.md] [--rounds 9] [--launches 8] [--frames 1024,4096]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dab-radio_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
PEAK_BYTES_PER_S = 8.0e12
STRIDE = 8192
NOISE_BYTES, TII_BYTES = 2 * 16384 + 20, 16384 + 2 * 768 + 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx", "bench_noise.md"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--frames", default="1024,4096")
    a = ap.parse_args()
    import numpy as np
    import torch
    import dabgpu
    assert torch.cuda.is_available(), "bench_noise needs the GPU: there is no CPU path to time"
    ctx = dabgpu.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(9800)
    rows = []
    for n in [int(x) for x in a.frames.split(",")]:
        iq = torch.randn((n, STRIDE, 2), dtype=torch.float32, device="cuda", generator=gen)
        iq[:, 2656:] *= 20.0
        out = {k: torch.zeros((n,), dtype=torch.float32, device="cuda") for k in ("noise_power", "signal_power", "weight", "snr")}
        valid = torch.zeros((n,), dtype=torch.int32, device="cuda")
        bank = dabgpu.TiiBank(ctx, n)

        def noise():
            ctx.noise_estimate(iq, n, STRIDE, 0, valid=valid, **out)

        def tii():
            bank.process(iq, STRIDE, 0)

        def timed(fn, reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        ops = {"noise": noise, "tii": tii}
        warm = 0.0
        while warm < 60.0:
            warm += sum(timed(f, 2) for f in ops.values())
        # what was timed is the estimate: every frame valid, the noise of two unit components per sample
        npow = out["noise_power"].cpu().numpy()
        assert int(valid.sum()) == n and abs(float(npow.mean()) / 2.0 - 1.0) < 0.01, (int(valid.sum()), float(npow.mean()))
        ms = {k: [] for k in ops}
        for _ in range(a.rounds):
            for k, f in ops.items():
                ms[k].append(timed(f, a.launches) / a.launches)
        c, d = np.sort(np.array(ms["noise"])), np.sort(np.array(ms["tii"]))
        row = dict(n=n, ms=float(np.median(c)), lo=float(c[0]), hi=float(c[-1]), tii_ms=float(np.median(d)), tii_lo=float(d[0]), tii_hi=float(d[-1]),
                   rate=NOISE_BYTES * n / (np.median(c) * 1e-3), tii_rate=TII_BYTES * n / (np.median(d) * 1e-3), mean_noise=float(npow.mean()),
                   dev=float(npow.std() / npow.mean()))
        rows.append(row)
        print(row, flush=True)
        bank.close()
        del iq
    ctx.close()
    name = torch.cuda.get_device_name(0)
    lines = ["# Noise estimate: call time", "",
             f"`python tools/bench_noise.py --frames {a.frames} --rounds {a.rounds} --launches {a.launches}` on {name}: `dabgpu_noise_estimate_frames`",
             f"(four floats and the flag per frame, no records, frames {STRIDE} samples apart, wide loader) beside `dabgpu_tii_bank_process` without a decision on the same buffer,",
             f"{a.rounds} alternating rounds of {a.launches} repetitions each after a 60 ms warm-up, device events: the median round (fastest .. slowest round).  Bytes over call time:",
             f"the algorithmic bytes of a frame ({NOISE_BYTES:,} for the estimate, {TII_BYTES:,} for the bank) per second of the call, and as a fraction of 8 TB/s -- a call rate, not a",
             "profiled kernel time.  Nothing comparable exists at the parent commit, so there is no bar; the ratio is the new call against the existing one, which reads half its bytes.", "",
             "| frames | estimate ms | bank ms | estimate / bank | estimate GB/s (of 8 TB/s) | bank GB/s (of 8 TB/s) | mean noise_power (2 put in), relative deviation |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} | {r['ms']:.4f} ({r['lo']:.4f} .. {r['hi']:.4f}) | {r['tii_ms']:.4f} ({r['tii_lo']:.4f} .. {r['tii_hi']:.4f}) | {r['ms'] / r['tii_ms']:.3f} | "
                     f"{r['rate'] / 1e9:,.0f} ({r['rate'] / PEAK_BYTES_PER_S:.3f}) | {r['tii_rate'] / 1e9:,.0f} ({r['tii_rate'] / PEAK_BYTES_PER_S:.3f}) | "
                     f"{r['mean_noise']:.4f}, {r['dev']:.4f} |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
