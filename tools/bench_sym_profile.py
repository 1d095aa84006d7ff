#!/usr/bin/env python3
"""Call times of the symbol noise profile and of the symbol-weighted combiner beside the calls they stand next to.
  estimator   dabgpu_sym_profile_frames (weights, noise, reference, flag; no records) against dabgpu_dd_profile_frames (state in place at
              alpha 0.25, band weights, mean, flag) on the same products: both read the frames' 921,600 bytes of products once and write
              well under 1 kB.  The mark: not slower than that call by more than 10 % (the margin is for the per-row wave sums).
  combiner    the one-branch dabgpu_diversity_combine_frames_symbols (band table and symbol table) against
              dabgpu_diversity_combine_frames_banded on the same inputs: 300 bytes per branch-frame of extra reads.  The mark: within
              +- 4 %, the box-to-box spread the README gives.
The products are unit steps at a level per carrier under noise, so that every frame is valid.  The calls of a pair are warmed up
(untimed launches until 60 ms of kernels have run), then ROUNDS timed rounds ALTERNATE them, LAUNCHES repetitions each, timed with
device events; the figure is the median round, the spread its fastest and slowest round.  The fraction of the 8 TB/s peak counts the
products read and the outputs written.

    python tools/bench_sym_profile.py [--out profiles/tx/bench_sym_profile.md] [--rounds 9] [--launches 8] [--frames 1024]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dab-radio_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
PEAK = 8.0e12
# hipcc -Rpass-analysis=kernel-resource-usage on csrc/sym_profile.hip and csrc/diversity.hip with the library's flags
RESOURCES = ("`sym_profile_kernel`: 63 VGPRs, 0 AGPRs, 106 SGPRs (68 of them kept in VGPR lanes), no scratch, 4512 bytes of LDS per workgroup of 256, "
             "occupancy 7 waves per SIMD; one workgroup per frame, fifteen 16-byte loads in flight per thread.  `diversity_combine_kernel<DV_SYMBOLS>`: "
             "70 VGPRs, 0 AGPRs, 98 SGPRs, no scratch, 6208 bytes of LDS, occupancy 7 (the banded instantiation: 68 VGPRs, 78 SGPRs, 6208 bytes, 7)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx", "bench_sym_profile.md"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--frames", default="1024")
    a = ap.parse_args()
    import numpy as np
    import torch
    import dabgpu
    assert torch.cuda.is_available(), "bench_sym_profile needs the GPU: there is no CPU path to time"
    ctx = dabgpu.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(9731)

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
        # unit steps of amplitude 1 on the diagonals under noise of deviation 0.2 per component, twice that on every eleventh row
        dq = torch.randn((n, 75, 1536, 2), dtype=torch.float32, device="cuda", generator=gen) * 0.2
        dq[:, ::11] *= 2.0
        dq += (torch.randint(0, 2, (n, 75, 1536, 2), device="cuda", generator=gen).to(torch.float32) * 2.0 - 1.0) * 0.70710678
        scale = torch.full((n,), 40.0, dtype=torch.float32, device="cuda")
        state = torch.zeros((n, 128), dtype=torch.float32, device="cuda")
        bw = torch.zeros((n, 128), dtype=torch.float32, device="cuda")
        mean = torch.zeros((n,), dtype=torch.float32, device="cuda")
        valid = torch.zeros((n,), dtype=torch.int32, device="cuda")
        v = torch.zeros((n, 75), dtype=torch.float32, device="cuda")
        q = torch.zeros((n, 75), dtype=torch.float32, device="cuda")
        ref = torch.zeros((n,), dtype=torch.float32, device="cuda")
        ok = torch.zeros((n,), dtype=torch.int32, device="cuda")
        out = torch.zeros((n, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
        k_out = torch.zeros((n,), dtype=torch.float32, device="cuda")
        table = dabgpu.diversity_table([(dq, scale)])
        dd = lambda: ctx.dd_profile(dq, n, profile_in=state, alpha=0.25, profile_out=state, band_weight=bw, mean_noise=mean, valid=valid)
        sym = lambda: ctx.sym_profile(dq, n, symbol_weight=v, symbol_noise=q, ref_noise=ref, valid=ok)
        dd()
        sym()
        est = pair({"sym": sym, "dd": dd})
        comb = pair({"symbols": lambda: ctx.diversity_combine(table, n, out, soft_scale=k_out, band_weights=[bw], symbol_weights=[v]),
                     "banded": lambda: ctx.diversity_combine(table, n, out, soft_scale=k_out, band_weights=[bw])})
        torch.cuda.synchronize()
        assert int(valid.sum()) == n and int(ok.sum()) == n and float(k_out.min()) > 0
        vv = v.cpu().numpy()
        read = n * 75 * 1536 * 8
        row = dict(n=n, est=est, comb=comb, v_min=float(vv.min()), ones=float((vv == 1).sum(axis=1).mean()),
                   frac_sym=float((read + n * (2 * 75 + 2) * 4) / (np.median(est["sym"]) * 1e-3) / PEAK),
                   frac_dd=float((read + n * (2 * 128 + 2) * 4 + n * 128 * 4) / (np.median(est["dd"]) * 1e-3) / PEAK),
                   frac_symbols=float((read + n * (128 + 75) * 4 + n * dabgpu.NB_FRAME_BITS) / (np.median(comb["symbols"]) * 1e-3) / PEAK),
                   frac_banded=float((read + n * 128 * 4 + n * dabgpu.NB_FRAME_BITS) / (np.median(comb["banded"]) * 1e-3) / PEAK))
        rows.append(row)
        print({k: ({x: fmt(y) for x, y in val.items()} if isinstance(val, dict) else val) for k, val in row.items()}, flush=True)
        del dq, out
    ctx.close()
    name = torch.cuda.get_device_name(0)
    lines = ["# Symbol noise profile and symbol-weighted combiner: call times", "",
             f"`python tools/bench_sym_profile.py --frames {a.frames} --rounds {a.rounds} --launches {a.launches}` on {name}.  {a.rounds} alternating rounds of",
             f"{a.launches} repetitions each after a 60 ms warm-up, device events; ms of one call, the median round (fastest .. slowest round).  Call times of a warm loop,",
             "not profiled kernel times.", "",
             "Estimator: `dabgpu_sym_profile_frames` (weights, noise, reference, flag; no records) against `dabgpu_dd_profile_frames` (state in place at alpha 0.25,",
             "band weights, mean, flag) on the same products.  Both read 921,600 bytes of products per frame once.  The mark: sym / dd <= 1.10.", "",
             "| frames | sym ms | dd ms | sym / dd | sym: of 8 TB/s | dd: of 8 TB/s | smallest weight | rows of weight 1 per frame |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} | {fmt(r['est']['sym'])} | {fmt(r['est']['dd'])} | {np.median(r['est']['sym']) / np.median(r['est']['dd']):.3f} | {r['frac_sym']:.3f} | "
                     f"{r['frac_dd']:.3f} | {r['v_min']:.3f} | {r['ones']:.1f} |")
    lines += ["", "Combiner: the one-branch `dabgpu_diversity_combine_frames_symbols` (band table and symbol table) against `dabgpu_diversity_combine_frames_banded` on",
              "the same products and band weights (default symbols_per_block, natural layout).  The mark: symbols / banded within 1 +- 0.04.", "",
              "| frames | symbols ms | banded ms | symbols / banded | symbols: of 8 TB/s | banded: of 8 TB/s |", "|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} | {fmt(r['comb']['symbols'])} | {fmt(r['comb']['banded'])} | {np.median(r['comb']['symbols']) / np.median(r['comb']['banded']):.3f} | "
                     f"{r['frac_symbols']:.3f} | {r['frac_banded']:.3f} |")
    lines += ["", f"Resources.  {RESOURCES}."]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
