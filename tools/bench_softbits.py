#!/usr/bin/env python3
"""Frames per second of the two soft-decision policies of the mode I demodulator through dabgpu_ofdm_demod_frames_soft: 1024 and 4096
frames, the float and the u8 loader, the natural and the class-order layout.  Per shape: both policies are warmed up (untimed launches
until 60 ms of kernels have run), then ROUNDS timed rounds that ALTERNATE the policies, LAUNCHES launches each, timed with device events; the
figure is the median round, the spread its fastest and slowest round.  symbols_per_block is given (25) so that no tuning state enters.

    python tools/bench_softbits.py [--out profiles/tx/bench_softbits.md] [--rounds 9] [--launches 8]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dab-radio_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx", "bench_softbits.md"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--frames", default="1024,4096")
    a = ap.parse_args()
    import numpy as np
    import torch
    import dabgpu
    assert torch.cuda.is_available(), "bench_softbits needs the GPU: there is no CPU path to time"
    ctx = dabgpu.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(9320)
    rows = []
    for n in [int(x) for x in a.frames.split(",")]:
        bits = torch.zeros((n, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
        corr = torch.zeros((n, 76, 2), dtype=torch.float32, device="cuda")
        scale = torch.zeros((n,), dtype=torch.float32, device="cuda")
        for fmt_name in ("raw_f32l", "raw_u8"):
            fmt = dabgpu.IQ_FORMATS.index(fmt_name)
            if fmt_name == "raw_f32l":
                raw = torch.randn((n, dabgpu.NB_FRAME_SAMPLES, 2), dtype=torch.float32, device="cuda", generator=gen)
            else:
                raw = torch.randint(0, 256, (n, dabgpu.NB_FRAME_SAMPLES, 2), dtype=torch.uint8, device="cuda", generator=gen)
            for layout, layout_name in ((dabgpu.BITS_NATURAL, "natural"), (dabgpu.BITS_MSC_CLASSED, "class order")):
                cfgs = {"normalised": dabgpu.SoftCfg(dabgpu.SOFT_NORMALISED, 64.0), "csi": dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0)}

                def launch(cfg):
                    ctx.ofdm_demod_frames_soft(raw, fmt, n, bits, cfg, cp_corr=corr, symbols_per_block=25, bits_layout=layout, soft_scale=scale)

                def timed(cfg, k):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(k):
                        launch(cfg)
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1)
                warm = 0.0
                while warm < 60.0:
                    warm += sum(timed(c, 2) for c in cfgs.values())
                ms = {k: [] for k in cfgs}
                for _ in range(a.rounds):
                    for k, c in cfgs.items():
                        ms[k].append(timed(c, a.launches) / a.launches)
                row = [n, fmt_name, layout_name]
                for k in cfgs:
                    v = np.sort(np.array(ms[k]))
                    row += [n / np.median(v) * 1e3, n / v[-1] * 1e3, n / v[0] * 1e3]
                row.append(np.median(ms["normalised"]) / np.median(ms["csi"]))
                rows.append(row)
                print(row, flush=True)
            del raw
    ctx.close()
    name = torch.cuda.get_device_name(0)
    lines = ["# Soft-decision policies: demodulator throughput", "",
             f"`tools/bench_softbits.py` on {name}: `dabgpu_ofdm_demod_frames_soft`, symbols_per_block 25, {a.rounds} alternating rounds of {a.launches} launches per policy after a",
             "60 ms warm-up, device events.  Frames/s: median round (slowest .. fastest round).  Ratio: weighted over normalised (above 1 = the weighted policy is faster).", "",
             "| frames | loader | layout | normalised | weighted (csi) | ratio |", "|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]:,.0f} ({r[4]:,.0f} .. {r[5]:,.0f}) | {r[6]:,.0f} ({r[7]:,.0f} .. {r[8]:,.0f}) | {r[9]:.3f} |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
