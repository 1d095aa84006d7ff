#!/usr/bin/env python3
"""What the stream bank's DQPSK products cost (dabgpu_stream_bank_set_products): three banks of the same library -- normalised, weighted
(DABGPU_SOFT_CSI with a scale buffer), weighted with products and records -- fed the same blocks of two frame periods per stream in
rounds that ALTERNATE the three, for 256 and 4096 streams in raw_u8 and complex float.  Reported: the median round of nine and the
spread, the ratio of the weighted bank to the one with products, and the algorithmic bytes per frame of the latter (the frame read in
its capture format + 230,400 soft bits + 921,600 bytes of products) over its median time.

    python tools/bench_stream_products.py [--streams 256,4096] [--rounds 9] [--out profiles/tx/bench_stream_products.md]

The streams are tools/bench_stream.py's (--compare-soft): one frame period long and periodic, so that the same block is the continuation
of itself and every call completes two frames per stream."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dab-radio_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dabgpu  # noqa: E402
from bench_stream import synth_frames  # noqa: E402

L = 196608
BITS_BYTES, PRODUCT_BYTES = 230400, 75 * 1536 * 8
KINDS = ("normalised", "weighted", "products")


def periodic_streams(E, dev):
    """[E][2 L] complex64: tools/bench_stream.py's periodic streams (own timing, a carrier offset of whole cycles per frame, noise that
    repeats with the frame), two periods of each"""
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    frame = synth_frames(E, dev, g)
    shift = torch.randint(0, L, (E,), generator=g, device=dev)
    cycles = torch.randint(-393, 394, (E,), generator=g, device=dev)               # |offset| <= 0.002 cycles per sample
    idx = torch.arange(L, device=dev)
    stream = torch.empty((E, 2 * L), dtype=torch.complex64, device=dev)
    one = stream[:, :L]
    for e in range(E):
        ph = (int(cycles[e]) * idx) % L
        one[e] = torch.roll(frame[e], -int(shift[e])) * torch.polar(torch.ones(L, device=dev), (2 * np.pi / L) * ph.float())
    del frame
    for e0 in range(0, E, 256):                                                     # (in pieces: the noise of 4096 streams at once is 6 GB more)
        m = min(256, E - e0)
        one[e0:e0 + m] += 0.02 * torch.view_as_complex(torch.randn((m, L, 2), generator=g, dtype=torch.float32, device=dev)) * 0.70710678
    stream[:, L:] = one
    return stream


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="256,4096")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--soft-level", type=float, default=64.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx", "bench_stream_products.md"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = dabgpu.Context(0)
    n_block = 2 * L
    max_frames = n_block // 191400 + 2
    rows = []
    for E in [int(x) for x in args.streams.split(",")]:
        stream = periodic_streams(E, dev)
        sv = torch.view_as_real(stream)
        peak = float(sv.abs().max().item())
        raw_u8 = torch.empty((E, 2 * L, 2), dtype=torch.uint8, device=dev)
        for e0 in range(0, E, 256):
            raw_u8[e0:e0 + 256] = torch.clamp(torch.round(sv[e0:e0 + 256] / peak * 127.0 + 127.5), 0, 255).to(torch.uint8)
        inputs = {"raw_u8": raw_u8, "raw_f32l": sv}
        bits = torch.zeros((E, max_frames, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device=dev)
        nf = torch.zeros(E, dtype=torch.int32, device=dev)
        scale = torch.zeros(E * max_frames, dtype=torch.float32, device=dev)
        dq = torch.zeros((E * max_frames, 75, 1536, 2), dtype=torch.float32, device=dev)
        rec = torch.zeros((E * max_frames, 6), dtype=torch.int32, device=dev)
        for name in ("raw_u8", "raw_f32l"):
            fmt, raw = dabgpu.IQ_FORMATS.index(name), inputs[name]
            banks = {k: dabgpu.StreamBank(ctx, E) for k in KINDS}
            banks["weighted"].set_soft(dabgpu.SoftCfg(dabgpu.SOFT_CSI, args.soft_level), scale)
            banks["products"].set_soft(dabgpu.SoftCfg(dabgpu.SOFT_CSI, args.soft_level), scale)
            banks["products"].set_products(dq, rec)

            def call(bank):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                bank.process_raw(raw, fmt, n_block, n_block, bits, max_frames, nf)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3, int(nf.sum().item())
            for _ in range(3):                                                   # acquisition, then the steady state
                for b in banks.values():
                    call(b)
            ms, got, last = {k: [] for k in banks}, {k: 0 for k in banks}, 0
            for _ in range(args.rounds):
                for k, b in banks.items():
                    t, n_ = call(b)
                    ms[k].append(t)
                    got[k] += n_
                    last = n_                                                    # (the bank with products runs last in a round)
            assert got["normalised"] == got["weighted"] == got["products"], "neither the policy nor the products change a frame count"
            assert int(rec.view(-1, 6)[:, 4].sum().item()) == last, "a valid record per frame the last call completed"
            desync = {k: int(b.status()["total_frames_desync"].sum()) for k, b in banks.items()}
            for b in banks.values():
                b.close()
            frames = got["products"] / args.rounds
            med = {k: float(np.median(ms[k])) for k in KINDS}
            per_frame = L * dabgpu.iq_format_sample_bytes(fmt) + BITS_BYTES + PRODUCT_BYTES
            row = dict(streams=E, format=name, frames_per_call=frames, desync=desync,
                       ms={k: [med[k], float(min(ms[k])), float(max(ms[k]))] for k in KINDS},
                       weighted_over_products=med["weighted"] / med["products"], bytes_per_frame=per_frame,
                       products_gb_per_s=frames * per_frame / (med["products"] * 1e-3) / 1e9)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del stream, sv, raw_u8, inputs, bits, nf, scale, dq, rec
        torch.cuda.empty_cache()
    ctx.close()
    lines = ["# Stream bank: what the DQPSK products cost", "",
             f"`tools/bench_stream_products.py` on {torch.cuda.get_device_name(0)}: three banks of the same library -- normalised, weighted (level {args.soft_level:g}, with a",
             "scale buffer), weighted with products and records (`dabgpu_stream_bank_set_products`) -- fed the same blocks of two frame periods per",
             f"stream (`dabgpu_stream_bank_process_raw`, three acquisition calls each, then {args.rounds} rounds that alternate the three; wall clock around a call,",
             "which synchronises).  ms per call: median round (fastest .. slowest).  Ratio: weighted over weighted with products (below 1 = the",
             "products cost time).  Bytes per frame: the frame read in its capture format + 230,400 soft bits + 921,600 bytes of products; GB/s:",
             "those bytes of the call's frames over the median time of the bank with products.", "",
             "| streams | format | frames per call | normalised ms | weighted ms | with products ms | ratio | bytes per frame | GB/s |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        cell = {k: f"{v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f})" for k, v in r["ms"].items()}
        lines.append(f"| {r['streams']} | {r['format']} | {r['frames_per_call']:.0f} | {cell['normalised']} | {cell['weighted']} | {cell['products']} | "
                     f"{r['weighted_over_products']:.3f} | {r['bytes_per_frame']:,} | {r['products_gb_per_s']:.0f} |")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
