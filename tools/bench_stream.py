#!/usr/bin/env python3
"""Throughput of the device-side unsynchronised front end (dabgpu_stream_bank_*): E receivers, each fed a continuous
synthetic Mode-I stream (own carrier offset and timing) in blocks, on one MI355X.

    python tools/bench_stream.py [--streams 256] [--block-frames 2] [--calls 6] [--soft-bits normalised|csi [--soft-level 64]]

--compare-soft times the weighted soft bits (dabgpu_stream_bank_set_soft, DABGPU_SOFT_CSI) against the normalised ones of the same
library: two banks fed the same blocks, rounds that ALTERNATE the policies, the median round and the spread, for 256 and 4096 streams
in raw_u8 and complex float; the table goes to profiles/tx/bench_stream_softbits.md.

    python tools/bench_stream.py --compare-soft [--compare-streams 256,4096] [--rounds 9] [--out profiles/tx/bench_stream_softbits.md]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dab-radio_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dabgpu  # noqa: E402


def synth_frames(E, dev, g):
    """one transmission frame per stream (NULL + PRS + 75 random QPSK symbols): a legal signal when repeated back to back"""
    prs, mapper, _ = dabgpu.host_tables()
    mp = torch.from_numpy(mapper.astype(np.int64)).to(dev)
    bins = torch.where(mp < 768, mp + (2048 - 768), mp - 768 + 1)
    prs_t = torch.from_numpy(prs).to(dev)
    L = 196608
    frame = torch.zeros((E, L), dtype=torch.complex64, device=dev)
    a = 0.70710678
    for e0 in range(0, E, 32):
        m = min(32, E - e0)
        b = torch.randint(0, 2, (m, 75, 3072), generator=g, device=dev, dtype=torch.uint8)
        z = torch.complex((1.0 - 2.0 * b[:, :, :1536].float()) * a, (1.0 - 2.0 * b[:, :, 1536:].float()) * a)
        spec = torch.zeros((m, 76, 2048), dtype=torch.complex64, device=dev)
        spec[:, 0] = prs_t
        cur = prs_t[bins].expand(m, -1).clone()
        for s_ in range(75):
            cur = cur * z[:, s_]
            spec[:, s_ + 1, bins] = cur
        t = torch.fft.ifft(spec, dim=2) * (2048.0 / 39.2)
        body = frame[e0:e0 + m, 2656:].view(m, 76, 2552)
        body[:, :, 504:] = t
        body[:, :, :504] = t[:, :, 2048 - 504:]
    return frame


def compare_soft(args):
    """both policies on the same blocks.  Every stream is one frame period long and periodic (its carrier offset is a whole number of cycles
    per frame, the noise repeats with the frame), so the same block of 196608 samples is the continuation of itself: a call completes one
    frame per stream, whatever the number of calls, and a bank of 4096 float streams needs no more input than 6.4 GB"""
    dev = torch.device("cuda", 0)
    ctx = dabgpu.Context(0)
    L = 196608
    rows = []
    for E in [int(x) for x in args.compare_streams.split(",")]:
        g = torch.Generator(device=dev)
        g.manual_seed(3)
        frame = synth_frames(E, dev, g)
        shift = torch.randint(0, L, (E,), generator=g, device=dev)
        cycles = torch.randint(-393, 394, (E,), generator=g, device=dev)           # |offset| <= 0.002 cycles per sample
        idx = torch.arange(L, device=dev)
        stream = torch.empty((E, L), dtype=torch.complex64, device=dev)
        for e in range(E):
            ph = (int(cycles[e]) * idx) % L
            stream[e] = torch.roll(frame[e], -int(shift[e])) * torch.polar(torch.ones(L, device=dev), (2 * np.pi / L) * ph.float())
        stream += 0.02 * torch.view_as_complex(torch.randn(stream.shape + (2,), generator=g, dtype=torch.float32, device=dev)) * 0.70710678
        del frame
        sv = torch.view_as_real(stream)
        peak = float(sv.abs().max().item())
        inputs = {"raw_u8": torch.clamp(torch.round(sv / peak * 127.0 + 127.5), 0, 255).to(torch.uint8), "raw_f32l": sv}
        max_frames = L // 191400 + 2
        for name in ("raw_u8", "raw_f32l"):
            fmt, raw = dabgpu.IQ_FORMATS.index(name), inputs[name]
            bits = torch.zeros((E, max_frames, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device=dev)
            nf = torch.zeros(E, dtype=torch.int32, device=dev)
            scale = torch.zeros(E * max_frames, dtype=torch.float32, device=dev)
            banks = {"normalised": dabgpu.StreamBank(ctx, E), "csi": dabgpu.StreamBank(ctx, E)}
            banks["csi"].set_soft(dabgpu.SoftCfg(dabgpu.SOFT_CSI, args.soft_level), scale)

            def call(bank):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                bank.process_raw(raw, fmt, L, L, bits, max_frames, nf)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3, int(nf.sum().item())
            for _ in range(3):                                                   # acquisition, then the steady state
                for b in banks.values():
                    call(b)
            ms, got = {k: [] for k in banks}, {k: 0 for k in banks}
            for _ in range(args.rounds):
                for k, b in banks.items():
                    t, n_ = call(b)
                    ms[k].append(t)
                    got[k] += n_
            assert got["normalised"] == got["csi"], "the policy changes no frame count"
            desync = {k: int(b.status()["total_frames_desync"].sum()) for k, b in banks.items()}
            for b in banks.values():
                b.close()
            row = [E, name, got["csi"] / args.rounds]
            for k in banks:
                v = np.sort(np.array(ms[k]))
                row += [float(np.median(v)), float(v[0]), float(v[-1])]
            row.append(float(np.median(ms["normalised"]) / np.median(ms["csi"])))
            rows.append(row)
            print(json.dumps({"streams": E, "format": name, "frames_per_call": row[2], "desync": desync, "normalised_ms": row[3:6], "csi_ms": row[6:9],
                              "normalised_over_csi": row[9]}), flush=True)
            del bits, nf, scale
        del stream, sv, inputs
    ctx.close()
    lines = ["# Stream bank: the two soft-decision policies", "",
             f"`tools/bench_stream.py --compare-soft` on {torch.cuda.get_device_name(0)}: two banks of the same library, one per policy (level {args.soft_level:g}), fed the same",
             "blocks of one frame period per stream (`dabgpu_stream_bank_process_raw`, three acquisition calls each, then "
             f"{args.rounds} rounds that alternate the policies; wall clock",
             "around a call, which synchronises).  ms per call: median round (fastest .. slowest).  Ratio: normalised over weighted (above 1 = the weighted",
             "policy is faster).", "",
             "| streams | format | frames per call | normalised ms | weighted (csi) ms | ratio |", "|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r[0]} | {r[1]} | {r[2]:.0f} | {r[3]:.3f} ({r[4]:.3f} .. {r[5]:.3f}) | {r[6]:.3f} ({r[7]:.3f} .. {r[8]:.3f}) | {r[9]:.3f} |")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--block-frames", type=int, default=2)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--format", type=str, default="c32", help="c32 | raw_u8 | raw_s16l : capture format of the blocks")
    ap.add_argument("--digest", action="store_true", help="also print a checksum of the input and which streams lost synchronisation (development: run-to-run comparison)")
    ap.add_argument("--retained", action="store_true", help="dabgpu_stream_bank_process_retained: every block stays valid until the next call "
                                                            "has returned (the stream sits in one device array here), no carry-over copy")
    ap.add_argument("--soft-bits", choices=["normalised", "csi"], default="normalised", help="soft-decision policy of the bank (dabgpu_stream_bank_set_soft)")
    ap.add_argument("--soft-level", type=float, default=64.0, help="level of --soft-bits csi")
    ap.add_argument("--compare-soft", action="store_true", help="time both policies on the same blocks in alternating rounds and write --out")
    ap.add_argument("--compare-streams", default="256,4096")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx", "bench_stream_softbits.md"))
    args = ap.parse_args()
    if args.compare_soft:
        return compare_soft(args)
    dev = torch.device("cuda", 0)
    ctx = dabgpu.Context(0)
    E = args.streams
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    L = 196608
    frame = synth_frames(E, dev, g)
    n_block = args.block_frames * L
    total = n_block * args.calls + L
    reps = total // L + 2
    shift = torch.randint(0, L, (E,), generator=g, device=dev)
    cfo = (torch.rand(E, generator=g, device=dev) - 0.5) * 0.004
    stream = torch.empty((E, total), dtype=torch.complex64, device=dev)
    idx = torch.arange(total, device=dev)
    for e in range(E):
        x = frame[e].repeat(reps)[int(shift[e]):int(shift[e]) + total]
        stream[e] = x * torch.polar(torch.ones(total, device=dev), 2 * np.pi * float(cfo[e]) * idx.float())
    # (seeded like everything above: the same input in every run -- an unseeded noise realisation now and then moved one marginal
    # synchronisation decision of the acquisition call, which looked like a run-to-run difference of the bank)
    stream += 0.02 * torch.view_as_complex(torch.randn(stream.shape + (2,), generator=g, dtype=torch.float32, device=dev)) * 0.70710678
    del frame
    bank = dabgpu.StreamBank(ctx, E)
    if args.soft_bits == "csi":
        bank.set_soft(dabgpu.SoftCfg(dabgpu.SOFT_CSI, args.soft_level))
    max_frames = n_block // 191400 + 2
    bits = torch.zeros((E, max_frames, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device=dev)
    nf = torch.zeros(E, dtype=torch.int32, device=dev)
    sv = torch.view_as_real(stream)
    in_digest = int(sv.view(torch.int32).to(torch.int64).sum().item()) if args.digest else None
    fmt = None
    if args.format != "c32":
        fmt = dabgpu.IQ_FORMATS.index(args.format)
        peak = float(sv.abs().max().item())
        if args.format == "raw_u8":
            raw = torch.clamp(torch.round(sv / peak * 127.0 + 127.5), 0, 255).to(torch.uint8)
        else:
            raw = torch.clamp(torch.round(sv / peak * 30000.0), -32768, 32767).to(torch.int16)
        del stream, sv
        sb = dabgpu.iq_format_sample_bytes(fmt)
    frames_total, times = 0, []
    for k in range(args.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if args.retained:
            f_, base_, sb_ = (dabgpu.IQ_FORMATS.index("raw_f32l"), sv.data_ptr(), 8) if fmt is None else (fmt, raw.data_ptr(), sb)
            bank.process_retained(base_ + k * n_block * sb_, f_, total, n_block, (base_ + (k - 1) * n_block * sb_) if k else None, bits, max_frames, nf)
        elif fmt is None:
            bank.process(sv[:, k * n_block:(k + 1) * n_block], total, n_block, bits, max_frames, nf)
        else:
            bank.process_raw(raw.data_ptr() + k * n_block * sb, fmt, total, n_block, bits, max_frames, nf)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        got = int(nf.sum().item())
        times.append((dt, got))
        frames_total += got
    st = bank.status()
    if args.digest:
        des = st["total_frames_desync"]
        print(json.dumps({"input_digest": in_digest, "streams_with_desync": [(int(i), int(des[i]), int(st["total_frames_read"][i])) for i in np.nonzero(des)[0]]}))
    steady = times[2:] if len(times) > 3 else times
    fps = sum(g_ for _, g_ in steady) / sum(t for t, _ in steady)
    soft = {} if args.soft_bits == "normalised" else {"soft_bits": args.soft_bits, "soft_level": args.soft_level}
    print(json.dumps({**soft, "streams": E, "format": args.format, "retained_blocks": bool(args.retained), "block_samples": n_block, "calls": args.calls, "frames_total": frames_total,
                      "frames_desync_total": int(st["total_frames_desync"].sum()), "steady_frames_per_s": fps,
                      "steady_x_realtime_per_stream": fps / E / (2.048e6 / 196608),
                      "per_call_ms": [round(t * 1e3, 3) for t, _ in times], "per_call_frames": [g_ for _, g_ in times]}))


if __name__ == "__main__":
    main()
