#!/usr/bin/env python3
"""Rate of the channel encoder bank (dabgpu_tx_bank_encode_frames / _transmit_frames, dab-radio_amd/csrc/dab_encode.hip) on one MI355X
against the modulator alone (dabgpu_ofdm_modulate_frames on the same number of frames, frame-bit payload, complex float output) in
the same process: --ensembles ensembles, F = 1 and F = 4 frames per ensemble and call, the canonical and the mixed multiplex of
tools/dabsynth.py, random FIB bodies and payload.  Warm-up calls, then one pair of HIP events per timed call; the median is reported.
Algorithmic bytes of the encoder per frame: 360 B of FIB bodies + 4 x cif_in_bytes in, 28,800 B out, and 2 x 4 x 8 B per occupied
capacity unit of interleaver state (one write, one read of every ring row).  One JSON line.

    python tools/bench_encode.py [--ensembles 4096] [--steps 30] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dab-radio_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import dabgpu  # noqa: E402
import dabsynth  # noqa: E402

FRAME_BYTES = 28800
SAMPLES = 196608


def median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ensembles", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 4])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_encode.py needs a GPU (no CPU fallback)")
    E = args.ensembles
    ctx = dabgpu.Context(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    f32 = dabgpu.IQ_FORMATS.index("raw_f32l")
    res = {"tool": "bench_encode", "ensembles": E, "steps": args.steps, "warmup": args.warmup, "cases": []}
    for name, layout in (("canonical", dabsynth.canonical_layout()), ("mixed", dabsynth.mixed_layout())):
        subs = [dabgpu.SubChannel(d["start"], d["length"], d["is_uep"], d["uep_index"], d["eep_level"], d["eep_type"]) for d in layout]
        occupied = sum(d["length"] for d in layout)
        for F in args.frames:
            n = E * F
            bank = dabgpu.TxBank(ctx, E, subs)
            fib = torch.randint(0, 256, (n * 360,), dtype=torch.uint8, device="cuda", generator=g)
            pay = torch.randint(0, 256, (n * 4 * bank.cif_in_bytes,), dtype=torch.uint8, device="cuda", generator=g)
            bits = torch.empty(n * FRAME_BYTES, dtype=torch.uint8, device="cuda")
            iq = torch.empty(n * SAMPLES * 8, dtype=torch.uint8, device="cuda")
            enc = median_ms(lambda: bank.encode_frames(fib, pay, F, bits), args.steps, args.warmup)
            mod = median_ms(lambda: ctx.ofdm_modulate_frames(1, bits, n, iq, layout=dabgpu.TX_PAYLOAD_FRAME_BITS, out_format=f32), args.steps, args.warmup)
            txm = median_ms(lambda: bank.transmit_frames(fib, pay, F, iq, out_format=f32), args.steps, args.warmup)
            enc_bytes = n * (360 + 4 * bank.cif_in_bytes + FRAME_BYTES + 2 * 4 * 8 * occupied)
            res["cases"].append({
                "multiplex": name, "frames_per_ensemble": F, "frames_per_call": n, "cif_in_bytes": bank.cif_in_bytes,
                "encode_ms": round(enc[0], 4), "encode_ms_min_max": [round(enc[1], 4), round(enc[2], 4)], "encode_frames_per_s": round(n / enc[0] * 1e3),
                "encode_algorithmic_bytes": enc_bytes, "encode_TB_per_s": round(enc_bytes / enc[0] / 1e9, 4),
                "modulate_ms": round(mod[0], 4), "modulate_ms_min_max": [round(mod[1], 4), round(mod[2], 4)],
                "transmit_ms": round(txm[0], 4), "transmit_ms_min_max": [round(txm[1], 4), round(txm[2], 4)],
                "transmit_over_modulate": round(txm[0] / mod[0], 4), "encode_over_modulate": round(enc[0] / mod[0], 4)})
            bank.close()
            del fib, pay, bits, iq
            torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
