#!/usr/bin/env python3
"""Rate of the OFDM transmitter (dabgpu_ofdm_modulate_frames, dab-radio_amd/csrc/ofdm_mod.hip) on one MI355X, transmission mode I,
random reference-layout payloads: (a) complex float output, no frequency shift; (b) 8-bit IQ with a +1000 Hz shift (simulate_transmitter's
output).  Warm-up, then HIP events on torch's current stream around back-to-back calls covering >= --min-seconds of work.
Algorithmic bytes per call: n * (28,800 payload + 196,608 samples * 8 | 2); the fraction is against 8 TB/s.  One JSON line.

    python tools/bench_tx.py [--frames 4096] [--min-seconds 1.0]
    bash tools/prof_kernels.sh tools/bench_tx.py          # kernel times (rocprofv3)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dab-radio_amd"))

import torch  # noqa: E402

import dabgpu  # noqa: E402

PAYLOAD_BYTES = 28800
SAMPLES = 196608
HBM_PEAK = 8.0e12


def timed(fn, min_seconds):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(5, int(min_seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tx.py needs a GPU (no CPU fallback)")
    n = args.frames
    ctx = dabgpu.Context(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    pay = torch.randint(0, 256, (n * PAYLOAD_BYTES,), dtype=torch.uint8, device="cuda", generator=g)
    f32, u8 = dabgpu.IQ_FORMATS.index("raw_f32l"), dabgpu.IQ_FORMATS.index("raw_u8")
    out = torch.empty(n * SAMPLES * 8, dtype=torch.uint8, device="cuda")
    res = {"tool": "bench_tx", "mode": 1, "frames_per_call": n, "tx_spb": os.environ.get("DABGPU_TX_SPB", "auto")}
    for name, fmt, hz, sample_bytes in (("f32", f32, 0.0, 8), ("u8_shift_1000hz", u8, 1000.0, 2)):
        fn = float(torch.tensor(hz, dtype=torch.float32) / torch.tensor(2.048e6, dtype=torch.float32))
        ms, reps = timed(lambda: ctx.ofdm_modulate_frames(1, pay, n, out, out_format=fmt, freq_norm=fn), args.min_seconds)
        nbytes = n * (PAYLOAD_BYTES + SAMPLES * sample_bytes)
        res[name] = {"ms_per_call": round(ms, 4), "calls": reps, "frames_per_s": round(n / ms * 1e3),
                     "algorithmic_bytes_per_call": nbytes, "TB_per_s": round(nbytes / ms / 1e9, 3),
                     "frac_of_8TBps": round(nbytes / ms / 1e9 / (HBM_PEAK / 1e12), 4)}
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
