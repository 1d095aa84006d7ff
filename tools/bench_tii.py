#!/usr/bin/env python3
"""Development bench: dabgpu_tii_bank_process (one transform per receiver) beside dabgpu_ofdm_sync (five transforms per receiver) on the
same receivers' samples in one process; median of --calls single calls timed by HIP events.
    python tools/bench_tii.py [--receivers 4096] [--calls 30] [--out profiles/tii/bench_tii.md]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dab-radio_amd"))
import numpy as np
import torch
import dabgpu

ap = argparse.ArgumentParser()
ap.add_argument("--receivers", type=int, default=4096)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tii", "bench_tii.md"))
a = ap.parse_args()
n, stride = a.receivers, 4224                      # a NULL period, the reach of a record's fine_time_offset, rounded to 16 bytes x 2
ctx = dabgpu.Context(0)
g = torch.Generator(device="cuda"); g.manual_seed(1)
x = torch.randn((n, stride, 2), generator=g, dtype=torch.float32, device="cuda")
sdt, rdt = np.dtype(dabgpu.SYNC_STATE_DTYPE), np.dtype(dabgpu.TII_RECORD_DTYPE)
rec = np.zeros(n, sdt)                             # the detector's records: every receiver valid, a settled offset, NULL at the slice's start
rec["sync_valid"], rec["freq_coarse"], rec["freq_fine"] = 1, np.float32(-3.0 / 2048), np.float32(-0.05 / 2048)
d_rec = torch.from_numpy(rec.view(np.uint8)).cuda()
d_sync = torch.zeros(n * sdt.itemsize, dtype=torch.uint8, device="cuda")     # the synchroniser's own (noise: it finds no peak)
bank = dabgpu.TiiBank(ctx, n)
res = torch.zeros(n * 24 * rdt.itemsize, dtype=torch.uint8, device="cuda")
cnt = torch.zeros(n, dtype=torch.int32, device="cuda")


def median_ms(call):
    for _ in range(5):
        call()
    ms = []
    for _ in range(a.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        call()
        e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


rows = {"dabgpu_ofdm_sync": median_ms(lambda: ctx.ofdm_sync(x, n, stride, d_sync)),
        "dabgpu_tii_bank_process, accumulate": median_ms(lambda: bank.process(x, stride, 0, states=d_rec)),
        "dabgpu_tii_bank_process, accumulate + decide": median_ms(lambda: bank.process(x, stride, 0, states=d_rec, decide=True, results=res, counts=cnt))}
_, frames = bank.read()
assert (frames == 2 * (a.calls + 5)).all()
bank.close()
read_gb = n * 2048 * 8 / 1e9
lines = ["# TII detector beside the synchroniser", "",
         f"{n} receivers, median of {a.calls} single calls by HIP events (min .. max), {os.path.basename(dabgpu.LIB_PATH)}, {torch.cuda.get_device_name(0)} (torch's name for the card).",
         f"Each call reads one 2048-sample window per receiver ({read_gb * 1e3:.1f} MB).", "",
         "| call | median ms | min | max | GB/s of window read |", "|---|---|---|---|---|"]
for k, (med, lo, hi) in rows.items():
    lines.append(f"| {k} | {med:.4f} | {lo:.4f} | {hi:.4f} | {read_gb / (med * 1e-3):.0f} |")
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(json.dumps({"receivers": n, "calls": a.calls, "median_ms": {k: v[0] for k, v in rows.items()}}))
