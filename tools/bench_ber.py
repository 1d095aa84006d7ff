#!/usr/bin/env python3
"""Time of the channel BER call (dabgpu_ber_frames_layout, dab-radio_amd/csrc/channel_ber.hip) on one MI355X beside the decode call whose
outputs it reads (dabgpu_decode_frames_layout), in the same process on the same box: the canonical 18 x 48 CU multiplex of
tools/dabsynth.py at --ensembles ensembles, FIC + MSC, a ring of 5 frames of random soft bits, both soft-bit layouts.  The decoded bytes
are what the decode call leaves on those soft bits.  Warm-up calls, then one pair of HIP events per timed call, the two calls
alternating; the median is reported.  Algorithmic bytes of the BER call: every consumed soft bit once (9216 + 4 x sum of kept bits per
ensemble), the decoded bytes (384 + 4 x cif bytes) and the records (16 per code word), against 8 TB/s.  One JSON line; --out writes the
table of profiles/tx/bench_ber.md (the interpretation below the table is written by hand).

    python tools/bench_ber.py [--ensembles 4096] [--steps 30] [--warmup 5] [--out FILE]
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

PEAK_TB_S = 8.0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ensembles", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ber.py needs a GPU (no CPU fallback)")
    E, H = args.ensembles, 5
    ctx = dabgpu.Context(0)
    subs = [dabgpu.SubChannel(d["start"], d["length"], d["is_uep"], d["uep_index"], d["eep_level"], d["eep_type"]) for d in dabsynth.canonical_layout()]
    plan = dabgpu.tx_encode_plan(subs)
    nb, n_sub = plan["cif_in_bytes"], len(subs)
    geo = dabgpu.ber_plan(subs, E, H, H * dabgpu.NB_FRAME_BITS, 4 * nb)
    soft = E * (dabgpu.NB_FIC_BITS + 4 * sum(int(p.kept_bits) for p in plan["subs"]))
    alg = soft + E * (384 + 4 * nb) + E * geo.codewords_per_ensemble * 16
    g = torch.Generator(device="cuda").manual_seed(1)
    hist = torch.randint(-128, 128, (E, H, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda", generator=g)
    fib = torch.zeros((E, 4, 96), dtype=torch.uint8, device="cuda"); fres = torch.zeros((E * 4, 16), dtype=torch.uint8, device="cuda")
    msc = torch.zeros((E, 4, nb), dtype=torch.uint8, device="cuda"); mres = torch.zeros((E * 4 * n_sub, 16), dtype=torch.uint8, device="cuda")
    fic_ber = torch.zeros((E, 4, 16), dtype=torch.uint8, device="cuda"); msc_ber = torch.zeros((E, 4, n_sub, 16), dtype=torch.uint8, device="cuda")
    res = {"tool": "bench_ber", "ensembles": E, "history_frames": H, "steps": args.steps, "warmup": args.warmup, "codewords_per_call": E * geo.codewords_per_ensemble,
           "lds_bytes_per_codeword": geo.lds_bytes, "grid": geo.grid, "soft_bits_per_call": soft, "algorithmic_bytes": alg, "cases": []}
    for name, layout in (("natural", dabgpu.BITS_NATURAL), ("classed", dabgpu.BITS_MSC_CLASSED)):
        stride = H * dabgpu.NB_FRAME_BITS
        dec = lambda: ctx.decode_frames(hist, E, stride, H, 2, subs, fib, fres, msc, 4 * nb, mres, bits_layout=layout)      # noqa: E731
        ber = lambda: ctx.ber_frames(hist, E, stride, H, 2, subs, fib, msc, 4 * nb, fic_ber, msc_ber, bits_layout=layout)    # noqa: E731
        for _ in range(args.warmup):
            dec(); ber()
        torch.cuda.synchronize()
        td, tb = [], []
        for _ in range(args.steps):
            td.append(timed(dec)); tb.append(timed(ber))
        md, mb = statistics.median(td), statistics.median(tb)
        recs = msc_ber.cpu().numpy().view(dabgpu.BER_RESULT_DTYPE)
        res["cases"].append({"layout": name, "ber_ms": round(mb, 4), "ber_ms_min_max": [round(min(tb), 4), round(max(tb), 4)],
                             "decode_ms": round(md, 4), "decode_ms_min_max": [round(min(td), 4), round(max(td), 4)], "ber_over_decode": round(mb / md, 4),
                             "algorithmic_TB_per_s": round(alg / mb / 1e9, 4), "fraction_of_8_TB_per_s": round(alg / mb / 1e9 / PEAK_TB_S, 4),
                             "us_per_codeword_wave": round(mb * 1e3 / (E * geo.codewords_per_ensemble), 5),
                             "msc_error_fraction": round(float(recs["n_errors"].sum()) / float(recs["n_bits"].sum()), 4)})
    ctx.close()
    print(json.dumps(res))
    if args.out:
        lines = ["# Channel BER call against the decode call", "",
                 f"Device: AMD Instinct MI355X ({torch.cuda.get_device_properties(0).gcnArchName}).  `python tools/bench_ber.py --ensembles {E} --steps {args.steps} --warmup {args.warmup}`: "
                 f"canonical 18 x 48 CU multiplex, {E} ensembles, FIC + MSC = {E * geo.codewords_per_ensemble} code words (one wavefront each, {geo.grid} workgroups of 4), "
                 f"ring of {H} frames of random soft bits, HIP events around every call, the two calls alternating, medians of {args.steps} (min .. max).  "
                 f"Algorithmic bytes of the BER call: {soft / 1e9:.3f} GB of consumed soft bits + decoded bytes + records = {alg / 1e9:.3f} GB.", "",
                 "| soft-bit layout | BER call ms | decode call ms | BER / decode | algorithmic TB/s | of 8 TB/s |", "|---|---|---|---|---|---|"]
        for c in res["cases"]:
            lines.append(f"| {c['layout']} | {c['ber_ms']:.3f} ({c['ber_ms_min_max'][0]:.3f} .. {c['ber_ms_min_max'][1]:.3f}) | "
                         f"{c['decode_ms']:.3f} ({c['decode_ms_min_max'][0]:.3f} .. {c['decode_ms_min_max'][1]:.3f}) | {c['ber_over_decode']:.3f} | "
                         f"{c['algorithmic_TB_per_s']:.3f} | {100 * c['fraction_of_8_TB_per_s']:.1f} % |")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
