#!/usr/bin/env python3
"""Time of the DAB+ super-frame encoder (dabgpu_dabplus_tx_encode) on one MI355X against the decoder's clean path on the same super frames.
S streams, one super frame per call, median of --reps calls by device events.  In the same process dabgpu_dabplus_bank_process takes the
encoder's output undamaged (5 logical frames per stream = one super frame per call): every super frame must come back with its fire code,
no corrected symbol and all access-unit CRCs, so the run checks itself.  Algorithmic bytes per call = access-unit bytes in + 120 n_rs out
per super frame; their share of 8 TB/s is for the record only (the kernel is latency-bound, not HBM-bound).

    python tools/bench_dabplus_tx.py [--reps 30] [--out profiles/tx/bench_dabplus_tx.json]
    python tools/bench_dabplus_tx.py --only 18432x192 --reps 5        (a short run for a kernel trace)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dab-radio_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dabgpu  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
SIZES = [(18432, 192), (18432, 24), (4096, 1536)]          # the size DESIGN 4.6 quotes for the decoder; n_rs = 1; n_rs = 64


def median_ms(run, reps, warmup=5):
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def one_size(ctx, S, n, reps):
    rng = np.random.default_rng(1)
    n_rs = n // 24
    desc = 0x60                                              # 48 kHz, SBR: 3 access units
    room = 110 * n_rs - 6 - 6
    lens = np.zeros((S, 1, 6), np.uint16)
    first = min(room // 3, 1360)                             # (the third unit's start has to fit 12 bits: equal thirds do not at n_rs = 64)
    lens[:, 0, 0] = first
    lens[:, 0, 1] = first
    lens[:, 0, 2] = room - 2 * first
    au = rng.integers(0, 256, S * room + 4, dtype=np.uint8)
    offs = (np.arange(S, dtype=np.int64) * room).reshape(S, 1)
    d_au, d_offs = torch.from_numpy(au).cuda(), torch.from_numpy(offs).cuda()
    d_lens = torch.from_numpy(lens.view(np.int16)).cuda()
    d_desc = torch.full((S, 1), desc, dtype=torch.uint8, device="cuda")
    d_n = torch.full((S,), n, dtype=torch.int32, device="cuda")
    d_frames = torch.zeros((S, 5, n), dtype=torch.uint8, device="cuda")
    d_so = torch.arange(S, dtype=torch.int64, device="cuda") * (5 * n)
    d_status = torch.full((S, 1), -1, dtype=torch.int32, device="cuda")
    tx = dabgpu.DabPlusTx(ctx)

    def encode():
        tx.encode(S, 1, d_au, d_offs, d_lens, d_desc, d_n, d_frames, d_so, n, d_status)
    enc = median_ms(encode, reps)
    assert not d_status.cpu().numpy().any(), "the encoder refused a super frame"
    # the decoder's clean path on what the encoder wrote
    rdt = np.dtype(dabgpu.SUPERFRAME_RESULT_DTYPE)
    d_sf = torch.zeros((S, 1, 5 * n), dtype=torch.uint8, device="cuda")
    d_res = torch.zeros((S, 1, rdt.itemsize), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros((S, 4), dtype=torch.int32, device="cuda")
    bank = dabgpu.DabPlusBank(ctx, S)

    def decode():
        bank.process(d_frames, d_so, n, d_n, 5, d_sf, 5 * n, d_res, 1, d_cnt)
    dec = median_ms(decode, reps)
    res = d_res.cpu().numpy().view(rdt).reshape(S)
    ok = bool((res["firecode_ok"] == 1).all() and (res["rs_corrected"] == 0).all() and (res["au_crc_ok_mask"] == 7).all()
              and (d_cnt[:, 0] == 1).all().item() and torch.equal(d_sf.reshape(S, 5 * n), d_frames.reshape(S, 5 * n)))
    bank.close()
    algo_bytes = S * (room + 120 * n_rs)
    return {"streams": S, "frame_bytes": n, "rs_codewords_per_superframe": n_rs, "reps": reps,
            "encode_ms_median": enc[0], "encode_ms_min": enc[1], "encode_ms_max": enc[2],
            "decode_clean_ms_median": dec[0], "decode_clean_ms_min": dec[1], "decode_clean_ms_max": dec[2],
            "encode_over_decode_clean": enc[0] / dec[0], "superframes_per_s": S / enc[0] * 1e3,
            "algorithmic_bytes_per_call": algo_bytes, "share_of_8TBps": algo_bytes / (enc[0] * 1e-3) / HBM_BYTES_PER_S,
            "decoder_accepts_every_superframe": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only", default="", help="SxN: one size only, e.g. 18432x192")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in args.only.split("x"))] if args.only else SIZES
    ctx = dabgpu.Context(0)
    out = {"device": torch.cuda.get_device_name(0), "sizes": [one_size(ctx, S, n, args.reps) for S, n in sizes]}
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    if not all(s["decoder_accepts_every_superframe"] for s in out["sizes"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
