#!/usr/bin/env python3
"""Times of packet mode with FEC on one MI355X, both directions, at the DAB+ bench's size: S streams (18,432), one FEC frame per stream and
call, 192-byte logical frames (13 per call: 2472 bytes and the first 24 of the next frame's padding), median of --reps calls by device events.
  encode   dabgpu_packet_tx_encode, 96-byte packets of one data group per stream
  receive  dabgpu_packet_bank_process over the encoder's output with 0 / 2 / 8 damaged symbols in every row
The run checks itself: every frame is corrected, its rs_count is the damage, the packets handed out are the encoder's.

    python tools/bench_packet.py [--streams 18432] [--reps 30] [--out profiles/tx/bench_packet.json]
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

RING, APP, FB, NF = 2472, 2256, 192, 13


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


def row_offsets():
    m = np.zeros((12, 204), np.int64)
    for y in range(12):
        for i in range(188):
            m[y, i] = i * 12 + y
        for i in range(16):
            t = i * 12 + y
            m[y, 188 + i] = APP + (t // 22) * 24 + 2 + t % 22
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=18432)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    S = args.streams
    ctx = dabgpu.Context(0)
    rng = np.random.default_rng(1)
    glen = 23 * 91 - 7                                       # one group that fills the 23 packets of a table but for 7 bytes
    st, table, first, consumed, _, _ = dabgpu.packet_tx_layout([glen], 0x155, 96, FB, 0, 0, 1)
    assert st == 0 and consumed == 1
    tab = np.zeros((S, 94), np.dtype(dabgpu.PACKET_TX_ENTRY_DTYPE))
    tab[:, :len(table)] = table
    data = rng.integers(0, 256, S * glen + 16, dtype=np.uint8)
    as_i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()
    as_i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()
    d_data = torch.from_numpy(data).cuda()
    d_goffs, d_gbase = as_i64(np.arange(S + 1) * glen), as_i32(np.arange(S + 1))
    d_tab = torch.from_numpy(tab.view(np.uint8)).cuda()
    d_first = as_i32(np.tile(first, (S, 1)))
    d_addr = torch.full((S,), 0x155, dtype=torch.int16, device="cuda")
    d_fb = torch.full((S,), FB, dtype=torch.int32, device="cuda")
    d_start = torch.zeros(S, dtype=torch.int64, device="cuda")
    d_frames = torch.zeros((S, NF, FB), dtype=torch.uint8, device="cuda")
    d_so = torch.arange(S, dtype=torch.int64, device="cuda") * (NF * FB)
    d_status = torch.full((S, 1), -1, dtype=torch.int32, device="cuda")
    tx = dabgpu.PacketTx(ctx)
    enc = median_ms(lambda: tx.encode(S, 1, d_data, d_goffs, d_gbase, d_tab, 94, d_first, d_addr, d_fb, d_start, d_frames, d_so, FB, d_status), args.reps)
    assert not d_status.cpu().numpy().any(), "the encoder refused a frame"
    clean = d_frames.cpu().numpy().reshape(S, NF * FB)
    out = {"device": torch.cuda.get_device_name(0), "streams": S, "frame_bytes": FB, "reps": args.reps,
           "encode_ms_median": enc[0], "encode_ms_min": enc[1], "encode_ms_max": enc[2], "fec_frames_per_s_encode": S / enc[0] * 1e3, "receive": []}
    # receive: each call starts from a fresh ring (the reset is outside the timed region would need a sync; a call over a whole frame ends with
    # an empty ring anyway, and the 24 trailing zero bytes leave one padding packet behind that the next call's frame pushes out)
    rows = row_offsets()
    cap = RING + NF * FB
    d_pk = torch.zeros((S, cap), dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros((S, 32 * 16), dtype=torch.uint8, device="cuda")
    d_fec = torch.zeros((S, 20), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros((S, 4), dtype=torch.int32, device="cuda")
    ok_all = True
    for damaged in (0, 2, 8):
        hurt = clean.copy()
        for y in range(12):
            cols = rng.choice(np.arange(1, 204), damaged, replace=False) if damaged else []
            for x in cols:
                v = int(rng.integers(1, 16)) << 2 if y == 0 else int(rng.integers(1, 256))
                hurt[:, rows[y, x]] ^= v
        d_in = torch.from_numpy(hurt).cuda()
        bank = dabgpu.PacketBank(ctx, S)
        t = median_ms(lambda: bank.process(d_in, d_so, FB, d_fb, NF, d_pk, cap, d_rec, 32, d_fec, 1, d_cnt), args.reps)
        torch.cuda.synchronize()
        cnt = d_cnt.cpu().numpy()
        fec = d_fec.cpu().numpy().view(np.dtype(dabgpu.PACKET_FEC_FRAME_DTYPE)).reshape(S)
        pk = d_pk.cpu().numpy()
        ok = bool((cnt[:, 2] == 1).all() and (cnt[:, 1] == APP).all() and (fec["rs_count"] == damaged).all() and np.array_equal(pk[:, :APP], clean[:, :APP]))
        ok_all &= ok
        bank.close()
        out["receive"].append({"damaged_symbols_per_row": damaged, "ms_median": t[0], "ms_min": t[1], "ms_max": t[2],
                               "fec_frames_per_s": S / t[0] * 1e3, "every_frame_corrected_and_equal": ok})
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    if not ok_all:
        sys.exit(1)


if __name__ == "__main__":
    main()
