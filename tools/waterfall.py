#!/usr/bin/env python3
"""First sensitivity figures of the receiver: FIB CRC pass rate and MSC byte-error rate per protection level against signal-to-noise
ratio, on the device from end to end.  One mode I transmission (dabgpu.TxBank) feeds E channel streams (dabgpu.Channel, one shared
input, a noise seed each); every stream is a receiver: dabgpu_ofdm_sync_demod_frames -> dabgpu_decode_frames_layout.  Two channels: white
noise alone, then two paths (the second 200 samples late at -6 dB) with the same noise.  Multiplex: 48-CU sub-channels at EEP 1-A,
2-A, 3-A (x 13, the canonical layout's profile) and 4-A plus a 52-CU UEP row (the full canonical 18 x 48 leaves no room for the other
levels).  SNR = mean power of the modulator's symbols after the taps (1536 x sum |tap|^2) over 2 sigma^2, as the transmitter tool defines it.
With --doppler-hz (and optionally --profile tu6|ra6|sfn2; default tu6) the channels are replaced by ONE fading channel: the preset's taps
on a fading bank (dabgpu.Channel(..., fading=)), a fading seed per receiver, SNR against the taps' mean power; give such a run its own --out
(profiles/tx/waterfall_fading.md).  Without those options the run and its output are the ones of before.
With --clock-ppm X[,Y...] the run is the white-noise channel followed by the resampler (dabgpu.Resampler behind dabgpu.Channel: the noise is
resampled too, as at a receiver's ADC) at a sampling-clock error of X ppm (step 1 + X 1e-6), one table per error, and the tables are
APPENDED to --out: the clock error's place in the sensitivity record.
With --adjacent-db A[,B...] [--adjacent-sides 1|2] the run is the white-noise channel followed by the combiner and the channeliser
(dabgpu.Channeliser, D = 4): the block 300 kHz above the centre of an 8.192 MS/s capture with a neighbour 1.712 MHz above it (sides = 1) or
to either side (2, the default), A dB above the wanted block's signal power -- the clean transmission rolled by 50001 and 120007 samples --,
then split back out; one table per level, APPENDED to --out: the adjacent block's place in the sensitivity record.
With --ber every table gains two columns: the channel BER the receiver MEASURES (dabgpu_ber_frames_layout on what it decoded: errors / bits over the
FIB groups of every frame and the sub-channel code words from CIF 15 on) and the TRUE channel BER of the same soft bits against the transmitted
bits (a second TxBank keeps the frame bits).  The two agree while the decoders deliver; below the waterfall the measured figure falls short of
the true one, because a wrongly decoded code word is re-encoded into a neighbour of what was received.  Without the flag the output is unchanged.
With --soft-bits csi [--soft-level L] every receiver runs twice on the same received samples, with the reference's soft bits and with the
channel-state weighted ones (dabgpu_ofdm_sync_demod_frames_soft), and every cell reads `normalised -> csi`; the output goes to
profiles/tx/waterfall_csi.md (waterfall.md is not rewritten), a run with --doppler-hz being APPENDED to it.
With --branches K (receive diversity; K = 2 .. 8) every receiver hears K realisations of the channel -- branch b of receiver e is channel stream
b x streams + e, with a noise seed and (under --doppler-hz) a fading seed of its own -- through dabgpu_ofdm_sync_demod_frames_branch (weighted soft
bits at --soft-level, DQPSK products, scale, sync record), and dabgpu_diversity_combine_frames puts the K branches' products into one frame of soft
bits in the decoder's ring.  Every cell reads `single -> combined`: branch 0 decoded alone, and the combination.  The output goes to
profiles/tx/waterfall_diversity.md.
With --branches K --branch-noise-db a,b,... (the extra noise of each branch in dB, K values) and / or --weights unit|estimated|true the branches are
combined with maximal-ratio weights: `estimated` takes them from dabgpu_noise_estimate_frames on every branch's slice and sync records (the slices
then hold the whole NULL in front of each frame), `true` is 1 / (2 noise_sigma^2) of the branch's own channel stream, `unit` no weight.  SNR is
that of a branch without extra noise.  The output goes to profiles/tx/waterfall_mrc.md, which such a run writes anew unless --append is given: the
committed file is a unit run followed by an estimated and a true run with --append, and any of them can be repeated alone into an --out of its own.
Without these two options the output is what it was.
(--interferer-source device: the interferer comes from dabgpu.Interferer, the library's own bank, in place of the torch one below; the default,
torch, is what the committed outputs were made with.)
With --interferer OFFSET_KHZ:WIDTH_KHZ:IS_DB a narrowband interferer is added to every channel stream behind the channel: Gaussian noise confined to
WIDTH_KHZ around OFFSET_KHZ from the block's centre (white noise made with torch on the device, every bin of its transform outside the band cleared;
a seed per stream), its total power IS_DB relative to the signal power the SNR refers to.  The torch source is the tool's own, kept so that the
committed outputs can be made again; the library's is dabgpu.Interferer.  It wants the branch path (--branches K, or --weights banded, which also takes K = 1).  With --weights banded [--alpha A] every branch's
slice and sync records go through dabgpu_noise_profile_frames (the state carried from frame to frame in place, smoothing A, default 0.25) and the
band weights into dabgpu_diversity_combine_frames_banded: with one branch interference-aware soft bits, with several maximal-ratio combining per
band.  Every cell still reads `single -> combined`, branch 0's own weighted soft bits against the banded combination.  The output goes to
profiles/tx/waterfall_banded.md.
With --interferer-gate PERIOD:ON:IS_DB a burst interferer is added to every channel stream behind the channel: white noise from the library's own
bank (dabgpu.Interferer, a seed per stream) behind its integer gate, on for ON of every PERIOD samples (20480:205 = 100 us every 10 ms), IS_DB
relative to the signal power while it is on.  With --blank [THRESHOLD] every receiver runs twice, on the received samples as they are and on the
same samples through the impulse blanker (dabgpu.Blanker, dabgpu_blanker_defaults with that threshold, default 3), and every cell reads
`unblanked -> blanked`; under every table the share of the blocks the blanker zeroed.  The output goes to profiles/tx/waterfall_blank.md.  Both
options belong to the plain receiver path (not with --branches, --weights, --soft-bits csi, --clock-ppm, --adjacent-db, --doppler-hz or --ber).
With --weights banded-dd the band weights come from dabgpu_dd_profile_frames on every branch's own DQPSK products in the place of
the NULL-based profile; the output goes to profiles/tx/waterfall_banded_dd.md.  With --weights banded|banded-dd, --interferer takes the bank's gate:
--interferer-gate PERIOD:ON:OFFSET then gates the band interferer itself (the library's source: on iff ((m - OFFSET) mod PERIOD) < ON), e.g.
196608:191952:3656 silences it from 1000 samples in front of every NULL symbol to 1000 behind it.
Without them the run and its outputs are what they were.
    python tools/waterfall.py [--streams 64] [--frames 6] [--snr 2:15:1] [--out profiles/tx/waterfall.md] [--doppler-hz F] [--profile NAME]
                              [--clock-ppm X[,Y...]] [--adjacent-db A[,B...]] [--adjacent-sides 1|2] [--ber] [--soft-bits csi] [--branches K]
                              [--branch-noise-db A,B,...] [--weights unit|estimated|true|banded|banded-dd] [--alpha A] [--interferer OFFSET_KHZ:WIDTH_KHZ:IS_DB]
                              [--append] [--interferer-gate PERIOD:ON:IS_DB] [--blank [THRESHOLD]]"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "dab-radio_amd")]

S, NULL, P_LEAD = 196608, 2656, 700
STRIDE = P_LEAD + 1544 + S
LEVELS = [("EEP 1-A", [(624, 48, 0, 0, 0)]), ("EEP 2-A", [(672, 48, 0, 0, 1)]), ("EEP 3-A", [(48 * k, 48, 0, 0, 2) for k in range(13)]),
          ("EEP 4-A", [(720, 48, 0, 0, 3)]), ("UEP row 20", [(768, 52, 1, 20, 0)])]
PROFILES = [("white noise", [(0, 1.0, 0.0)]), ("two paths (second 200 samples late, -6 dB) + noise", [(0, 1.0, 0.0), (200, 0.5, 0.0)])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--snr", default="2:15:1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx", "waterfall.md"))
    ap.add_argument("--doppler-hz", type=float, default=None)
    ap.add_argument("--profile", default=None)
    ap.add_argument("--clock-ppm", default=None)
    ap.add_argument("--adjacent-db", default=None)
    ap.add_argument("--adjacent-sides", type=int, default=2, choices=(1, 2))
    ap.add_argument("--ber", action="store_true")
    ap.add_argument("--soft-bits", default="normalised", choices=("normalised", "csi"))
    ap.add_argument("--soft-level", type=float, default=64.0)
    ap.add_argument("--branches", type=int, default=1)
    ap.add_argument("--branch-noise-db", default=None)
    ap.add_argument("--weights", default="unit", choices=("unit", "estimated", "true", "banded", "banded-dd"))
    ap.add_argument("--alpha", type=float, default=0.25)
    ap.add_argument("--interferer", default=None)
    ap.add_argument("--interferer-source", default="torch", choices=("torch", "device"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--interferer-gate", default=None)
    ap.add_argument("--blank", nargs="?", type=float, const=3.0, default=None)
    a = ap.parse_args()
    K = a.branches
    mrc = a.branch_noise_db is not None or a.weights != "unit"
    banded = a.weights in ("banded", "banded-dd")
    dd = a.weights == "banded-dd"
    branch_path = K > 1 or banded
    if mrc and K == 1 and not banded:
        ap.error("--branch-noise-db and --weights want --branches K")
    if not 0.0 < a.alpha <= 1.0:
        ap.error("--alpha takes a value in (0, 1]")
    jam = None
    if a.interferer is not None:
        if not branch_path:
            ap.error("--interferer wants --branches K or --weights banded")
        jam = [float(v) for v in a.interferer.split(":")]
        if len(jam) != 3 or not 0.0 < jam[1] <= 2048.0 or abs(jam[0]) + jam[1] / 2.0 > 1024.0:
            ap.error("--interferer takes OFFSET_KHZ:WIDTH_KHZ:IS_DB inside the sampled band")
    if a.append and not mrc:
        ap.error("--append wants --branch-noise-db or --weights (the other records decide by their options whether they append)")
    branch_db = [float(v) for v in a.branch_noise_db.split(",")] if a.branch_noise_db is not None else [0.0] * K
    if len(branch_db) != K:
        ap.error("--branch-noise-db takes one value per branch")
    p_lead = NULL + P_LEAD if mrc else P_LEAD                                   # (with weights: the whole NULL in front of every frame)
    stride = p_lead + 1544 + S
    if branch_path:
        if (K < 2 and not banded) or K < 1 or K > 8:
            ap.error("--branches takes 2 .. 8")
        if a.clock_ppm is not None or a.adjacent_db is not None or a.ber or a.soft_bits == "csi":
            ap.error("--branches is not available with --clock-ppm, --adjacent-db, --ber or --soft-bits (its branches are weighted already)")
        if a.out == ap.get_default("out"):
            a.out = os.path.join(ROOT, "profiles", "tx", "waterfall_banded_dd.md" if dd else "waterfall_banded.md" if banded else "waterfall_mrc.md" if mrc else "waterfall_diversity.md")
    csi = a.soft_bits == "csi"
    if csi and (a.clock_ppm is not None or a.adjacent_db is not None):
        ap.error("--soft-bits csi is not available with --clock-ppm or --adjacent-db")
    if csi and a.out == ap.get_default("out"):
        a.out = os.path.join(ROOT, "profiles", "tx", "waterfall_csi.md")           # (waterfall.md is never rewritten by such a run)
    if a.adjacent_db is not None and (a.doppler_hz is not None or a.clock_ppm is not None):
        ap.error("--adjacent-db is not available with --doppler-hz or --clock-ppm")
    adjacent_db = [float(v) for v in a.adjacent_db.split(",")] if a.adjacent_db is not None else []
    if a.clock_ppm is not None and a.doppler_hz is not None:
        ap.error("--clock-ppm is not available with --doppler-hz")
    clock_ppm = [float(v) for v in a.clock_ppm.split(",")] if a.clock_ppm is not None else []
    if a.profile is not None and a.doppler_hz is None:
        ap.error("--profile wants --doppler-hz")
    gate = None
    if a.interferer_gate is not None:
        gate = a.interferer_gate.split(":")
        if len(gate) != 3:
            ap.error("--interferer-gate takes PERIOD:ON:IS_DB")
        gate = (int(gate[0]), int(gate[1]), float(gate[2]))
        if not 0 < gate[1] <= gate[0]:
            ap.error("--interferer-gate: 0 < ON <= PERIOD samples")
    jam_gate = None
    if gate is not None and jam is not None:
        # the band interferer behind the bank's own gate: the third field is the gate's offset in samples, the source the library's
        if not banded or gate[2] != int(gate[2]):
            ap.error("--interferer with --interferer-gate PERIOD:ON:OFFSET wants --weights banded or banded-dd")
        jam_gate, gate = dict(gate_period=gate[0], gate_on=gate[1], gate_offset=int(gate[2])), None
        a.interferer_source = "device"
    blank = a.blank is not None
    if blank or gate is not None:
        if branch_path or mrc or csi or a.clock_ppm is not None or a.adjacent_db is not None or a.doppler_hz is not None or a.ber:
            ap.error("--interferer-gate and --blank belong to the plain receiver path")
    if blank:
        if not 1.0 < a.blank <= 1024.0:
            ap.error("--blank takes a threshold above 1, up to 1024")
        if a.out == ap.get_default("out"):
            a.out = os.path.join(ROOT, "profiles", "tx", "waterfall_blank.md")          # (waterfall.md is never rewritten by such a run)
    import numpy as np
    import torch
    import dabgpu
    policies = [dabgpu.SOFT_NORMALISED, dabgpu.SOFT_CSI] if csi else [dabgpu.SOFT_NORMALISED]
    lo, hi, step = (float(v) for v in a.snr.split(":"))
    snrs = [lo + i * step for i in range(int(round((hi - lo) / step)) + 1)]
    E, F, H = a.streams, a.frames, 8
    EC = E * K                                                                  # channel streams: K realisations per receiver
    ctx = dabgpu.Context(0)
    subs, owner = [], []
    for li, (_, lst) in enumerate(LEVELS):
        for (start, length, uep, row, lvl) in lst:
            subs.append(dabgpu.SubChannel(start, length, uep, row, lvl, 0)); owner.append(li)
    plan = dabgpu.tx_encode_plan(subs)
    nb = plan["cif_in_bytes"]
    spans = [(int(p.in_offset), int(p.in_bytes)) for p in plan["subs"]]
    rng = np.random.default_rng(1)
    fib = rng.integers(0, 256, (1, F, 4, 3, 30), dtype=np.uint8)
    pay = rng.integers(0, 256, (1, F, 4, nb), dtype=np.uint8)
    bank = dabgpu.TxBank(ctx, 1, subs)
    d_iq = torch.zeros((F * S, 2), dtype=torch.float32, device="cuda")
    bank.transmit_frames(torch.from_numpy(fib).cuda(), torch.from_numpy(pay).cuda(), F, d_iq)
    if a.ber:
        # the transmitted frame bits (a bank of its own: transmit_frames above has advanced the first one's time interleaver) and, per frame, where
        # the decoders' soft bits come from: (ring slot, frame bit) of the FIC and of every sub-channel code word from CIF 15 on
        bank2 = dabgpu.TxBank(ctx, 1, subs)
        d_sent = torch.zeros((F, dabgpu.NB_FRAME_BITS // 8), dtype=torch.uint8, device="cuda")
        bank2.encode_frames(torch.from_numpy(fib).cuda(), torch.from_numpy(pay).cuda(), F, d_sent)
        torch.cuda.synchronize()
        bank2.close()
        sent = torch.from_numpy(np.unpackbits(d_sent.cpu().numpy(), axis=1, bitorder="little").astype(np.bool_)).cuda()
        delay = np.array([0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15])
        consumed = []
        for j in range(F):
            fr, pos = [np.full(dabgpu.NB_FIC_BITS, j)], [np.arange(dabgpu.NB_FIC_BITS)]
            for c in range(4):
                if 4 * j + c < 15:
                    continue
                for p in plan["subs"]:
                    i = np.arange(int(p.kept_bits))
                    cif = 4 * j + c - (15 - delay[i % 16])
                    fr.append(cif // 4); pos.append(dabgpu.NB_FIC_BITS + dabgpu.NB_CIF_BITS * (cif % 4) + 64 * int(p.start_address) + i)
            consumed.append((torch.from_numpy(np.concatenate(fr)).cuda(), torch.from_numpy(np.concatenate(pos)).cuda()))
        bdt = np.dtype(dabgpu.BER_RESULT_DTYPE)
    n_out = F * S + 4096
    n_rx = n_out + (256 if clock_ppm or adjacent_db else 0)                   # (the resampler and the combiner read ahead of their output)
    ADJ_D, ADJ_RATE, ADJ_OFFSET, ADJ_SPACING, ADJ_ROLLS = 4, 8192000.0, 300000.0, 1712000.0, (50001, 120007)
    n_rows = 1 + (a.adjacent_sides if adjacent_db else 0)
    n_wide = n_out * ADJ_D + 72 * ADJ_D
    # with neighbours a receiver has n_rows block rows: the channel writes row 0, the others hold the clean transmission rolled
    d_rows = torch.zeros((EC, n_rows, n_rx, 2), dtype=torch.float32, device="cuda")
    d_rx = d_rows[:, 0]
    for k, roll in enumerate(ADJ_ROLLS[2 - a.adjacent_sides:] if adjacent_db else ()):
        d_rows[:, 1 + k, :F * S] = torch.roll(d_iq, roll, 0)
    d_wide = torch.zeros((E, n_wide, 2), dtype=torch.float32, device="cuda") if adjacent_db else None
    d_back = torch.zeros((E, n_out, 2), dtype=torch.float32, device="cuda") if adjacent_db else None
    d_rs = torch.zeros((E, n_out, 2), dtype=torch.float32, device="cuda") if clock_ppm else None
    sdt, rdt = np.dtype(dabgpu.SYNC_STATE_DTYPE), np.dtype(dabgpu.RESULT_DTYPE)
    cifs = torch.from_numpy(pay.reshape(4 * F, nb)).cuda()
    text = [f"# Receiver sensitivity: FIB CRC pass rate and MSC byte-error rate against SNR", "",
            f"Device: AMD Instinct MI355X ({torch.cuda.get_device_properties(0).gcnArchName}).  {E} receivers x {F} mode I frames per point, one transmission, a noise seed per receiver; "
            f"FIBs of every frame ({E * F * 12} per point), sub-channel bytes of the {4 * F - 15} CIFs from CIF 15 on "
            f"(per point: {', '.join(f'{name} {E * (4 * F - 15) * sum(spans[i][1] for i in range(len(subs)) if owner[i] == li)}' for li, (name, _) in enumerate(LEVELS))} bytes).  "
            "No carrier or timing offset.  `python tools/waterfall.py`.", ""]
    if csi:
        fading_args = "" if a.doppler_hz is None else f" --profile {a.profile or 'tu6'} --doppler-hz {a.doppler_hz:g}"
        text = [f"# Receiver sensitivity of the two soft-decision policies{' (fading channel, appended)' if a.doppler_hz is not None else ''}", "",
                f"Device: AMD Instinct MI355X ({torch.cuda.get_device_properties(0).gcnArchName}).  The run of `waterfall.md` with the receiver call switched: every cell is "
                f"`normalised -> csi` (dabgpu_ofdm_sync_demod_frames -> dabgpu_ofdm_sync_demod_frames_soft, DABGPU_SOFT_CSI, level {a.soft_level:g}) on the SAME received samples.  "
                f"{E} receivers x {F} mode I frames per point, FIBs of every frame ({E * F * 12} per point), sub-channel bytes of the {4 * F - 15} CIFs from CIF 15 on.  "
                f"`python tools/waterfall.py --soft-bits csi{fading_args}`; "
                "the verdict line is the csi policy's.", ""]
    if branch_path:
        fading_args = "" if a.doppler_hz is None else f" --profile {a.profile or 'tu6'} --doppler-hz {a.doppler_hz:g}"
        text = [f"# Receiver sensitivity with receive diversity: {K} branches per receiver", "",
                f"Device: AMD Instinct MI355X ({torch.cuda.get_device_properties(0).gcnArchName}).  Every receiver hears {K} realisations of the channel (a noise seed"
                f"{'' if a.doppler_hz is None else ' and a fading seed'} per branch): dabgpu_ofdm_sync_demod_frames_branch per branch (DABGPU_SOFT_CSI, level {a.soft_level:g}), "
                f"dabgpu_diversity_combine_frames over the branches' products, scales and sync records into the decoder's ring.  Every cell is `single -> combined`: branch 0 "
                f"decoded alone, and the combination, on the SAME received samples.  {E} receivers x {F} mode I frames per point, FIBs of every frame ({E * F * 12} per point), "
                f"sub-channel bytes of the {4 * F - 15} CIFs from CIF 15 on.  SNR is per branch.  "
                f"`python tools/waterfall.py --branches {K} --streams {E} --frames {F} --snr {a.snr}{fading_args}`; the verdict line is the combination's.", ""]
        if mrc:
            how = {"unit": "no weights (every branch 1)", "estimated": "the weight arrays dabgpu_noise_estimate_frames wrote from every branch's slice and sync records",
                   "banded": f"the band weights dabgpu_noise_profile_frames wrote from every branch's slice and sync records (alpha {a.alpha:g}, the state carried from "
                             "frame to frame), applied by dabgpu_diversity_combine_frames_banded",
                   "banded-dd": f"the band weights dabgpu_dd_profile_frames wrote from every branch's own DQPSK products and sync records (alpha {a.alpha:g}, the state "
                                "carried from frame to frame), applied by dabgpu_diversity_combine_frames_banded",
                   "true": "the true weights 1 / (2 noise_sigma^2) of every branch's channel stream"}[a.weights]
            text = [f"# Receive diversity with {'band weights' if banded else 'branches of unequal noise'}: weights {a.weights}", "",
                    f"Device: AMD Instinct MI355X ({torch.cuda.get_device_properties(0).gcnArchName}).  The run of `waterfall_diversity.md` with the branches' noise raised by "
                    f"{', '.join(f'{d:g}' for d in branch_db)} dB (SNR is that of a branch without extra noise) and the combination made with {how}.  Every cell is "
                    f"`single -> combined`: branch 0 decoded alone, and the combination, on the SAME received samples.  {E} receivers x {F} mode I frames per point, FIBs of "
                    f"every frame ({E * F * 12} per point), sub-channel bytes of the {4 * F - 15} CIFs from CIF 15 on.  "
                    f"`python tools/waterfall.py --branches {K} --branch-noise-db {','.join(f'{d:g}' for d in branch_db)} --weights {a.weights} --streams {E} --frames {F} "
                    f"--snr {a.snr}{fading_args}{' --alpha %g' % a.alpha if banded else ''}{' --interferer ' + a.interferer if jam else ''}{' --interferer-source device' if jam and a.interferer_source == 'device' and not jam_gate else ''}{' --interferer-gate ' + a.interferer_gate if jam_gate else ''}"
                    f"{' --append' if a.append else ''}`; the verdict line is the combination's."
                    + (f"  Interferer: Gaussian noise {jam[1]:g} kHz wide {jam[0]:+g} kHz from the centre, {jam[2]:+g} dB relative to the signal, a seed per stream; the "
                       "frame scale rests on the power of the phase reference symbol, interferer included." if jam else "")
                    + (f"  The interferer is gated: on for {jam_gate['gate_on']} of every {jam_gate['gate_period']} samples from sample {jam_gate['gate_offset']} on." if jam_gate else ""), ""]
    if blank:
        text = ["# Receiver sensitivity with and without the impulse blanker", "",
                f"Device: AMD Instinct MI355X ({torch.cuda.get_device_properties(0).gcnArchName}).  The run of `waterfall.md` with every receiver run twice on the SAME received "
                f"samples: as they are, and through dabgpu.Blanker (threshold {a.blank:g}, gap 8, window 16, guard 1 blocks of 32 samples); every cell is `unblanked -> blanked`.  "
                + (f"Interferer: white noise from dabgpu.Interferer behind a gate, on for {gate[1]} of every {gate[0]} samples, {gate[2]:+g} dB relative to the signal while on, "
                   "a seed per stream.  " if gate else "No interferer.  ") +
                f"{E} receivers x {F} mode I frames per point, FIBs of every frame ({E * F * 12} per point), sub-channel bytes of the {4 * F - 15} CIFs from CIF 15 on.  "
                f"`python tools/waterfall.py --blank {a.blank:g}{' --interferer-gate ' + a.interferer_gate if gate else ''} --streams {E} --frames {F} --snr {a.snr}`; "
                "the verdict line is the blanked receiver's.", ""]
        blanker = dabgpu.Blanker(ctx, [dabgpu.blanker_stream(threshold=a.blank) for _ in range(E)])
        d_blank = torch.zeros((E, n_rx, 2), dtype=torch.float32, device="cuda")
        d_mask = torch.zeros((E, dabgpu.blanker_mask_words(n_rx)), dtype=torch.int32, device="cuda")
    verdicts = []
    profiles, fading =[(n, t, None, None) for n, t in PROFILES], None
    if adjacent_db:
        text = [f"# Adjacent blocks (appended by `python tools/waterfall.py --adjacent-db {a.adjacent_db} --adjacent-sides {a.adjacent_sides}`)", "",
                f"Device: AMD Instinct MI355X ({torch.cuda.get_device_properties(0).gcnArchName}).  The white-noise channel of the first table followed by the combiner and the "
                f"channeliser (D = 4): the block {ADJ_OFFSET / 1e3:g} kHz above the centre of an 8.192 MS/s capture, a neighbour 1.712 MHz "
                f"{'to either side' if a.adjacent_sides == 2 else 'above it'} (the clean transmission rolled by {' and '.join(str(r) for r in ADJ_ROLLS[2 - a.adjacent_sides:])} samples), "
                f"each the given level above the wanted block's signal power; {E} receivers x {F} mode I frames per point, byte counts per point as above.", ""]
        profiles = [(f"white noise, neighbour{'s' if a.adjacent_sides == 2 else ''} {adb:+g} dB", PROFILES[0][1], None, adb) for adb in adjacent_db]
    if clock_ppm:
        text = [f"# Sampling-clock error (appended by `python tools/waterfall.py --clock-ppm {a.clock_ppm}`)", "",
                f"Device: AMD Instinct MI355X ({torch.cuda.get_device_properties(0).gcnArchName}).  The white-noise channel of the first table followed by the resampler "
                f"(step 1 + ppm 1e-6, the noise resampled too): {E} receivers x {F} mode I frames per point, byte counts per point as above.  The frame start drifts "
                "by ppm 1e-6 x 196608 samples per frame; every frame is synchronised from a slice at its nominal position.", ""]
        profiles = [(f"white noise, sampling clock {ppm:g} ppm off", PROFILES[0][1], ppm, None) for ppm in clock_ppm]
    if a.doppler_hz is not None:
        prof = dabgpu.channel_profile(a.profile or "tu6")
        profiles = [(f"{a.profile or 'tu6'} (as recalled from COST 207), Doppler {a.doppler_hz:g} Hz, a fading seed per receiver, + noise", prof["taps"], None, None)]
        fading = dabgpu.channel_fading_plan([dabgpu.channel_stream(taps=prof["taps"]) for _ in range(EC)],
                                            [dabgpu.channel_fading_spec(a.doppler_hz / 2.048e6, 5000 + e, prof["kinds"], prof["rice_k"], prof["los_cos"])
                                             for e in range(EC)])
    for pname, taps, ppm, adb in profiles:
        comb = spl = None
        if adb is not None:
            offs = ([ADJ_OFFSET - ADJ_SPACING] if a.adjacent_sides == 2 else []) + [ADJ_OFFSET + ADJ_SPACING]
            wanted = [dabgpu.channeliser_channel(dabgpu.channeliser_freq(ADJ_OFFSET, ADJ_RATE), 0, 1.0, e) for e in range(E)]
            both = [c for e in range(E) for c in [wanted[e]] + [dabgpu.channeliser_channel(dabgpu.channeliser_freq(o, ADJ_RATE), 0, 10.0 ** (adb / 20.0), e) for o in offs]]
            comb, spl = dabgpu.Channeliser(ctx, both, E, ADJ_D), dabgpu.Channeliser(ctx, wanted, E, ADJ_D)
        rs = dabgpu.Resampler(ctx, [dabgpu.resample_stream(dabgpu.resample_step(ppm=ppm)) for _ in range(E)]) if ppm is not None else None
        h2 = sum(re * re + im * im for _, re, im in taps)
        rows, rows_ref, chan, shares = [], [], [], []
        ch = dabgpu.Channel(ctx, [dabgpu.channel_stream(taps=taps, seed=1000 + e, noise_sigma=1.0) for e in range(EC)], fading=fading)
        for snr in snrs:
            sigma = math.sqrt(1536.0 * h2 / (2.0 * 10.0 ** (snr / 10.0)))
            ch.set_params([dabgpu.channel_stream(taps=taps, seed=1000 + e, noise_sigma=sigma * 10.0 ** (branch_db[e // E] / 20.0)) for e in range(EC)])
            ch.seek(0)
            ch.apply(d_iq, F * S, n_rx, d_rx, in_stride_samples=0, out_stride_bytes=n_rows * n_rx * 8)
            d_use = d_rx
            if jam is not None and a.interferer_source == "device":
                # the library's own source (include/dabgpu.h "Interferer"): a BAND source of that width and power, a seed per stream, in place
                shape = dabgpu.interferer_design(jam[1] / 2048.0)
                amp = math.sqrt(1536.0 * h2 * 10.0 ** (jam[2] / 10.0))
                itf = dabgpu.Interferer(ctx, [dabgpu.interferer_stream([dabgpu.interferer_source(dabgpu.INTERFERER_BAND, amp=amp, shape=0,
                                                                                                  cycles_per_sample=jam[0] / 2048.0, **(jam_gate or {}))],
                                                                          seed=7000 + e)
                                              for e in range(EC)], [shape])
                itf.apply(d_rx, n_rx, d_rx, in_stride_samples=n_rows * n_rx, out_stride_bytes=n_rows * n_rx * 8)
                torch.cuda.synchronize()
                itf.close()
            elif jam is not None:
                # Gaussian noise confined to the band, total power IS_DB over the signal's 1536 h2, a seed per stream
                gen = torch.Generator(device="cuda")
                f_khz = torch.fft.fftfreq(n_rx, device="cuda") * 2048.0
                keep = (f_khz - jam[0] + 1024.0) % 2048.0 - 1024.0
                keep = keep.abs() <= jam[1] / 2.0
                for e in range(EC):
                    gen.manual_seed(7000 + e)
                    X = torch.fft.fft(torch.view_as_complex(torch.randn((n_rx, 2), dtype=torch.float32, device="cuda", generator=gen)))
                    x = torch.fft.ifft(torch.where(keep, X, torch.zeros_like(X)))
                    x = x * math.sqrt(1536.0 * h2 * 10.0 ** (jam[2] / 10.0)) / x.abs().square().mean().sqrt()
                    d_rx[e] += torch.view_as_real(x)
            if gate is not None:
                # the library's burst source (include/dabgpu.h "Interferer"): white noise behind an integer gate, a seed per stream, in place
                amp = math.sqrt(1536.0 * h2 * 10.0 ** (gate[2] / 10.0))
                itf = dabgpu.Interferer(ctx, [dabgpu.interferer_stream([dabgpu.interferer_source(dabgpu.INTERFERER_BAND, amp=amp, shape=-1, gate_period=gate[0],
                                                                                                  gate_on=gate[1], gate_offset=-1000)], seed=7000 + e)
                                              for e in range(EC)])
                itf.apply(d_rx, n_rx, d_rx, in_stride_samples=n_rows * n_rx, out_stride_bytes=n_rows * n_rx * 8)
                torch.cuda.synchronize()
                itf.close()
            if blank:
                blanker.seek(0)
                blanker.apply(d_rx, n_rx, n_rx, d_blank, in_stride_samples=n_rx, d_mask=d_mask)
                torch.cuda.synchronize()
                bits = int(np.unpackbits(d_mask.cpu().numpy().view(np.uint8)).sum())
                shares.append(bits / (E * ((n_rx + 31) // 32)))
                passes = [(dabgpu.SOFT_NORMALISED, d_rx), (dabgpu.SOFT_NORMALISED, d_blank)]
            if comb is not None:
                comb.seek(0); spl.seek(0)
                comb.combine(d_rows, n_rx, n_wide, d_wide, in_stride_samples=n_rx, out_stride_bytes=n_wide * 8)
                spl.split(d_wide, n_wide, n_out, d_back, in_stride_samples=n_wide, out_stride_bytes=n_out * 8)
                d_use = d_back
            if rs is not None:
                rs.seek(0)
                rs.apply(d_rx, n_rx, n_out, d_rs, in_stride_samples=n_rx, out_stride_bytes=n_out * 8)
                d_use = d_rs
            if not blank:
                passes = [(pol, d_use) for pol in policies]                 # (receiver call, its samples)
            if branch_path:
                # receive diversity: ring 0 takes branch 0's own soft bits, ring 1 the combination of the K branches
                soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, a.soft_level)
                d_st = [torch.zeros(E * sdt.itemsize, dtype=torch.uint8, device="cuda") for _ in range(K)]
                dq = [torch.zeros((E, 75, 1536, 2), dtype=torch.float32, device="cuda") for _ in range(K)]
                kb = [torch.zeros((E,), dtype=torch.float32, device="cuda") for _ in range(K)]
                wb = [None] * K
                if a.weights == "estimated":
                    wb = [torch.zeros((E,), dtype=torch.float32, device="cuda") for _ in range(K)]
                elif banded:
                    state = [torch.zeros((E, 128), dtype=torch.float32, device="cuda") for _ in range(K)]
                    bands = [torch.zeros((E, 128), dtype=torch.float32, device="cuda") for _ in range(K)]
                elif a.weights == "true":
                    wb = [torch.full((E,), 1.0 / (2.0 * (sigma * 10.0 ** (branch_db[b] / 20.0)) ** 2), dtype=torch.float32, device="cuda") for b in range(K)]
                rings = [torch.zeros((E, H, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda") for _ in range(2)]
                own = torch.zeros((E, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
                d_fib = torch.zeros((E, 4, 96), dtype=torch.uint8, device="cuda"); fres = torch.zeros((E * 4, 16), dtype=torch.uint8, device="cuda")
                msc = torch.zeros((E, 4, nb), dtype=torch.uint8, device="cuda"); mres = torch.zeros((E * 4 * len(subs), 16), dtype=torch.uint8, device="cuda")
                crc_ok, crc_n = [0, 0], [0, 0]
                err = [[0] * len(LEVELS) for _ in range(2)]; tot = [[0] * len(LEVELS) for _ in range(2)]
                for j in range(F):
                    a0 = NULL + j * S - p_lead
                    lo = max(a0, 0)                                     # (frame 0's slice begins in front of the stream when it holds the NULL)
                    for b in range(K):
                        sl = torch.zeros((E, stride, 2), dtype=torch.float32, device="cuda")
                        seg = d_use[b * E:(b + 1) * E, lo:a0 + stride]
                        sl[:, lo - a0:lo - a0 + seg.shape[1]] = seg
                        if b == 0:
                            rings[0][:, j % H].zero_()                  # (a frame the synchroniser refuses stays an erasure, not a stale frame)
                        ctx.ofdm_sync_demod_frames_branch(sl, E, stride, p_lead, d_st[b], rings[0][:, j % H] if b == 0 else own, soft, dq[b],
                                                          bits_frame_stride=H * dabgpu.NB_FRAME_BITS if b == 0 else 0, soft_scale=kb[b])
                        if a.weights == "estimated":
                            ctx.noise_estimate(sl, E, stride, p_lead - NULL, states=d_st[b], weight=wb[b])
                        if dd:
                            ctx.dd_profile(dq[b], E, sync=d_st[b], profile_in=state[b], alpha=a.alpha, profile_out=state[b], band_weight=bands[b])
                        elif banded:
                            ctx.noise_profile(sl, E, stride, p_lead - NULL, states=d_st[b], profile_in=state[b], alpha=a.alpha, profile_out=state[b],
                                              band_weight=bands[b])
                    ctx.diversity_combine([(dq[b], kb[b], wb[b], d_st[b]) for b in range(K)], E, rings[1][:, j % H], bits_frame_stride=H * dabgpu.NB_FRAME_BITS,
                                          band_weights=bands if banded else None)
                    for r in range(2):
                        ctx.decode_frames(rings[r], E, H * dabgpu.NB_FRAME_BITS, H, j % H, subs, d_fib, fres, msc, 4 * nb, mres)
                        torch.cuda.synchronize()
                        masks = fres.cpu().numpy().view(rdt)["crc_ok_mask"].reshape(-1)
                        crc_ok[r] += int(sum(bin(int(m) & 7).count("1") for m in masks)); crc_n[r] += 3 * masks.size
                        for c in range(4):
                            if 4 * j + c < 15:
                                continue
                            bad = (msc[:, c] != cifs[4 * j + c - 15][None, :])
                            for i, (off, n) in enumerate(spans):
                                err[r][owner[i]] += int(bad[:, off:off + n].sum()); tot[r][owner[i]] += E * n
                rows_ref.append((snr, crc_ok[0] / crc_n[0], [e / t for e, t in zip(err[0], tot[0])], tot[0]))
                rows.append((snr, crc_ok[1] / crc_n[1], [e / t for e, t in zip(err[1], tot[1])], tot[1]))
            for pi, (pol, d_src) in enumerate(passes if not branch_path else []):
                d_st = torch.zeros(E * sdt.itemsize, dtype=torch.uint8, device="cuda")
                hist = torch.zeros((E, H, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
                d_fib = torch.zeros((E, 4, 96), dtype=torch.uint8, device="cuda"); fres = torch.zeros((E * 4, 16), dtype=torch.uint8, device="cuda")
                msc = torch.zeros((E, 4, nb), dtype=torch.uint8, device="cuda"); mres = torch.zeros((E * 4 * len(subs), 16), dtype=torch.uint8, device="cuda")
                crc_ok, crc_n = 0, 0
                if a.ber:
                    fic_ber = torch.zeros((E, 4, 16), dtype=torch.uint8, device="cuda"); msc_ber = torch.zeros((E, 4, len(subs), 16), dtype=torch.uint8, device="cuda")
                    m_err = m_bits = t_err = t_bits = 0
                err = [0] * len(LEVELS); tot = [0] * len(LEVELS)
                for j in range(F):
                    a0 = NULL + j * S - P_LEAD
                    sl = torch.zeros((E, STRIDE, 2), dtype=torch.float32, device="cuda")
                    seg = d_src[:, a0:a0 + STRIDE]
                    sl[:, :seg.shape[1]] = seg
                    if pol == dabgpu.SOFT_NORMALISED:
                        ctx.ofdm_sync_demod_frames(sl, E, STRIDE, P_LEAD, d_st, hist[:, j % H], bits_frame_stride=H * dabgpu.NB_FRAME_BITS)
                    else:
                        ctx.ofdm_sync_demod_frames_soft(sl, E, STRIDE, P_LEAD, d_st, hist[:, j % H], dabgpu.SoftCfg(pol, a.soft_level),
                                                        bits_frame_stride=H * dabgpu.NB_FRAME_BITS)
                    ctx.decode_frames(hist, E, H * dabgpu.NB_FRAME_BITS, H, j % H, subs, d_fib, fres, msc, 4 * nb, mres)
                    if a.ber:
                        ctx.ber_frames(hist, E, H * dabgpu.NB_FRAME_BITS, H, j % H, subs, d_fib, msc, 4 * nb, fic_ber, msc_ber)
                        torch.cuda.synchronize()
                        recs = [fic_ber.cpu().numpy().view(bdt).reshape(E, 4)] + [msc_ber.cpu().numpy().view(bdt).reshape(E, 4, len(subs))[:, c]
                                                                                  for c in range(4) if 4 * j + c >= 15]
                        m_err += sum(int(r["n_errors"].sum()) for r in recs); m_bits += sum(int(r["n_bits"].sum()) for r in recs)
                        fr, pos = consumed[j]
                        soft = hist[:, fr % H, pos]
                        t_err += int(((soft != 0) & ((soft >= 0) != sent[fr, pos][None, :])).sum()); t_bits += int((soft != 0).sum())
                    torch.cuda.synchronize()
                    masks = fres.cpu().numpy().view(rdt)["crc_ok_mask"].reshape(-1)
                    crc_ok += int(sum(bin(int(m) & 7).count("1") for m in masks)); crc_n += 3 * masks.size
                    for c in range(4):
                        if 4 * j + c < 15:
                            continue
                        bad = (msc[:, c] != cifs[4 * j + c - 15][None, :])
                        for i, (off, n) in enumerate(spans):
                            err[owner[i]] += int(bad[:, off:off + n].sum()); tot[owner[i]] += E * n
                if pi == len(passes) - 1:
                    rows.append((snr, crc_ok / crc_n, [e / t for e, t in zip(err, tot)], tot))
                    if a.ber:
                        assert m_bits == t_bits
                        chan.append((m_err / m_bits, t_err / t_bits))
                else:
                    rows_ref.append((snr, crc_ok / crc_n, [e / t for e, t in zip(err, tot)], tot))
        ch.close()
        if rs is not None:
            rs.close()
        if comb is not None:
            comb.close(); spl.close()
        if csi or branch_path or blank:
            # both policies side by side: normalised -> csi in every cell (receive diversity: single -> combined)
            text += [f"## {pname}", "", "| SNR dB | FIB CRC pass | " + " | ".join(name + " byte errors" for name, _ in LEVELS) + " |", "|---|---|" + "---|" * len(LEVELS)]
            fmt = lambda r: f"{r:.2e}" if r else "0"
            text += [f"| {snr:g} | {ok0:.4f} -> {ok:.4f} | " + " | ".join(f"{fmt(r0)} -> {fmt(r)}" for r0, r in zip(ber0, ber)) + " |"
                     for (snr, ok0, ber0, _), (_, ok, ber, _) in zip(rows_ref, rows)]
        else:
            text += [f"## {pname}", "", "| SNR dB | FIB CRC pass | " + " | ".join(name + " byte errors" for name, _ in LEVELS) + " |", "|---|---|" + "---|" * len(LEVELS)]
            text += [f"| {snr:g} | {ok:.4f} | " + " | ".join(f"{r:.2e}" if r else "0" for r in ber) + " |" for snr, ok, ber, _ in rows]
        if blank:
            text += ["", "Blocks the blanker zeroed, of all: " + ", ".join(f"{snr:g} dB {100.0 * sh:.2f} %" for (snr, _, _, _), sh in zip(rows, shares)) + "."]
        if a.ber:
            n0 = len(text) - len(rows) - 2
            text[n0] += " channel BER measured | channel BER true |"; text[n0 + 1] += "---|---|"
            for k, (m, tr) in enumerate(chan):
                text[n0 + 2 + k] += f" {m:.3e} | {tr:.3e} |"
        # acceptance: error-free at the top, non-increasing within counting error, required SNR ordered by level
        top = rows[-1]
        free = top[1] == 1.0 and all(r == 0 for r in top[2])
        mono = True
        for li in range(len(LEVELS)):
            for (s0, _, b0, t0), (s1, _, b1, _) in zip(rows, rows[1:]):
                slack = 3 * math.sqrt(max(b0[li], 1.0 / t0[li]) / t0[li] * 255)        # byte errors come in bursts of a decoder's error event
                mono = mono and b1[li] <= b0[li] + slack
        need = [next((snr for k, (snr, _, ber, _) in enumerate(rows) if all(r[2][li] == 0 for r in rows[k:])), float("inf")) for li in range(len(LEVELS))]
        order = need[0] <= need[1] <= need[2] <= need[3]
        text += ["", f"Error-free at {top[0]:g} dB: {'yes' if free else 'NO'}.  Non-increasing with SNR within the counting error: {'yes' if mono else 'NO'}.  "
                 f"First SNR from which no byte error remains: " + ", ".join(f"{name} {n:g} dB" for (name, _), n in zip(LEVELS, need)) +
                 f" -- ordered 1-A <= 2-A <= 3-A <= 4-A: {'yes' if order else 'NO'}.", ""]
        verdicts.append(free and mono and order)
    if blank:
        blanker.close()
    text = "\n".join(text) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    append = bool(clock_ppm or adjacent_db or ((csi or branch_path) and a.doppler_hz is not None) or a.append)       # (the csi record: white noise and two paths first, the fading run behind them)
    open(a.out, "a" if append else "w").write(("\n" if append else "") + text)
    return 0 if all(verdicts) else 1


if __name__ == "__main__":
    sys.exit(main())
