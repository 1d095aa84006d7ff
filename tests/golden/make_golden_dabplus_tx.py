"""Generates tests/golden/dabplus_tx_vectors.npz: inputs of the DAB+ super-frame encoder, what tests/dabplus_tx_model.py makes of them, and what
the reference's OWN AAC_Frame_Processor (compiled in place into oracle/_ref/libdab_ref.so) reported when it was given those bytes: the 12 event
fields of ref_aac_process after the fifth logical frame.  DATA only.  Run from the repo root: python tests/golden/make_golden_dabplus_tx.py

What each group of cases is there to catch (every accepted case checks parity, CRCs and fire code at once; a wrong byte anywhere fails it):
  rand_<n>_<d>     the four unit counts at every size: 1, 2, 3 and 5 twelve-bit header fields = odd and even numbers, with and without pad bits
                   (header packing); n >= 48 has more than one code word (byte interleaving); 768 / 792 / 816 sit around the 32-code-word
                   threshold of the parity mapping, 1536 is the full wavefront
  zeros_*, ones_*  all-zero / all-0xFF payloads: zero symbols contribute nothing to the parity, the CRC's start value and inversion show
  empty_*          zero-length units (CRC of nothing = 0x0000) and one-byte units
  big_*            one unit takes nearly all the room (the CRC chunking at its longest, 32 / 16 / 8 lanes)
  edge_4095        a 1536-byte frame whose second unit starts at 4095: the largest value a header field holds
  bad_*            refused super frames: status and zero frames
Which case fails first when ONE step of the encoder is wrong (every accepted case fails then; these are the smallest that isolate it):
  parity           rand_24_13: one code word, so a wrong parity byte is the only thing interleaving cannot hide; zeros_48 for the "zero symbol
                   contributes nothing" branch
  interleaving     rand_48_13 (n_rs = 2, the smallest with a stride) and rand_72_6f (n_rs = 3, no power of two)
  unit CRC         ones_72 (start value and inversion), empty_24 and empty_72 -- the ONLY cases with zero-length units, whose CRC 0x0000 is a
                   branch of its own in crc_lanes -- and onebyte_24, the ONLY case with one-byte units, the other special branch
  fire code        rand_24_51 and empty_24: six units put unit bytes and, in empty_24, CRC bytes inside bytes 2..10 that the fire code covers
  header packing   rand_24_3a (1 field, 4 pad bits), rand_24_6f (2 fields, none), rand_24_13 (3 fields, 4 pad bits), rand_24_51 (5 fields, 4 pad
                   bits); edge_4095 sets every bit of a field"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle as O  # noqa: E402
import dabplus_tx_model as T  # noqa: E402

DESCRIPTORS = (0x13, 0x3A, 0x51, 0x6F)          # (dac_rate, sbr) = 00, 01, 10, 11 -> 4, 2, 6, 3 units; the other bits vary


def cases(rng):
    out = []

    def add(name, n, d, lens, fill=None):
        aus = [rng.integers(0, 256, l, dtype=np.uint8) if fill is None else np.full(l, fill, np.uint8) for l in lens]
        out.append((name, n, d, aus))

    for n in (24, 48, 72, 192, 768, 792, 816, 1536):
        for d in DESCRIPTORS:
            if n in (768, 816) and d in DESCRIPTORS[1:3]:
                continue
            add(f"rand_{n}_{d:02x}", n, d, T.split_lengths(rng, d, n))
    add("zeros_48", 48, 0x13, T.split_lengths(rng, 0x13, 48), fill=0)
    add("ones_72", 72, 0x6F, T.split_lengths(rng, 0x6F, 72), fill=0xFF)
    add("empty_24", 24, 0x51, T.split_lengths(rng, 0x51, 24, "zeros"))
    add("empty_72", 72, 0x13, T.split_lengths(rng, 0x13, 72, "zeros"))
    add("onebyte_24", 24, 0x51, [1, 1, 1, 1, 1, 110 - 11 - 12 - 5])
    add("big_72", 72, 0x3A, T.split_lengths(rng, 0x3A, 72, "first_big"))
    add("big_792", 792, 0x13, T.split_lengths(rng, 0x13, 792, "first_big"))
    add("big_1536", 1536, 0x51, T.split_lengths(rng, 0x51, 1536, "zeros"))
    room = 110 * 64 - 5 - 4
    add("edge_4095", 1536, 0x3A, [4095 - 5 - 2, room - (4095 - 5 - 2)])
    add("bad_start_4096", 1536, 0x3A, [4096 - 5 - 2, room - (4096 - 5 - 2)])
    good = T.split_lengths(rng, 0x6F, 96)
    add("bad_short_96", 96, 0x6F, [good[0], good[1], good[2] - 1])
    add("bad_long_96", 96, 0x6F, [good[0] + 1, good[1], good[2]])
    for n in (0, 23, 25, 1560):
        add(f"bad_size_{n}", n, 0x13, [10, 20, 30, 40])
    return out


def reference_events(R, frames, n):
    """the five logical frames into a fresh AAC_Frame_Processor of the reference -> (12 event fields, unit lengths, unit bytes) after the last"""
    h = C.c_void_p(R.ref_aac_create())
    for j in range(5):
        fr = np.ascontiguousarray(frames[j * n:(j + 1) * n])
        o = np.zeros(12, np.int32); al = np.zeros(6, np.int32); ab = np.zeros((6, 8192), np.uint8)
        R.ref_aac_process(h, fr.ctypes.data, n, o.ctypes.data, al.ctypes.data, ab.ctypes.data, 8192)
    R.ref_aac_destroy(h)
    return o, al, ab


def main():
    R = O.ref()
    assert R is not None and hasattr(R, "ref_aac_create"), "oracle/_ref/libdab_ref.so missing: needs the reference's sources"
    rng = np.random.default_rng(20261017)
    out, names = {}, []
    all_cases = cases(rng)
    N = len(all_cases)
    out["frame_bytes"] = np.zeros(N, np.uint32); out["descriptor"] = np.zeros(N, np.uint8); out["au_len"] = np.zeros((N, 6), np.uint16)
    out["status"] = np.zeros(N, np.int32); out["ref_events"] = np.zeros((N, 12), np.int32); out["has_ref"] = np.zeros(N, np.uint8)
    for i, (name, n, d, aus) in enumerate(all_cases):
        frames, status = T.encode(d, aus, n)
        names.append(name)
        out["frame_bytes"][i], out["descriptor"][i], out["status"][i] = n, d, status
        out["au_len"][i, :len(aus)] = [len(a) for a in aus]
        out[f"au_{i}"] = np.concatenate(aus + [np.zeros(0, np.uint8)])
        out[f"frames_{i}"] = frames
        if status != T.STATUS_FRAME_SIZE:
            ev, al, ab = reference_events(R, frames, n)
            out["ref_events"][i], out["has_ref"][i] = ev, 1
            if status == 0:
                na = T.num_aus_of(d)
                # the reference's verdict: no fire-code or RS event, header read back, every unit delivered byte for byte, none bad
                assert ev[0] == 0 and ev[1] == -1 and ev[2] == 1 and ev[8] == na and int(np.uint32(ev[9])) == (1 << na) - 1 and ev[10] == 0, (name, ev)
                for a in range(na):
                    assert al[a] == len(aus[a]) and np.array_equal(ab[a][:al[a]], aus[a]), (name, a)
            else:
                assert ev[0] == 0 and ev[1] == -1 and ev[2] == 1 and ev[9] == 0 and ev[10] == 0, (name, ev)       # zero frames: a header and no unit
    out["names"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "dabplus_tx_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", N, "cases; status:", np.unique(out["status"], return_counts=True))


if __name__ == "__main__":
    main()
