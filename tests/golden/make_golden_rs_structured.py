"""Writes tests/golden/rs_structured_vectors.npz: what the reference's own Reed_Solomon_Decoder answers for the structured error patterns of
tests/rs_structured.py, each received as pattern XOR the zero code word.  DATA only.  Run from the repo root:

    python tests/golden/make_golden_rs_structured.py [reference tree]

RS(120,110) goes through ref_rs120_decode of oracle/_ref/libdab_ref.so (the decoder as AAC_Frame_Processor constructs it), RS(204,188)
through the driver of make_golden_packet_fec.py (the decoder as MSC_Reed_Solomon_Data_Packet_Processor constructs it), compiled in a
temporary directory.  Per code the file holds the patterns, their kinds, and per word Decode's count, its positions (in the unshortened
block, in the order of its search, -1 beyond the count) and the word it leaves."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import oracle as O  # noqa: E402
import rs_structured as RS  # noqa: E402
import make_golden_packet_fec as P  # noqa: E402


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    O.build()
    R = O.ref()
    assert R is not None and hasattr(R, "ref_rs120_decode"), "oracle/_ref/libdab_ref.so missing: needs the reference tree"
    out = {}
    # ---- RS(120,110) ----
    pats, kinds = RS.words(120)
    counts, fixed, positions = [], [], []
    for w in pats:
        a, pos = w.copy(), np.full(10, -1, np.int32)
        c = int(R.ref_rs120_decode(a.ctypes.data, pos.ctypes.data))
        pos[max(c, 0):] = -1
        counts.append(c); fixed.append(a); positions.append(pos)
    out.update(rs120_patterns=pats, rs120_kind=np.array(kinds), rs120_count=np.array(counts, np.int32), rs120_positions=np.stack(positions),
               rs120_fixed=np.stack(fixed))
    # ---- RS(204,188) ----
    pats, kinds = RS.words(204)
    with tempfile.TemporaryDirectory() as tmp:
        exe = P.build_driver(ref, tmp)
        counts, positions, fixed, _ = P.run_driver(exe, tmp, list(pats), [])
    out.update(rs204_patterns=pats, rs204_kind=np.array(kinds), rs204_count=counts, rs204_positions=positions, rs204_fixed=fixed)
    path = os.path.join(HERE, "rs_structured_vectors.npz")
    np.savez_compressed(path, **out)
    for code in (120, 204):
        c = out[f"rs{code}_count"]
        print(f"RS({code}): {len(c)} words, counts {dict(zip(*[v.tolist() for v in np.unique(c, return_counts=True)]))}")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
