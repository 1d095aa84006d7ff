"""Writes tests/golden/packet_fec_vectors.npz: what the reference's own Reed_Solomon_Decoder (8, 0x11D, 0, 1, 16, 51) and
MSC_Reed_Solomon_Data_Packet_Processor answer for inputs made by tests/packet_fec_model.py.

    python tests/golden/make_golden_packet_fec.py [reference tree]

A small driver (below) is compiled in a temporary directory against msc_reed_solomon_data_packet_processor.cpp and reed_solomon_decoder.cpp
where they lie, with the flags the oracle uses for the reference's objects plus -DNDEBUG (a release build: the asserts of the pop walk are
off, as in the reference's own presets).  Only data is written.

(a) RS words: sparse and random words with 0..10 symbol errors, errors in parity only, and words built so that the decoder reports a
    position inside the 51 padding symbols (the parity of a single non-zero PADDING symbol, with further errors on top): Decode's count, its
    positions and the word it leaves.
(b) packet sequences, each a list of buffers as Basic_Data_Packet_Channel::ProcessFECPackets walks them: the ReadPacket return values and the
    callback log (bytes, flag) in order."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import packet_fec_model as M  # noqa: E402

DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
#include "dab/algorithms/reed_solomon_decoder.h"
#include "dab/msc/msc_reed_solomon_data_packet_processor.h"

static uint32_t rd32(FILE* f) { uint32_t v = 0; if (fread(&v, 4, 1, f) != 1) return 0; return v; }
static void wr32(FILE* f, uint32_t v) { fwrite(&v, 4, 1, f); }

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    Reed_Solomon_Decoder dec(8, 0x11D, 0, 1, 16, 51);
    const uint32_t n_words = rd32(in);
    for (uint32_t w = 0; w < n_words; w++) {
        uint8_t word[204];
        if (fread(word, 1, 204, in) != 204) return 3;
        int pos[16];
        for (int i = 0; i < 16; i++) pos[i] = -1;
        const int count = dec.Decode(word, pos, 0);
        wr32(out, (uint32_t)count);
        for (int i = 0; i < 16; i++) wr32(out, (uint32_t)((i < count) ? pos[i] : -1));
        fwrite(word, 1, 204, out);
    }
    const uint32_t n_seq = rd32(in);
    for (uint32_t s = 0; s < n_seq; s++) {
        MSC_Reed_Solomon_Data_Packet_Processor proc;
        std::vector<uint8_t> log;
        uint32_t n_cb = 0;
        proc.SetCallback([&](tcb::span<const uint8_t> p, bool corrected) {
            log.push_back(corrected ? 1 : 0);
            const uint32_t n = (uint32_t)p.size();
            for (int k = 0; k < 4; k++) log.push_back((uint8_t)(n >> (8 * k)));
            log.insert(log.end(), p.begin(), p.end());
            n_cb++;
        });
        std::vector<uint32_t> rets;
        const uint32_t n_bufs = rd32(in);
        for (uint32_t b = 0; b < n_bufs; b++) {
            const uint32_t len = rd32(in);
            std::vector<uint8_t> buf(len);
            if (len && fread(buf.data(), 1, len, in) != len) return 3;
            tcb::span<const uint8_t> rest(buf);
            while (!rest.empty()) {
                const size_t used = proc.ReadPacket(rest);
                rets.push_back((uint32_t)used);
                rest = rest.subspan(used);
            }
        }
        wr32(out, (uint32_t)rets.size());
        for (uint32_t r : rets) wr32(out, r);
        wr32(out, n_cb);
        wr32(out, (uint32_t)log.size());
        fwrite(log.data(), 1, log.size(), out);
    }
    fclose(out);
    return 0;
}
"""


def build_driver(ref, tmp):
    import torch
    fmt_inc = os.path.join(os.path.dirname(torch.__file__), "include")
    src = os.path.join(tmp, "driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "driver")
    flags = ["-O2", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-DFMT_HEADER_ONLY", "-DNDEBUG", "-w", "-I" + os.path.join(ref, "src"),
             "-I" + fmt_inc]
    subprocess.check_call(["g++"] + flags + [src, os.path.join(ref, "src", "dab", "msc", "msc_reed_solomon_data_packet_processor.cpp"),
                                             os.path.join(ref, "src", "dab", "algorithms", "reed_solomon_decoder.cpp"), "-o", exe])
    return exe


def run_driver(exe, tmp, words, sequences):
    blob = [np.uint32(len(words)).tobytes()] + [np.asarray(w, np.uint8).tobytes() for w in words]
    blob.append(np.uint32(len(sequences)).tobytes())
    for bufs in sequences:
        blob.append(np.uint32(len(bufs)).tobytes())
        for b in bufs:
            blob += [np.uint32(len(b)).tobytes(), np.asarray(b, np.uint8).tobytes()]
    with open(os.path.join(tmp, "in.bin"), "wb") as f:
        f.write(b"".join(blob))
    subprocess.check_call([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")])
    raw = np.fromfile(os.path.join(tmp, "out.bin"), np.uint8)
    at = 0

    def u32(n=1):
        nonlocal at
        v = raw[at:at + 4 * n].view("<u4").copy()
        at += 4 * n
        return v
    counts, positions, fixed = [], [], []
    for _ in words:
        counts.append(int(u32().view("<i4")[0]))
        positions.append(u32(16).view("<i4"))
        fixed.append(raw[at:at + 204].copy())
        at += 204
    logs = []
    for _ in sequences:
        rets = u32(int(u32()[0]))
        n_cb, n_log = int(u32()[0]), int(u32()[0])
        logs.append((rets, n_cb, raw[at:at + n_log].copy()))
        at += n_log
    assert at == raw.size
    return np.array(counts, np.int32), np.array(positions, np.int32), np.array(fixed, np.uint8), logs


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    words, word_kinds = M.golden_rs_words()
    names, sequences = M.golden_sequences()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref, tmp)
        counts, positions, fixed, logs = run_driver(exe, tmp, words, sequences)
    below = [(c > 0 and ((p[:c] - M.PAD) < 0).any()) for c, p in zip(counts, positions)]
    assert any(below), "no word with a reported position inside the padding"
    out = dict(rs_words=np.array(words, np.uint8), rs_kind=np.array(word_kinds), rs_count=counts, rs_positions=positions, rs_fixed=fixed,
               names=np.array(names))
    for i, (bufs, (rets, n_cb, log)) in enumerate(zip(sequences, logs)):
        out[f"buf_len_{i}"] = np.array([len(b) for b in bufs], np.uint32)
        out[f"buf_{i}"] = np.concatenate([np.asarray(b, np.uint8) for b in bufs] + [np.zeros(0, np.uint8)])
        out[f"ret_{i}"] = rets.astype(np.uint32)
        out[f"log_{i}"] = log                         # per callback: flag, u32 length, bytes
        out[f"n_cb_{i}"] = np.uint32(n_cb)
    path = os.path.join(HERE, "packet_fec_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(words)} RS words ({int(sum(below))} with a position inside the padding, counts {sorted(set(counts.tolist()))}), "
          f"{len(sequences)} sequences, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
