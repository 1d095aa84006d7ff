"""The numpy model of packet mode with FEC (tests/packet_fec_model.py) against the reference's answers committed in
tests/golden/packet_fec_vectors.npz (made by tests/golden/make_golden_packet_fec.py from the reference's own decoder and processor), byte
for byte and flag for flag; CRC known answers; the encoder's rows have zero syndromes; properties of the packet layout."""
import os

import numpy as np
import pytest

import packet_fec_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vectors():
    return np.load(os.path.join(ROOT, "tests", "golden", "packet_fec_vectors.npz"))


def sequence(v, i):
    lens = v[f"buf_len_{i}"]
    ends = np.cumsum(lens)
    return [v[f"buf_{i}"][e - n:e] for n, e in zip(lens, ends)]


def test_fixture_inputs_are_the_models(vectors):
    words, kinds = M.golden_rs_words()
    assert np.array_equal(np.array(words, np.uint8), vectors["rs_words"]) and kinds == [str(k) for k in vectors["rs_kind"]]
    names, seqs = M.golden_sequences()
    assert names == [str(n) for n in vectors["names"]]
    for i, bufs in enumerate(seqs):
        got = sequence(vectors, i)
        assert len(got) == len(bufs) and all(np.array_equal(a, b) for a, b in zip(got, bufs)), names[i]


def test_rs_decoder_equals_the_reference(vectors):
    v = vectors
    below = 0
    for w, count, pos, fixed, kind in zip(v["rs_words"], v["rs_count"], v["rs_positions"], v["rs_fixed"], v["rs_kind"]):
        c, locs, out = M.rs_decode(w)
        assert c == int(count), kind
        assert locs == [int(p) for p in pos[:max(c, 0)]], kind
        assert np.array_equal(np.array(out, np.uint8), fixed), kind
        below += c > 0 and any(p < M.PAD for p in locs)
    assert below >= 1, "no word whose reported position lies inside the padding"
    counts = set(int(c) for c in v["rs_count"])
    assert counts >= set(range(-1, 9))
    # errors in parity only: reported, the data untouched
    for w, count, fixed, kind in zip(v["rs_words"], v["rs_count"], v["rs_fixed"], v["rs_kind"]):
        if str(kind) == "parity_only":
            assert count > 0 and np.array_equal(w[:M.RS_K], fixed[:M.RS_K])


def test_processor_equals_the_reference(vectors):
    v = vectors
    names = [str(n) for n in v["names"]]
    seen_corrected = seen_uncorrected = seen_minus_one = seen_discard = 0
    for i, name in enumerate(names):
        proc = M.Processor()
        rets = []
        for buf in sequence(v, i):
            rets += proc.read_buffer(buf)
        assert rets == [int(r) for r in v[f"ret_{i}"]], name
        ref = M.parse_log(v[f"log_{i}"])
        assert len(ref) == int(v[f"n_cb_{i}"]) == len(proc.log), name
        for k, ((p, flag), (rp, rflag)) in enumerate(zip(proc.log, ref)):
            assert flag == rflag and np.array_equal(p, rp), (name, k)
        seen_corrected += sum(f for _, f in ref)
        seen_uncorrected += sum(not f for _, f in ref)
        seen_minus_one += sum(c < 0 for _, cnt in proc.fec_frames for c in cnt)
        seen_discard += proc.discarded
    assert seen_corrected and seen_uncorrected and seen_minus_one and seen_discard


def test_fixture_situations(vectors):
    """the situations the fixture is there for do occur in it"""
    v = vectors
    names = [str(n) for n in v["names"]]

    def run(name):
        proc = M.Processor()
        for buf in sequence(v, names.index(name)):
            proc.read_buffer(buf)
        return proc
    p = run("pop_into_fec_region")
    last, flag = p.log[-1]
    assert flag and len(last) == 96 and last[24] == (M.FEC_ADDR >> 8) and last[25] == 0xFE          # FEC packet 0 inside the last packet handed out
    assert p.fec_frames[0][1][0] == 1 and p.fec_frames[0][1][5] == -1
    assert sum(len(q) for q, _ in p.log) == M.APP + 72
    p = run("uncorrectable_row0_wrong_header")
    assert p.fec_frames[0][1][0] == -1 and any(len(q) == 48 for q, _ in p.log)
    p = run("data_length_longer")
    assert p.fec_frames[0][1][0] == 1 and all(len(q) == 24 for q, _ in p.log) and len(p.log) == 94
    p = run("errors_1_to_8")
    assert p.fec_frames[0][1] == [1, 2, 3, 4, 5, 6, 7, 8, 1, 2, 3, 4]
    p = run("starts_mid_frame_discards")
    assert p.discarded > 0 and p.fec_frames[0][1] == [2] * 12
    for name in ("counter_skipped", "counter_repeated", "counter_starts_at_3", "starts_mid_frame_short_ring"):
        p = run(name)
        assert any(not f for _, f in p.log) and len(p.fec_frames) == 1, name
        assert any(not f and ((int(q[0]) & 3) << 8 | int(q[1])) == M.FEC_ADDR for q, f in p.log), name       # FEC packets handed out uncorrected


def test_crc_known_answers():
    assert M.crc16(b"123456789") == 0xD64E            # CRC-16/GENIBUS: x^16+x^12+x^5+1, start 0xFFFF, inverted
    assert M.crc16(b"") == 0x0000
    assert M.crc16(bytes(22)) == (M.crc16(bytes(21) + b"\x00"))
    p = M.build_packet(dict(group=0, offset=0, length=24, useful=3, flags=3, ci=2), [b"abc"], 0x123)
    assert M.packet_crc_ok(p) and p[0] == (0 << 6 | 2 << 4 | 3 << 2 | 1) and p[1] == 0x23 and p[2] == 3 and bytes(p[3:6]) == b"abc"
    p[5] ^= 1
    assert not M.packet_crc_ok(p)


def test_encoder_rows_have_zero_syndromes():
    rng = np.random.default_rng(7300)
    for lengths in (M.LENGTHS, (24,), (96,)):
        frame, _ = M.random_fec_frame(rng, lengths, max_useful=19)
        for y in range(M.ROWS):
            assert not any(M.syndromes(frame[M.ROW_OFFSETS[y]])), (lengths, y)
        # the FEC packets: counters 0..8, the FEC address, six zero bytes at the end
        fec = frame[M.APP:].reshape(9, 24)
        assert [int(b) >> 2 for b in fec[:, 0]] == list(range(9)) and all(int(b) & 3 == 3 for b in fec[:, 0]) and (fec[:, 1] == 0xFE).all()
        assert not fec[8, 18:].any()
    assert len(M.GEN) == 17 and M.GEN[16] == 1 and all(M.poly_eval(M.GEN, M.EXP[r]) == 0 for r in range(16))


def check_layout(group_len, address, length, fb, start, ci, K):
    st, ent, first, consumed, end_start, end_ci = M.layout(group_len, address, length, fb, start, ci, K)
    assert st == 0
    assert len(first) == K + 1 and first[0] == 0 and first[-1] == len(ent) and end_start == start + K * M.RING
    at = {}
    n_data = 0
    for t in range(K):
        pos = t * M.RING
        for e in ent[first[t]:first[t + 1]]:
            assert e["position"] == pos and e["length"] in M.LENGTHS
            assert (start + pos) % fb + e["length"] <= fb, "a packet crosses a logical-frame boundary"
            pos += e["length"]
            if e["group"] < 0:
                assert e["length"] == 24 and e["useful"] == 0 and e["flags"] == 0
                continue
            assert e["length"] == length and e["useful"] <= length - 5
            assert e["ci"] == (ci + n_data) & 3
            n_data += 1
            g = e["group"]
            assert e["offset"] == at.get(g, 0) and bool(e["flags"] & 2) == (g not in at)
            at[g] = e["offset"] + e["useful"]
            assert bool(e["flags"] & 1) == (at[g] == group_len[g])
            if not e["flags"] & 1:
                assert e["useful"] == length - 5
        assert pos == t * M.RING + M.APP, "an application data table is not 2256 bytes"
    assert end_ci == (ci + n_data) & 3
    assert sorted(at) == list(range(consumed)) and all(at[g] == group_len[g] for g in at)
    return ent, first, consumed


def test_layout_properties_and_reassembly():
    rng = np.random.default_rng(7400)
    for trial in range(40):
        length = int(rng.choice(M.LENGTHS))
        fb = 24 * int(rng.integers(max(1, length // 24), 70))
        if trial % 5 == 0:
            fb = length
        K = int(rng.integers(1, 5))
        group_len = [int(x) for x in rng.integers(0, 700, int(rng.integers(0, 30)))]
        if trial % 7 == 0:
            group_len += [8191, 0, 0, 1]
        start = 24 * int(rng.integers(0, 5000))
        address, ci = int(rng.integers(1, 1022)), int(rng.integers(0, 4))
        ent, first, consumed = check_layout(group_len, address, length, fb, start, ci, K)
        groups = [rng.integers(0, 256, n, dtype=np.uint8) for n in group_len]
        s = M.encode(groups, ent, first, address)
        # through the receive model: every row clean, every packet handed back corrected, the groups reassemble
        res = M.run_frames(M.rx_buffers(s, fb, start))
        assert all(f["rs_count"] == [0] * 12 for f in res["fec_frames"]) and len(res["fec_frames"]) == K
        assert res["counts"][0] == len(ent) and all(r["is_corrected"] and r["crc_ok"] for r in res["records"])
        ra = M.Reassembler(address)
        ra.last_ci = (ci - 1) & 3
        got = ra.feed(res["packets"], res["records"])
        assert got == [bytes(g) for g in groups[:consumed]]


def test_layout_refusals_in_order():
    L = M.layout
    assert L([9000], 0, 25, 7, 5, 0, 1)[0] == M.BAD_ADDRESS
    assert L([9000], 1022, 25, 7, 5, 0, 1)[0] == M.BAD_ADDRESS
    assert L([9000], 1, 25, 7, 5, 0, 1)[0] == M.BAD_LENGTH
    assert L([9000], 1, 96, 7, 5, 0, 1)[0] == M.BAD_FRAME_BYTES
    assert L([9000], 1, 96, 0, 5, 0, 1)[0] == M.BAD_FRAME_BYTES
    assert L([9000], 1, 96, 72, 5, 0, 1)[0] == M.FRAME_TOO_SMALL
    assert L([9000], 1, 96, 96, 5, 0, 1)[0] == M.BAD_GROUP
    assert L([8191], 1, 96, 96, 5, 0, 1)[0] == M.BAD_START
    assert L([8191], 1, 96, 96, 0, 0, 1)[0] == 0
