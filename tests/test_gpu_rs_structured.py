"""-m gpu: the structured Reed-Solomon words (tests/rs_structured.py) through both kernels that correct on the device, held to what the
REFERENCE's decoder recorded for them (tests/golden/rs_structured_vectors.npz) -- the cases that random damage never produces: a root in
every lane's share of the Chien search and on every seam between two shares, a root inside the padding (counted, not applied), a
miscorrection into another code word, locators with zero inner coefficients, S_0 = 0, received symbols that are 0, and the first failing
code word of a super frame at either end with correctable ones around it.

DAB+ (dabplus.hip, RS(120,110)): one stream per frame size through dabgpu.DabPlusBank.process, for n_rs = 1, 2, 3, 5, 8, 32, 33, 63, 64 code
words per super frame (lane-share and Horner syndromes, 64 down to 1 lanes per code word in the search).  Every super frame is valid random
code words in the interleaved columns XOR patterns, checked (a) against oracle.AacFrameProcessor and (b) from the fixture alone.
Packet mode (packet_fec.hip, RS(204,188)): FEC frames with patterns on their rows through dabgpu.PacketBank, 24- and 96-byte logical frames;
rs_count per row against the reference's recorded count, and packets, records and counts against the numpy model.
Byte and integer equality throughout."""
import os

import numpy as np
import pytest

import dabplus_model as D
import packet_fec_model as M
import rs_structured as RS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = {"single", "exactly_t", "beyond_t", "miscorrect", "padding_root", "degenerate", "recorded"}
DAB_SIZES = [24, 48, 72, 120, 192, 768, 792, 1512, 1536]         # n_rs = 1, 2, 3, 5, 8, 32, 33, 63, 64


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name))


class Word:
    """an error pattern and what the reference's decoder recorded for it"""

    def __init__(self, pattern, count, fixed, kind, base="random"):
        self.pattern, self.count, self.fixed, self.kind, self.base = pattern, int(count), fixed, kind, base
        self.family = RS.family(kind)


def words_of(code):
    """the structured words of `code` and the words recorded earlier (received words, used as patterns: the code is linear)"""
    v = golden("rs_structured_vectors.npz")
    out = [Word(p, c, f, str(k)) for p, c, f, k in zip(v[f"rs{code}_patterns"], v[f"rs{code}_count"], v[f"rs{code}_fixed"], v[f"rs{code}_kind"])]
    if code == 120:
        d = golden("dabplus_vectors.npz")
        assert d["rs_in"].shape == (440, 120)
        out += [Word(p, c, f, "recorded") for p, c, f in zip(d["rs_in"], d["rs_count"], d["rs_out"])]
    else:
        d = golden("packet_fec_vectors.npz")
        assert d["rs_words"].shape == (296, 204)
        out += [Word(p, c, f, "recorded") for p, c, f in zip(d["rs_words"], d["rs_count"], d["rs_fixed"])]
    return out


def pick(words, kind):
    return next(w for w in words if w.kind == kind)


# ------------------------------------------------------------------------------------------------------------------------------------------
# DAB+
# ------------------------------------------------------------------------------------------------------------------------------------------
def dab_plan(n_rs):
    """-> list of super frames, each a list of n_rs Words.  All correctable words first, n_rs to a super frame (nothing hides them); then every
    uncorrectable word as the FIRST failing column of a super frame of its own, at column 0, n_rs - 1, n_rs / 2, k mod n_rs in turn, with
    correctable words in all other columns; then first failing column 0, n_rs - 1, and both; then the two super frames with received zeros"""
    words = words_of(120)
    good = [w for w in words if w.count >= 0]
    bad = [w for w in words if w.count < 0]
    clean = pick(words, "degenerate:clean")
    plan = []
    for a in range(0, len(good), n_rs):
        chunk = good[a:a + n_rs]
        plan.append(chunk + [clean] * (n_rs - len(chunk)))
    at = 0

    def filler(k):
        nonlocal at
        out = [good[(at + i) % len(good)] for i in range(k)]
        at += k
        return out
    for k, w in enumerate(bad):
        col = (0, n_rs - 1, n_rs // 2, k % n_rs)[k % 4]
        sf = filler(n_rs)
        sf[col] = w
        plan.append(sf)
    beyond = [w for w in bad if w.family == "beyond_t"]
    for cols in ((0,), (n_rs - 1,), (0, n_rs - 1)):
        sf = filler(n_rs)
        for c in cols:
            sf[c] = beyond[c % len(beyond)]
        plan.append(sf)
    # received symbols that are 0: one error alone on the zero code word in an all-zero super frame (its fire code bytes are zero as well), and
    # two errors whose value is the symbol underneath
    col = min(2, n_rs - 1)
    w1, w2 = pick(words, "degenerate:weight_1"), [w for w in words if w.kind == "degenerate:two_equal"][1]
    sf = [Word(clean.pattern, 0, clean.fixed, clean.kind, "zero") for _ in range(n_rs)]
    sf[col] = Word(w1.pattern, w1.count, w1.fixed, w1.kind, "zero")
    plan.append(sf)
    sf = filler(n_rs)
    sf[col] = Word(w2.pattern, w2.count, w2.fixed, w2.kind, "equal")
    plan.append(sf)
    return plan


def dab_superframe(firecode_crc, rng, cols):
    """-> (received super frame, expected super frame, rs_failed_index, rs_corrected) from the fixture's records alone.  Data bytes 0 and 1
    of the code words underneath are chosen so that the RECEIVED bytes 0..1 are the fire code of received bytes 2..10: acquisition passes"""
    n_rs = len(cols)
    data = rng.integers(0, 256, (n_rs, 110)).astype(np.uint8)
    pat = np.stack([w.pattern for w in cols])
    for i, w in enumerate(cols):
        if w.base == "zero":
            data[i] = 0
        elif w.base == "equal":
            rows = np.nonzero(w.pattern)[0]
            assert rows.max() < 110
            data[i, rows] = w.pattern[rows]
    head = [(b % n_rs, b // n_rs) for b in range(11)]
    fc = firecode_crc(np.array([data[i, j] ^ pat[i, j] for i, j in head[2:]], np.uint8))
    for (i, j), v in zip(head[:2], (fc >> 8, fc & 0xFF)):
        data[i, j] = v ^ pat[i, j]
    cw = RS.encode(120, data)
    valid = np.ascontiguousarray(cw.T).reshape(-1)
    received = D.apply_patterns(valid, pat)
    counts = [w.count for w in cols]
    first = next((i for i, c in enumerate(counts) if c < 0), -1)
    upto = n_rs if first < 0 else first
    exp = cw ^ pat                                                    # from the first failing column on: the received bytes
    for i in range(upto):
        exp[i] = cw[i] ^ pat[i] ^ (pat[i] ^ cols[i].fixed)
    for i, w in enumerate(cols):
        rows = np.nonzero(w.pattern)[0]
        if w.base == "zero":
            assert np.array_equal(cw[i] ^ pat[i], w.pattern), "nothing but the errors: every other received symbol is 0"
        elif w.base == "equal":
            assert rows.size and not (cw[i] ^ pat[i])[rows].any(), "the received symbols under the errors are 0"
    return received, np.ascontiguousarray(exp.T).reshape(-1), first, int(sum(counts[:upto]))


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("n", DAB_SIZES)
def test_dabplus_structured_words(ctx, oracle, n):
    import dabgpu
    import torch
    from test_gpu_dabplus import same_record
    n_rs = n // 24
    rng = np.random.default_rng(8800 + n)
    plan = dab_plan(n_rs)
    built = [dab_superframe(oracle.firecode_crc, rng, cols) for cols in plan]
    # from the expected side: what this launch shows of every family and count, and where its super frames fail first
    shown, firsts = set(), set()
    for cols, (_, _, first, _) in zip(plan, built):
        firsts.add(first)
        for w in cols[:n_rs if first < 0 else first + 1]:
            shown.add((w.family, w.count))
    assert {f for f, _ in shown} == FAMILIES and {c for _, c in shown} == set(range(-1, 6)), shown
    assert {tuple(i for i, w in enumerate(cols) if w.count < 0) for cols in plan} >= {(0,), (n_rs - 1,), tuple(sorted({0, n_rs - 1}))}
    assert firsts >= {-1, 0, n_rs - 1}
    # every position once as a single error, in super frames where nothing fails
    assert {int(np.nonzero(w.pattern)[0][0]) for cols, b in zip(plan, built) if b[2] < 0 for w in cols if w.kind == "single"} == set(range(120))
    n_sf = len(plan)
    F = 5 * n_sf
    frames = np.stack([b[0] for b in built]).reshape(F, n)
    rec_dt = np.dtype(dabgpu.SUPERFRAME_RESULT_DTYPE)
    bank = dabgpu.DabPlusBank(ctx, 1)
    d_frames = torch.from_numpy(frames).cuda()
    d_off = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
    d_sf = torch.full((1, n_sf, 5 * n), 0xC3, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros((1, n_sf, rec_dt.itemsize), dtype=torch.uint8, device="cuda")
    d_cnt = torch.full((1, 4), -9, dtype=torch.int32, device="cuda")
    bank.process(d_frames, d_off, n, d_n, F, d_sf, 5 * n, d_res, n_sf, d_cnt)
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(rec_dt).reshape(n_sf)
    sfs, cnt = d_sf.cpu().numpy()[0], d_cnt.cpu().numpy()[0]
    bank.close()
    assert cnt[0] == n_sf and cnt[1] == 0, cnt                        # every first frame passed the fire code: a super frame every 5 frames
    proc = oracle.AacFrameProcessor()
    k = 0
    for f in range(F):
        _, o, sf_o = proc.process(frames[f])
        assert not o["firecode_wait_failed"] and bool(o["superframe_done"]) == (f % 5 == 4), f
        if not o["superframe_done"]:
            continue
        g, (_, exp_sf, first, corrected) = res[k], built[k]
        tag = (n, k, [w.kind for w in plan[k]][:8], first)
        # (b) from the fixture, without the oracle
        assert int(g["rs_failed_index"]) == first, tag
        assert int(g["rs_corrected"]) == corrected, tag
        assert np.array_equal(sfs[k], exp_sf), (tag, np.nonzero(sfs[k] != exp_sf)[0][:8] % n_rs)
        # (a) the oracle's record and bytes
        ok, field = same_record(g, o)
        assert ok, (tag, field, g, o)
        assert int(g["frame_index"]) == f and np.array_equal(sfs[k], sf_o), tag
        k += 1
    assert k == n_sf


# ------------------------------------------------------------------------------------------------------------------------------------------
# packet mode
# ------------------------------------------------------------------------------------------------------------------------------------------
class WalkOnly(M.Processor):
    """the model's packet walk without its row decoder: which FEC frames reach the correction at all (that does not depend on the rows)"""

    def _correct(self):
        self.fec_frames.append((len(self.log), [0] * M.ROWS))


def fec_ends(fb, n):
    """logical frame in which FEC frame k of a stream ends -> k"""
    return {((k + 1) * M.RING - 1) // fb: k for k in range(n)}


def logical(frames, fb, n_frames=None):
    """FEC frames -> logical frames [n][fb], zero bytes behind (24-byte packets of address 0)"""
    s = np.concatenate(frames)
    n = -(-s.size // fb) if n_frames is None else n_frames
    flat = np.zeros(n * fb, np.uint8)
    flat[:s.size] = s
    return flat.reshape(n, fb)


def packet_fec_frames(seed, fb):
    """-> (FEC frames, per frame its 12 Words or None).  FEC frames of 24-byte packets (a damaged length field then keeps the walk on the
    24-byte grid) with 12 patterns each, row 0 -- byte 0 of every packet -- included.  Where the model's walk does not reach the correction
    (a pattern on row 0 sent it astray), the frame's patterns are fed again on rows 1..11 of further frames"""
    rng = np.random.default_rng(seed)
    words = words_of(204)
    t_random = pick(words, "exactly_t:random")
    t_parity = pick(words, "exactly_t:parity")
    two_equal = [w for w in words if w.kind == "degenerate:two_equal"][1]
    rows_of = []
    order = list(rng.permutation(len(words))) if fb == 96 else list(range(len(words)))       # other rows and neighbours in the second stream
    # a packet whose length field grows no longer fits its logical frame and is lost, and the frame with it: row 0 takes the words that
    # leave bits 6..7 of byte 0 of every packet (its even data symbols) alone, while there are any
    keeps = [i for i in order if not (words[i].pattern[0:M.RS_K:2] & 0xC0).any()]
    rest = [i for i in order if (words[i].pattern[0:M.RS_K:2] & 0xC0).any()]
    while keeps or rest:
        row0 = [(keeps or rest).pop(0)]
        others = []
        while len(others) < 11 and (rest or keeps):
            others.append((rest or keeps).pop(0))
        rows_of.append([words[i] for i in row0 + others] + [None] * (11 - len(others)))
    rows_of.append([t_random] * 12)                                    # one t-error pattern on all 12 rows: all rows fill their slots at once
    rows_of.append([t_parity] * 12)
    for w in [w for w in words if w.family in ("miscorrect", "padding_root")][:6]:             # row 0 alone: the packet headers
        rows_of.append([w] + [None] * 11)
    rows_of.append([None] * 5 + [Word(two_equal.pattern, two_equal.count, two_equal.fixed, two_equal.kind, "equal")] + [None] * 6)

    def fec_frame(rows):
        f, _ = M.random_fec_frame(rng, (24,))
        for y, w in enumerate(rows):
            if w is not None and w.base == "equal":                    # the symbols under the errors are the error values: received as 0
                xs = np.nonzero(w.pattern)[0]
                assert xs.max() < M.RS_K
                f[M.ROW_OFFSETS[y, xs]] = w.pattern[xs]
                f[M.APP:] = M.fec_packets(f[:M.APP])
        out = M.apply_patterns(f, [None if w is None else w.pattern for w in rows])
        for y, w in enumerate(rows):
            if w is not None and w.base == "equal":
                assert not out[M.ROW_OFFSETS[y, np.nonzero(w.pattern)[0]]].any()
        return out
    frames = [fec_frame(r) for r in rows_of]
    walk = M.run_frames(list(logical(frames, fb)), WalkOnly())
    ends = fec_ends(fb, len(frames))
    done = {ends[e["frame_index"]] for e in walk["fec_frames"]}
    again = [w for k, r in enumerate(rows_of) if k not in done for w in r if w is not None]
    for a in range(0, len(again), 11):
        chunk = again[a:a + 11]
        rows_of.append([None] + chunk + [None] * (11 - len(chunk)))
        frames.append(fec_frame(rows_of[-1]))
    return frames, rows_of


@pytest.fixture(scope="module")
def packet_case():
    """the streams of one launch -- the FEC frames with 24-byte logical frames dealt to four streams, those with 96-byte logical frames in a
    fifth, which is about as long -- as (frame bytes, logical frames, {FEC frame the model corrects: its 12 Words}, what the model reports
    for the call); shared, not modified"""
    specs = []
    frames, rows_of = packet_fec_frames(8924, 24)
    per = -(-len(frames) // 4)
    for a in range(0, len(frames), per):
        specs.append((24, frames[a:a + per], rows_of[a:a + per]))
    specs.append((96,) + packet_fec_frames(8996, 96))
    n_frames = max(-(-len(frames) * M.RING // fb) for fb, frames, _ in specs)
    out = []
    for fb, frames, rows_of in specs:
        stream = logical(frames, fb, n_frames)
        exp = M.run_frames(list(stream))
        ends = fec_ends(fb, len(frames))
        rows = {ends[e["frame_index"]]: rows_of[ends[e["frame_index"]]] for e in exp["fec_frames"]}
        stream.setflags(write=False)
        out.append((fb, stream, rows, exp))
    return out


def test_packet_structured_words(ctx, packet_case):
    import dabgpu
    from test_gpu_packet_fec import Call, same
    # from the expected side: the model's counts are the reference's records, and for either size of logical frame every word, every family
    # and every count is in a frame that was corrected
    for size in (24, 96):
        shown, ids, all_rows = set(), set(), []
        for fb, stream, rows, exp in packet_case:
            if fb != size:
                continue
            ends = fec_ends(fb, len(exp["fec_frames"]) + 64)
            for e in exp["fec_frames"]:
                r = rows[ends[e["frame_index"]]]
                assert e["rs_count"] == [0 if w is None else w.count for w in r], (fb, e["frame_index"])
                shown |= {(w.family, w.count) for w in r if w is not None}
                ids |= {id(w) for w in r if w is not None and w.base == "random"}
                all_rows.append(r)
        assert {f for f, _ in shown} == FAMILIES and {c for _, c in shown} == set(range(-1, 9)), shown
        assert len(ids) == len(words_of(204)) == 280 + 296
        assert any(all(w is not None and w.kind.startswith("exactly_t") for w in r) and len({id(w) for w in r}) == 1 for r in all_rows)
        assert any(r[0] is not None and all(w is None for w in r[1:]) for r in all_rows)
        assert any(w is not None and w.base == "equal" for r in all_rows for w in r)
    streams = [c[1] for c in packet_case]
    bank = dabgpu.PacketBank(ctx, len(streams))
    call = Call(streams)
    call.run(bank)
    got = call.fetch()
    bank.close()
    for s, ((fb, _, rows, exp), g) in enumerate(zip(packet_case, got)):
        ends = fec_ends(fb, len(rows) + 64)
        seen = {}
        for rec in g["fec_frames"][:g["counts"][2]]:
            seen[ends[int(rec["frame_index"])]] = rec["rs_count"].tolist()
        assert sorted(seen) == sorted(rows), (s, fb)
        for k, r in rows.items():                                      # the reference's recorded count per row
            assert seen[k] == [0 if w is None else w.count for w in r], (s, fb, k, [None if w is None else w.kind for w in r])
        same(g, exp, ("structured", s, fb))                            # packets, records, counts: the model's
