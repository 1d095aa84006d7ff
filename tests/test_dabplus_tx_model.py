"""CPU: the DAB+ super-frame encoder's numpy model (tests/dabplus_tx_model.py, written from TS 102 563 with its own arithmetic) against the
oracle's pieces, against the receivers -- the oracle's AacFrameProcessor and, where oracle/_ref was built, the reference's own
AAC_Frame_Processor --, against the committed vectors, and the library's device-free layout function (dabgpu_dabplus_superframe_layout)
against the model's."""
import ctypes as C
import os

import numpy as np
import pytest

import dabplus_tx_model as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESCRIPTORS = (0x13, 0x3A, 0x51, 0x6F)                   # 4, 2, 6, 3 access units: 3, 1, 5, 2 header fields
SIZES = (24, 48, 72, 792, 1536)


@pytest.fixture(scope="module")
def dabgpu():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "dab-radio_amd", "libdabgpu.so")):
        g.build()
    import dabgpu
    return dabgpu


@pytest.fixture(scope="module")
def vectors():
    return np.load(os.path.join(ROOT, "tests", "golden", "dabplus_tx_vectors.npz"))


def sweep():
    """(frame bytes, descriptor, unit lengths): every size x unit count, random / one big unit / empty units"""
    rng = np.random.default_rng(7)
    for n in SIZES:
        for d in DESCRIPTORS:
            yield n, d, T.split_lengths(rng, d, n)
            yield n, d, T.split_lengths(rng, d, n, "zeros")
            if 110 * (n // 24) <= 4095:
                yield n, d, T.split_lengths(rng, d, n, "first_big")


def test_parity_and_fire_code_equal_the_oracles(oracle):
    rng = np.random.default_rng(3)
    for k in range(200):
        data = rng.integers(0, 256, 110, dtype=np.uint8)
        if k % 7 == 0:
            data[rng.integers(0, 110, 60)] = 0
        assert np.array_equal(T.rs_parity(data), oracle.rs120_encode(data)), k
        nine = rng.integers(0, 256, 9, dtype=np.uint8)
        assert T.firecode(nine) == oracle.firecode_crc(nine), k
    assert T.firecode(np.zeros(9, np.uint8)) == 0 and T.au_crc([]) == 0


def test_the_oracle_receiver_hands_the_units_back(oracle):
    rng = np.random.default_rng(4)
    for n, d, lens in sweep():
        aus = [rng.integers(0, 256, l, dtype=np.uint8) for l in lens]
        frames, status = T.encode(d, aus, n)
        assert status == 0, (n, d, lens)
        p = oracle.AacFrameProcessor()
        for j in range(5):
            rc, r, sf = p.process(frames[j * n:(j + 1) * n])
        na = T.num_aus_of(d)
        assert r["superframe_done"] and r["firecode_ok"] and r["rs_corrected"] == 0 and r["rs_failed_index"] == -1 and r["header_valid"], (n, d, lens)
        assert int(r["num_aus"]) == na and int(r["au_crc_ok_mask"]) == (1 << na) - 1 and int(r["au_walk_stopped_at"]) == -1, (n, d, lens)
        start = T.layout(n, d, lens)[1]
        assert list(r["au_start"][:na + 1]) == start[:na + 1]
        for a in range(na):
            assert np.array_equal(sf[start[a]:start[a] + lens[a]], aus[a]), (n, d, a)


def test_the_reference_receiver_hands_the_units_back(oracle):
    R = oracle.ref()
    if R is None or not hasattr(R, "ref_aac_create"):
        pytest.skip("oracle/_ref not built (the reference's sources are not here)")
    rng = np.random.default_rng(5)
    for n, d, lens in sweep():
        aus = [rng.integers(0, 256, l, dtype=np.uint8) for l in lens]
        frames, status = T.encode(d, aus, n)
        h = C.c_void_p(R.ref_aac_create())
        for j in range(5):
            fr = np.ascontiguousarray(frames[j * n:(j + 1) * n])
            ev = np.zeros(12, np.int32); al = np.zeros(6, np.int32); ab = np.zeros((6, 8192), np.uint8)
            R.ref_aac_process(h, fr.ctypes.data, n, ev.ctypes.data, al.ctypes.data, ab.ctypes.data, 8192)
        R.ref_aac_destroy(h)
        na = T.num_aus_of(d)
        assert ev[0] == 0 and ev[1] == -1 and ev[2] == 1 and ev[8] == na and int(np.uint32(ev[9])) == (1 << na) - 1 and ev[10] == 0, (n, d, lens, ev)
        for a in range(na):
            assert al[a] == lens[a] and np.array_equal(ab[a][:al[a]], aus[a]), (n, d, a)


def test_committed_vectors_are_the_models_and_carry_the_references_verdict(vectors):
    names = [str(s) for s in vectors["names"]]
    assert len(names) >= 40 and set(np.unique(vectors["status"])) == {0, 1, 2, 3}
    for i, name in enumerate(names):
        n, d, lens = int(vectors["frame_bytes"][i]), int(vectors["descriptor"][i]), vectors["au_len"][i]
        na = T.num_aus_of(d)
        blob, aus, off = vectors[f"au_{i}"], [], 0
        for a in range(na):
            aus.append(blob[off:off + int(lens[a])]); off += int(lens[a])
        frames, status = T.encode(d, aus, n)
        assert status == int(vectors["status"][i]) and np.array_equal(frames, vectors[f"frames_{i}"]), name
        ev = vectors["ref_events"][i]
        if status == 0:
            assert vectors["has_ref"][i] and ev[0] == 0 and ev[1] == -1 and ev[2] == 1 and ev[8] == na and int(np.uint32(ev[9])) == (1 << na) - 1, name
        elif vectors["has_ref"][i]:
            assert ev[2] == 1 and ev[9] == 0 and not frames.any(), name          # zero frames: a header, no unit


def test_layout_function_equals_the_model(dabgpu, vectors):
    cases = [(n, d, lens) for n, d, lens in sweep()]
    cases += [(int(vectors["frame_bytes"][i]), int(vectors["descriptor"][i]), [int(v) for v in vectors["au_len"][i]]) for i in range(len(vectors["names"]))]
    for n, d, lens in cases:
        st, start, na, n_rs = dabgpu.DabPlusTx.layout(n, d, lens)
        est, estart, ena, enrs = T.layout(n, d, list(lens) + [0] * 6)
        assert (st, na, n_rs) == (est, ena, enrs), (n, d, lens)
        if st == 0:
            assert list(start) == estart, (n, d, lens)


def test_layout_function_refusals(dabgpu):
    lay = dabgpu.DabPlusTx.layout
    for n in (0, 23, 25, 1560):
        assert lay(n, 0x00, [10, 10, 10, 10])[0] == 1
    # 96-byte frames, three units: 440 data bytes = 6 header + 3 x 2 CRC + 428 payload
    assert lay(96, 0x60, [100, 200, 128])[0] == 0
    assert lay(96, 0x60, [100, 200, 127])[0] == 2 and lay(96, 0x60, [100, 200, 129])[0] == 2
    # 1536-byte frames, two units: the second starts at 5 + len + 2
    room = 110 * 64 - 5 - 4
    st, start, na, n_rs = lay(1536, 0x20, [4095 - 7, room - (4095 - 7)])
    assert st == 0 and na == 2 and n_rs == 64 and list(start[:3]) == [5, 4095, 7040]
    assert lay(1536, 0x20, [4096 - 7, room - (4096 - 7)])[0] == 3
    # a length of 0xFFFF is refused, not wrapped
    assert lay(1536, 0x40, [0xFFFF] * 6)[0] == 2
    assert lay(24, 0x40, [0, 0, 0, 0, 0, 110 - 11 - 12])[0] == 0


def test_entry_points_refuse_bad_arguments_without_a_device(dabgpu):
    L = dabgpu.lib()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    assert L.dabgpu_dabplus_tx_encode(None, 1, 1, p, p, p, p, p, p, p, 24, p, None) == 2
    assert L.dabgpu_dabplus_tx_encode_host_sync(None, 1, p, p, p, p, 24, p, p) == 2
    assert b"null context" in L.dabgpu_last_error()
