"""The structured Reed-Solomon words (tests/rs_structured.py) and what the reference's own decoder answered for them
(tests/golden/rs_structured_vectors.npz, written by tests/golden/make_golden_rs_structured.py), on the host: the committed patterns are the
generator's; the records hold the situations the device tests rely on (stated on the reference's records, never on device output); and
dab-radio_amd/csrc/rs_core.h (through tests/cpp/rs_core_host.cpp), the numpy model of packet mode and the C oracle's RS(120,110) path
give the records word for word.  Everything is byte or integer equality."""
import os
import subprocess

import numpy as np
import pytest

import rs_structured as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = (120, 204)


@pytest.fixture(scope="module")
def recorded():
    """code -> dict(patterns, kind, count, positions, fixed)"""
    v = np.load(os.path.join(ROOT, "tests", "golden", "rs_structured_vectors.npz"))
    return {code: dict(patterns=v[f"rs{code}_patterns"], kind=[str(k) for k in v[f"rs{code}_kind"]], count=v[f"rs{code}_count"],
                       positions=v[f"rs{code}_positions"], fixed=v[f"rs{code}_fixed"]) for code in CODES}


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rs_structured") / "rs_core_host"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "dab-radio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "rs_core_host.cpp"), "-o", str(exe)], check=True, timeout=600)
    return str(exe)


@pytest.mark.parametrize("code", CODES)
def test_committed_patterns_are_the_generators(recorded, code):
    pats, kinds = RS.words(code)
    r = recorded[code]
    assert pats.dtype == np.uint8 and pats.shape == r["patterns"].shape and np.array_equal(pats, r["patterns"])
    assert kinds == r["kind"]
    n = len(kinds)
    assert r["count"].shape == (n,) and r["fixed"].shape == (n, code) and r["positions"].shape[0] == n


@pytest.mark.parametrize("code", CODES)
def test_the_records_hold_the_situations(recorded, code):
    c = RS.CODES[code]
    N, K, ROOTS, T, PAD = c["N"], c["K"], c["ROOTS"], c["T"], c["PAD"]
    r = recorded[code]
    fam = [RS.family(k) for k in r["kind"]]
    assert set(fam) == {"single", "exactly_t", "beyond_t", "miscorrect", "padding_root", "degenerate"}
    assert set(int(v) for v in r["count"]) >= set(range(-1, T + 1))
    n_single, seen_m = 0, set()
    for k, (kind, f) in enumerate(zip(r["kind"], fam)):
        pat, cnt, fixed = r["patterns"][k], int(r["count"][k]), r["fixed"][k]
        pos = [int(p) for p in r["positions"][k][:max(cnt, 0)]]
        assert all(int(p) == -1 for p in r["positions"][k][max(cnt, 0):]), kind
        if cnt < 0:
            assert np.array_equal(fixed, pat), (kind, "an uncorrectable word is left as received")
        if f == "single":
            assert cnt == 1 and pos == [PAD + n_single] and not fixed.any(), (kind, k)
            n_single += 1
        elif f == "exactly_t":
            assert cnt == T and sorted(pos) == [PAD + int(p) for p in np.nonzero(pat)[0]] and not fixed.any(), (kind, k)
        elif f == "miscorrect":
            assert cnt == T and fixed.any(), (kind, k)
            assert np.count_nonzero(fixed) == ROOTS + 1 and np.count_nonzero(fixed[:K]) == 1          # the unit message's code word
        elif f == "padding_root":
            m = int(kind.split(":m")[1])
            seen_m.add(m)
            assert cnt == m and sum(p < PAD for p in pos) == 1, (kind, k, cnt, pos)
            assert np.count_nonzero(fixed) == ROOTS and not fixed[:K].any()                            # the padding symbol's parity, whole
        elif kind == "degenerate:two_equal":
            assert cnt == 2 and np.bitwise_xor.reduce(pat) == 0 and not fixed.any()
        elif kind == "degenerate:sigma1_zero":
            assert cnt == 3 and not fixed.any() and RS.locator_of(code, np.nonzero(pat)[0])[1] == 0
        elif kind == "degenerate:two_zero_coefficients":
            assert cnt == T and not fixed.any() and sum(1 for s in RS.locator_of(code, np.nonzero(pat)[0])[1:T] if s == 0) >= 2
        elif kind == "degenerate:weight_1":
            assert cnt == 1 and not fixed.any()
        elif kind == "degenerate:clean":
            assert cnt == 0 and not pat.any() and not fixed.any()
    assert n_single == N and seen_m == set(range(1, T + 1))
    assert sum(k == "degenerate:sigma1_zero" for k in r["kind"]) >= 6
    assert any(k == "degenerate:sigma1_zero" and p[K:].any() for k, p in zip(r["kind"], r["patterns"]))
    assert sum(k == "degenerate:two_equal" for k in r["kind"]) == 3
    assert any(f == "beyond_t" and int(cnt) == -1 for f, cnt in zip(fam, r["count"]))


@pytest.mark.parametrize("code", CODES)
def test_rs_core_equals_the_records_word_for_word(host_exe, recorded, tmp_path, code):
    r = recorded[code]
    n = len(r["kind"])
    (tmp_path / "in.bin").write_bytes(np.ascontiguousarray(r["patterns"], np.uint8).tobytes())
    subprocess.run([host_exe, "decode", str(code), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=60)
    got = np.fromfile(tmp_path / "out.bin", "<i4").reshape(n, 1 + 16 + code)
    for k in range(n):
        c = int(got[k, 0])
        assert c == int(r["count"][k]), (k, r["kind"][k])
        assert got[k, 1:1 + max(c, 0)].tolist() == [int(p) for p in r["positions"][k][:max(c, 0)]], (k, r["kind"][k])
        assert np.array_equal(got[k, 17:], r["fixed"][k]), (k, r["kind"][k])


def test_packet_model_equals_the_records_word_for_word(recorded):
    import packet_fec_model as M
    r = recorded[204]
    for k, pat in enumerate(r["patterns"]):
        c, locs, fixed = M.rs_decode(pat)
        assert c == int(r["count"][k]), (k, r["kind"][k])
        assert locs == [int(p) for p in r["positions"][k][:max(c, 0)]], (k, r["kind"][k])
        assert np.array_equal(np.array(fixed, np.uint8), r["fixed"][k]), (k, r["kind"][k])


def test_c_oracle_rs120_equals_the_records_word_for_word(oracle, recorded):
    r = recorded[120]
    for k, pat in enumerate(r["patterns"]):
        c, fixed, pos = oracle.rs120_decode(pat)
        assert c == int(r["count"][k]), (k, r["kind"][k])
        assert pos.tolist() == [int(p) for p in r["positions"][k][:max(c, 0)]], (k, r["kind"][k])
        assert np.array_equal(fixed, r["fixed"][k]), (k, r["kind"][k])


def test_apply_patterns_helpers():
    """the helpers the device tests build their inputs with: a pattern lands on the symbols of its column / row, nowhere else"""
    import dabplus_model as D
    import packet_fec_model as M
    rng = np.random.Generator(np.random.PCG64(5))
    n_rs = 3
    sf = rng.integers(0, 256, 120 * n_rs).astype(np.uint8)
    pats = rng.integers(0, 256, (n_rs, 120)).astype(np.uint8)
    out = D.apply_patterns(sf, pats)
    for i in range(n_rs):
        assert np.array_equal(out[i::n_rs], sf[i::n_rs] ^ pats[i])
    frame = rng.integers(0, 256, M.RING).astype(np.uint8)
    rows = {0: rng.integers(0, 256, 204).astype(np.uint8), 11: rng.integers(0, 256, 204).astype(np.uint8)}
    out = M.apply_patterns(frame, rows)
    diff = out ^ frame
    for y, p in rows.items():
        assert np.array_equal(diff[M.ROW_OFFSETS[y]], p)
    untouched = np.ones(M.RING, bool)
    untouched[M.ROW_OFFSETS[[0, 11]].reshape(-1)] = False
    assert not diff[untouched].any()
