"""dab-radio_amd/csrc/rs_core.h, the Reed-Solomon arithmetic of the DAB+ and packet-mode kernels, compiled for the host
(tests/cpp/rs_core_host.cpp, its own main) and held to the words recorded from the reference's own decoder for both codes
(tests/golden/dabplus_vectors.npz: RS(120,110); tests/golden/packet_fec_vectors.npz: RS(204,188)): per word the count, the error positions
and the corrected word; the parity map reproduces the parity bytes of every recorded valid code word; and a seeded fuzz of the same driver
built with -fsanitize=address,undefined and run directly."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "cpp", "rs_core_host.cpp")]
INC = ["-I" + os.path.join(ROOT, "dab-radio_amd", "csrc")]


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rs_core_host") / "rs_core_host"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall"] + INC + SRC + ["-o", str(exe)], check=True, timeout=600)
    return str(exe)


@pytest.fixture(scope="module")
def recorded():
    """code -> (received words, the reference's counts, positions, words after correction, kinds)"""
    d = np.load(os.path.join(ROOT, "tests", "golden", "dabplus_vectors.npz"))
    p = np.load(os.path.join(ROOT, "tests", "golden", "packet_fec_vectors.npz"))
    return {120: (d["rs_in"], d["rs_count"], d["rs_positions"], d["rs_out"], None),
            204: (p["rs_words"], p["rs_count"], p["rs_positions"], p["rs_fixed"], [str(k) for k in p["rs_kind"]])}


def run(host_exe, tmp_path, mode, code, rows):
    (tmp_path / "in.bin").write_bytes(np.ascontiguousarray(rows, np.uint8).tobytes())
    subprocess.run([host_exe, mode, str(code), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=60)
    return tmp_path / "out.bin"


@pytest.mark.parametrize("code,n_words,counts_seen", [(120, 440, range(-1, 6)), (204, 296, range(-1, 9))])
def test_decoder_equals_the_reference_word_for_word(host_exe, recorded, tmp_path, code, n_words, counts_seen):
    words, counts, positions, fixed, _ = recorded[code]
    assert words.shape == (n_words, code) and set(int(c) for c in counts) >= set(counts_seen)
    got = np.fromfile(run(host_exe, tmp_path, "decode", code, words), "<i4").reshape(n_words, 1 + 16 + code)
    below = 0
    for k in range(n_words):
        c = int(got[k, 0])
        assert c == int(counts[k]), k
        assert got[k, 1:1 + max(c, 0)].tolist() == [int(p) for p in positions[k][:max(c, 0)]], k
        assert np.array_equal(got[k, 17:], fixed[k]), k
        below += c > 0 and bool((got[k, 1:1 + c] < 255 - code).any())
    if code == 204:
        assert below >= 1, "no word whose reported position lies inside the padding"


def test_parity_map_reproduces_every_recorded_code_word(host_exe, recorded, tmp_path):
    _, counts, _, fixed, _ = recorded[120]
    cw120 = fixed[counts >= 0]
    _, _, _, fixed, kinds = recorded[204]
    cw204 = fixed[[k in [f"errors_{e}" for e in range(9)] for k in kinds]]
    assert cw120.shape == (202, 120) and cw204.shape == (216, 204)
    for code, roots, cws in ((120, 10, cw120), (204, 16, cw204)):
        got = np.fromfile(run(host_exe, tmp_path, "parity", code, cws[:, :code - roots]), np.uint8).reshape(-1, roots)
        assert np.array_equal(got, cws[:, code - roots:]), code


def test_fuzz_program_under_sanitizers(tmp_path):
    exe = tmp_path / "rs_core_host_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] +
                   INC + SRC + ["-o", str(exe)], check=True, timeout=600)
    res = subprocess.run([str(exe), "fuzz", "7700", "3000"], capture_output=True, timeout=600)
    assert res.returncode == 0, res.stderr.decode()[-3000:]
    assert b"fuzz ok" in res.stdout
