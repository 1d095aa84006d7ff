"""-m gpu: the C++ classes DAB_IQ_Balancer and DAB_Stream_IQ_Balancer (dab-radio_amd/host/ofdm/dab_iq_balancer.{h,cpp}) through
tests/cpp/iqbal_class_harness (built by build()), block by block over odd block lengths: the output, flush included, and the final
record do not depend on the block lengths and equal the host model walked chunk by chunk, bit for bit, primed and in one pass; a parameter
set the library refuses surfaces as the class's exception."""
import os
import subprocess

import numpy as np
import pytest

import iqbal_model as IM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "iqbal_class_harness")
N = 7013
CHUNK = 2048


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    d = tmp_path_factory.mktemp("iqbal_class")
    rng = np.random.default_rng(7600)
    x = (rng.standard_normal(N) + 1j * rng.standard_normal(N)) / np.sqrt(2.0)
    x = IM.impair(x, 0.42, 3.0, 0.3 + 0.2j).astype(np.complex64)
    x[5000] = np.nan                                                          # tile 4 is skipped
    x.tofile(d / "in.c64")
    return d, IM.build_host_model(d), x


def run(d, P, lengths, prime, out="out.bin", chunk=CHUNK):
    (d / "p.bin").write_bytes(bytes(IM.to_struct(P)))
    return subprocess.run([EXE, str(d / "p.bin"), str(d / "in.c64"), str(d / out), str(d / (out + ".state")), str(chunk), str(int(prime))] +
                          [str(n) for n in lengths], capture_output=True, text=True, timeout=120)


def expected(host, P, x, prime):
    """the class's definition restated on the host model: chunks of CHUNK from sample 0 on, the rest at the flush"""
    rec = IM.host_records(host, 1)
    out, pos = [], 0
    while pos < N:
        n = min(CHUNK, N - pos)
        tiles = n // IM.TILE * IM.TILE
        seg = x[pos:pos + n]
        if prime:
            if tiles:
                IM.host_apply(host, [P], rec, seg, pos, tiles, IM.MEASURE)
            out.append(IM.host_apply(host, [P], rec, seg, pos, n, IM.APPLY)[0][0])
        elif n == CHUNK:
            out.append(IM.host_apply(host, [P], rec, seg, pos, n, IM.MEASURE | IM.APPLY)[0][0])
        else:
            if tiles:
                out.append(IM.host_apply(host, [P], rec, seg, pos, tiles, IM.MEASURE | IM.APPLY)[0][0])
            if n > tiles:
                out.append(IM.host_apply(host, [P], rec, seg[tiles:], pos + tiles, n - tiles, IM.APPLY)[0][0])
        pos += n
    return np.concatenate(out), rec


def same_but_nan(got, want):
    got, want = (np.ascontiguousarray(v).view(np.float32) for v in (got, want))
    nan = np.isnan(want)
    return bool(np.all(np.isnan(got[nan]))) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


@pytest.mark.parametrize("prime", [True, False], ids=["primed", "one_pass"])
@pytest.mark.parametrize("P", [IM.params(min_weight=1024.0, forget=1.0), IM.params(min_weight=2048.0, forget=0.9),
                               IM.params(mode=IM.FIXED, a=1.02 - 0.03j, b=-0.02 - 0.03j, c=0.25j), IM.params(mode=IM.OFF)],
                         ids=["track", "track_forget", "fixed", "off"])
def test_stream_class_equals_the_model_whatever_the_blocks(setup, P, prime):
    d, host, x = setup
    exp, rec = expected(host, P, x, prime)
    for k, lengths in enumerate(((N,), (1029, 7, 2041, 3936), (1, 31, 1, 800, 1, 1024, 1023, 4132), (3000, 0, 4013))):
        assert sum(lengths) == N
        res = run(d, P, lengths, prime, out=f"out{k}.bin")
        assert res.returncode == 0, res.stderr
        got = np.fromfile(d / f"out{k}.bin", np.complex64)
        assert got.size == N and same_but_nan(got, exp), f"blocks {lengths}"
        state = np.fromfile(d / f"out{k}.bin.state", IM.RECORD_DTYPE)
        assert state.tobytes() == rec.tobytes(), f"blocks {lengths}"
        w = abs(complex(rec["w_re"][0], rec["w_im"][0]))
        want_db = "inf" if w == 0 else f"{-20 * np.log10(w):.2f}"
        assert res.stdout.strip() == f"iq chunks={N // CHUNK} rejection_db={want_db}", f"blocks {lengths}"
    if P["mode"] == IM.TRACK:
        assert rec["valid"][0] == 1 and rec["tiles_skipped"][0] == 1 and rec["tiles_used"][0] == 5
        if prime:                                                             # the first chunk is corrected already: the image is down
            K1, K2 = IM.front_end(0.42, 3.0)
            assert abs(complex(rec["w_re"][0], rec["w_im"][0]) - K2 / np.conj(K1)) < 0.05


def test_class_reports_a_refused_parameter_set(setup):
    d, _, _ = setup
    res = run(d, IM.params(forget=1.5), (4,), True)
    assert res.returncode == 1 and "DAB_IQ_Balancer" in res.stderr and "forget 1.5" in res.stderr
