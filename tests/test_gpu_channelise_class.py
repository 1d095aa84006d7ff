"""-m gpu: the C++ classes DAB_Channeliser and DAB_Stream_Channeliser (dab-radio_amd/host/dab/tx/dab_channeliser.{h,cpp}) through
tests/cpp/channeliser_harness (built by build()), and the Python class's life cycle.  Consecutive calls of odd lengths from a seeked
position equal the host model bit for bit, both directions, complex float and u8; the stream class over ragged block sizes equals one
call over the whole input; a channel list the library refuses surfaces as the class's exception."""
import os
import subprocess

import numpy as np
import pytest

import channelise_model as CM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "channeliser_harness")
D, RATE = 4, 8192000.0


def channels():
    return [CM.channel(CM.freq_q64(-1412000.0, RATE), 1 << 61, 1.0), CM.channel(CM.freq_q64(300000.0, RATE), 0, -0.5), CM.channel(0, 0, 2.0)]


def run(tmp_path, mode, chs, x, *args):
    (tmp_path / "c.bin").write_bytes(b"".join(bytes(CM.to_struct(c)) for c in chs))
    np.ascontiguousarray(x, np.complex64).tofile(tmp_path / "in.c64")
    return subprocess.run([EXE, mode, str(D), str(tmp_path / "c.bin"), str(tmp_path / "in.c64"), str(tmp_path / "out.bin")] + [str(a) for a in args],
                          capture_output=True, text=True, timeout=120)


def signal(seed, n):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def test_split_calls_equal_the_host_model(tmp_path):
    host = CM.build_host_model(tmp_path)
    F = CM.host_design(host, D)
    chs, x = channels(), signal(7600, 5001)
    lengths, seek, start = (513, 7, 600), 12345, -29
    res = run(tmp_path, "split", chs, x, 1, start, seek, *lengths)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.split("\n")
    assert float(lines[0].split()[1]) == pytest.approx(F.error, rel=1e-8) and F.error <= 1e-4
    got = np.fromfile(tmp_path / "out.bin", np.complex64)
    at, off = seek, 0
    for line, n in zip(lines[1:], lengths):
        lo = at * D + start - CM.peak(D)
        assert [int(v) for v in line.split()[1:]] == [lo, (n - 1) * D + CM.taps(D)]
        exp = CM.host_split(host, chs, F, x, at, start, n, True)
        assert np.array_equal(got[off:off + 3 * n].view(np.uint8), exp.reshape(-1).view(np.uint8)), f"call of {n} at {at}"
        at, off = at + n, off + 3 * n
    assert lines[1 + len(lengths)] == f"position {at}" and off == got.size


@pytest.mark.parametrize("scale", [0.0, 25.0], ids=["f32", "u8"])
def test_combine_calls_equal_the_host_model(tmp_path, scale):
    host = CM.build_host_model(tmp_path)
    F = CM.host_design(host, D)
    chs = channels()
    x = np.stack([signal(7700 + c, 1201) for c in range(3)])
    lengths, seek, start = (1029, 7, 2048), 777, 5
    res = run(tmp_path, "combine", chs, x, 1, start, seek, repr(scale), *lengths)
    assert res.returncode == 0, res.stderr
    n = sum(lengths)
    if scale == 0.0:
        got = np.fromfile(tmp_path / "out.bin", np.complex64)
        exp = CM.host_combine(host, chs, 1, F, x, seek, start, n, True)[0]
    else:
        got = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(-1, 2)
        exp = CM.host_combine(host, chs, 1, F, x, seek, start, n, True, CM.U8, scale)[0]
    assert got.shape == exp.shape and np.array_equal(got.view(np.uint8), exp.view(np.uint8))
    assert f"position {seek + n}" in res.stdout


def test_stream_class_over_ragged_blocks_equals_one_call(tmp_path):
    """blocks of 1, 7, 4096 and 65536 samples in turn: every output whose taps are in is delivered, and the whole is one split from sample 0"""
    host = CM.build_host_model(tmp_path)
    F = CM.host_design(host, D)
    chs, x = channels(), signal(7800, 150000)
    res = run(tmp_path, "stream", chs, x, 1, 7, 4096, 65536)
    assert res.returncode == 0, res.stderr
    n = (x.size - CM.taps(D) + CM.peak(D)) // D + 1                          # the outputs whose last tap lies inside the input
    assert f"outputs {n}" in res.stdout
    got = np.fromfile(tmp_path / "out.bin", np.complex64).reshape(3, n)
    exp = CM.host_split(host, chs, F, x, 0, 0, n, False)
    assert np.array_equal(got.view(np.uint8), exp.view(np.uint8))


def test_stream_combiner_over_ragged_blocks_equals_one_call(tmp_path):
    """the other direction: rows fed 1, 7, 4096 and 65536 samples at a time give the wideband samples of one combine over the whole rows"""
    host = CM.build_host_model(tmp_path)
    F = CM.host_design(host, D)
    chs = channels()
    x = np.stack([signal(7850 + c, 40000) for c in range(3)])
    res = run(tmp_path, "cstream", chs, x, 1, 7, 4096, 65536)
    assert res.returncode == 0, res.stderr
    n = x.shape[1] * D - CM.peak(D)                                          # the samples whose latest block sample is in
    assert f"outputs {n}" in res.stdout
    got = np.fromfile(tmp_path / "out.bin", np.complex64)
    exp = CM.host_combine(host, chs, 1, F, x, 0, 0, n, False)[0]
    assert got.shape == exp.shape and np.array_equal(got.view(np.uint8), exp.view(np.uint8))


def test_class_reports_a_refused_channel_list(tmp_path):
    res = run(tmp_path, "split", [CM.channel()] * 9, np.ones(16, np.complex64), 0, 0, 0, 4)
    assert res.returncode == 1 and "DAB_Channeliser" in res.stderr and "9 channels" in res.stderr


def test_python_class_life_cycle():
    """create, plan, both host forms, retune, seek, close twice, use after close; two banks side by side keep their own positions"""
    import dabgpu
    ctx = dabgpu.Context(0)
    chs = [CM.to_struct(c, dabgpu.ChanneliserChannel) for c in channels()]
    a, b = dabgpu.Channeliser(ctx, chs, 1, D), dabgpu.Channeliser(ctx, chs[:1], 1, dabgpu.channeliser_design(D), start=3)
    assert a.decim == b.decim == D and a.plan["taps"] == 288 and a.design.error <= 1e-4 and (a.n_channels, b.n_channels) == (3, 1)
    x = signal(7900, 3000)
    y0 = a.split_host(x, 100, wrap=True)
    y1 = a.split_host(x, 100, wrap=True)                                     # the stream goes on
    z = b.split_host(x, 50, wrap=True)
    a.seek(0)
    whole = a.split_host(x, 200, wrap=True)
    assert np.array_equal(np.concatenate([y0, y1], axis=1).view(np.uint8), whole.view(np.uint8)) and z.shape == (1, 50) and not np.array_equal(z[0], y0[0, :50])
    a.set_params(chs[:2], start=3)
    a.seek(0)
    assert np.array_equal(a.split_host(x, 50, wrap=True)[0].view(np.uint8), z[0].view(np.uint8)) and a.n_channels == 2
    w = a.combine_host(np.stack([x[:500], x[500:1000]]), 300, in_stride_samples=500)
    assert w.shape == (1, 300) and np.isfinite(w).all()
    with pytest.raises(dabgpu.DabGpuError):
        a.set_params(chs + chs[:1])
    a.close(); a.close(); b.close()
    with pytest.raises(dabgpu.DabGpuError):
        a.seek(0)
    ctx.close()
