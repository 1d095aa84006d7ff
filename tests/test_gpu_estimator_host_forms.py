"""GPU: the single-frame host forms of the per-frame estimators with every combination of their optional arguments
(dabgpu_noise_profile_host_sync, _dd_profile_host_sync, _sym_profile_host_sync, _clock_track_host_sync; _noise_estimate_host_sync once: it
has none).  The Python wrappers always pass every output, so the branches for an output the caller did not ask for run only here.

One frame per call, through the C entry points.  Per form two frames: one the form accepts and one it declares invalid (the skip path has
optional stores of its own).  Every output that is present equals, bit for bit, what the call with every OUTPUT present returned for the
same frame and the same optional inputs (the other tests of each estimator hold that call to the host model); every buffer carries
guard words behind it that stay untouched; state that goes in and out (the profile, the slope) is updated exactly when it is given."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD, MARK = 16, 0xA5C3F00D
NULL, REACH = 2656, 2656 + 2552


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def L():
    import dabgpu
    return dabgpu.lib()


class Buf:
    """n words for the library to write (or, with init, to read and write), GUARD words behind them"""
    def __init__(self, n, init=None):
        self.n = n
        self.a = np.full(n + GUARD, MARK, np.uint32)
        if init is not None:
            self.a[:n] = np.asarray(init).view(np.uint32).reshape(-1)

    @property
    def ptr(self):
        return self.a.ctypes.data

    def words(self):
        assert (self.a[self.n:] == MARK).all(), "guard words written"
        return self.a[:self.n].copy()


def ptr_of(b):
    return None if b is None else b.ptr


def subsets(names):
    return [frozenset(c) for r in range(len(names) + 1) for c in itertools.combinations(names, r)]


@pytest.fixture(scope="module")
def null_frames():
    """[accepted, invalid]: noise, a louder symbol behind the NULL; the invalid one has a NaN inside the NULL window"""
    rng = np.random.default_rng(9900)
    n = 700 + REACH + 1600
    x = (0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    a = 700 + NULL + 8
    x[a:] += (4.0 * (rng.standard_normal(n - a) + 1j * rng.standard_normal(n - a))).astype(np.complex64)
    bad = x.copy()
    bad[700 + 608 + 1000] = np.nan
    return [x, bad]


@pytest.fixture(scope="module")
def product_frames():
    """[accepted, one symbol of NaN products, all zero]: unit steps at an amplitude per carrier under noise"""
    rng = np.random.default_rng(9901)
    c = np.arange(1536)
    amp = (2.0e5 * (1.0 + 0.5 * np.cos(2 * np.pi * c / 311.0))).astype(F32)
    step = np.exp(1j * np.pi * (rng.integers(0, 4, (75, 1536)) * 0.5 + 0.25))
    z = rng.standard_normal((75, 1536)) + 1j * rng.standard_normal((75, 1536))
    d = (amp[None, :] * step + amp.mean() * 0.1 * z).astype(np.complex64)
    nan = d.copy()
    nan[10] = complex(np.nan, 1.0)
    return [d, nan, np.zeros_like(d)]


def check_all(form, call, outputs, inputs, frames):
    """call(frame, present) -> {name: words} of the arguments that were present.  For every frame and every choice of the optional inputs:
    the call with every output present is the reference (valid 1 for frames[0], 0 for the others), every subset of the outputs equals it"""
    n_calls = 0
    for i, frame in enumerate(frames):
        for ins in subsets(inputs):
            ref = call(frame, ins | frozenset(outputs))
            assert int(ref["valid"][0]) == (1 if i == 0 else 0), (form, i, sorted(ins))
            for outs in subsets(outputs):
                got = call(frame, ins | outs)
                n_calls += 1
                assert set(got) == set(ins | outs), (form, sorted(got))
                for name in outs | (ins & frozenset(outputs + ["profile", "slope"])):
                    assert got[name].tobytes() == ref[name].tobytes(), (form, i, sorted(ins), sorted(outs), name)
    return n_calls


def test_noise_profile_every_subset(ctx, L, null_frames):
    rng = np.random.default_rng(9902)
    exclude = rng.integers(0, 1 << 32, 48, dtype=np.uint64).astype(np.uint32) & np.uint32(0x11111111)
    state = (0.02 * (1.0 + rng.random(128))).astype(F32)

    def call(x, present):
        b = dict(exclude=Buf(48, exclude), profile=Buf(128, state), band_weight=Buf(128), mean_noise=Buf(1), carrier_power=Buf(1536), valid=Buf(1))
        b = {k: v for k, v in b.items() if k in present}
        st = L.dabgpu_noise_profile_host_sync(ctx._h, x.ctypes.data, x.size, 700, 1.0e-4, 3, ptr_of(b.get("exclude")), ptr_of(b.get("profile")), 0.25,
                                              ptr_of(b.get("band_weight")), ptr_of(b.get("mean_noise")), ptr_of(b.get("carrier_power")),
                                              ptr_of(b.get("valid")))
        assert st == 0, L.dabgpu_last_error()
        out = {k: v.words() for k, v in b.items()}
        if "exclude" in out:
            assert np.array_equal(out["exclude"], exclude)                                  # an input only
        return out

    # the profile is input and output at once: with it the band values are smoothed against it (and it comes back updated, or as it
    # went in for a frame that is skipped), without it they are the frame's own and no profile is returned
    outputs = ["band_weight", "mean_noise", "carrier_power", "valid"]
    assert check_all("noise_profile", call, outputs, ["exclude", "profile"], null_frames) == 2 * 64
    ok, bad = (call(x, frozenset(["profile", "valid", "band_weight"])) for x in null_frames)
    assert not np.array_equal(ok["profile"], state.view(np.uint32)) and np.array_equal(bad["profile"], state.view(np.uint32))
    assert not bad["band_weight"].any() and ok["band_weight"].all()
    assert not np.array_equal(call(null_frames[0], frozenset(["band_weight"]))["band_weight"], ok["band_weight"])       # the state matters


def test_dd_profile_every_subset(ctx, L, product_frames):
    rng = np.random.default_rng(9903)
    exclude = rng.integers(0, 1 << 32, 48, dtype=np.uint64).astype(np.uint32) & np.uint32(0x01010101)
    state = (1.2e-38 * (1.0 + 0.25 * rng.random(128))).astype(F32)      # so small that a frame without noise of its own decays it below the usable range

    def call(d, present):
        b = dict(exclude=Buf(48, exclude), profile=Buf(128, state), band_weight=Buf(128), mean_noise=Buf(1), carrier_noise=Buf(1536),
                 carrier_amplitude=Buf(1536), valid=Buf(1))
        b = {k: v for k, v in b.items() if k in present}
        st = L.dabgpu_dd_profile_host_sync(ctx._h, d.ctypes.data, ptr_of(b.get("exclude")), ptr_of(b.get("profile")), 0.25, ptr_of(b.get("band_weight")),
                                           ptr_of(b.get("mean_noise")), ptr_of(b.get("carrier_noise")), ptr_of(b.get("carrier_amplitude")),
                                           ptr_of(b.get("valid")))
        assert st == 0, L.dabgpu_last_error()
        out = {k: v.words() for k, v in b.items()}
        if "exclude" in out:
            assert np.array_equal(out["exclude"], exclude)
        return out

    outputs = ["band_weight", "mean_noise", "carrier_noise", "carrier_amplitude", "valid"]
    assert check_all("dd_profile", call, outputs, ["exclude", "profile"], product_frames[:2]) == 2 * 128
    ok, bad = (call(d, frozenset(["profile", "valid", "carrier_noise"])) for d in product_frames[:2])
    assert not np.array_equal(ok["profile"], state.view(np.uint32)) and np.array_equal(bad["profile"], state.view(np.uint32))
    assert not bad["carrier_noise"].any() and ok["carrier_noise"].any()


def test_sym_profile_every_subset(ctx, L, product_frames):
    def call(d, present):
        b = {k: Buf(n) for k, n in (("symbol_weight", 75), ("symbol_noise", 75), ("ref_noise", 1), ("valid", 1)) if k in present}
        st = L.dabgpu_sym_profile_host_sync(ctx._h, d.ctypes.data, ptr_of(b.get("symbol_weight")), ptr_of(b.get("symbol_noise")),
                                            ptr_of(b.get("ref_noise")), ptr_of(b.get("valid")))
        assert st == 0, L.dabgpu_last_error()
        return {k: v.words() for k, v in b.items()}

    outputs = ["symbol_weight", "symbol_noise", "ref_noise", "valid"]
    assert check_all("sym_profile", call, outputs, [], [product_frames[0], product_frames[2]]) == 2 * 16
    assert call(product_frames[0], frozenset(outputs))["symbol_weight"].all() and not call(product_frames[2], frozenset(outputs))["symbol_weight"].any()


def test_clock_track_every_subset(ctx, L, product_frames):
    slope_in = np.array([123456789012345], np.int64)

    def call(d, present):
        b = {k: Buf(n) for k, n in (("dqpsk_out", 75 * 1536 * 2), ("corr", 2), ("valid", 1)) if k in present}
        slope = Buf(2, slope_in)
        st = L.dabgpu_clock_track_host_sync(ctx._h, d.ctypes.data, ptr_of(b.get("dqpsk_out")), slope.ptr, 0.5, ptr_of(b.get("corr")), ptr_of(b.get("valid")))
        assert st == 0, L.dabgpu_last_error()
        return dict({k: v.words() for k, v in b.items()}, slope=slope.words())

    outputs = ["dqpsk_out", "corr", "valid"]
    n = 0
    for i, d in enumerate([product_frames[0], product_frames[2]]):
        ref = call(d, frozenset(outputs))
        assert int(ref["valid"][0]) == 1 - i
        assert (ref["slope"].view(np.int64)[0] == slope_in[0]) == (i == 1)                   # a skipped frame keeps the slope as it came
        for outs in subsets(outputs):
            got = call(d, outs)
            n += 1
            assert set(got) == set(outs) | {"slope"}
            for name in got:
                assert got[name].tobytes() == ref[name].tobytes(), (i, sorted(outs), name)
    assert n == 2 * 8


def test_noise_estimate_once(ctx, L, null_frames):
    import dabgpu
    for i, x in enumerate(null_frames):
        rec = Buf(5)
        assert L.dabgpu_noise_estimate_host_sync(ctx._h, x.ctypes.data, x.size, 700, 1.0e-4, 3, rec.ptr) == 0, L.dabgpu_last_error()
        got = rec.words()
        want = ctx.noise_estimate_host(x, 700, freq_offset=1.0e-4, fine_time_offset=3)
        assert got.tobytes() == np.asarray(want).tobytes() and int(got[4]) == 1 - i and np.dtype(dabgpu.NOISE_RECORD_DTYPE).itemsize == 20
        assert bool(got[:4].any()) == (i == 0)
