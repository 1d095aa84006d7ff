"""GPU: the three single-frame host forms of receive diversity (dabgpu_diversity_combine_host_sync, _banded_host_sync,
_symbols_host_sync) and the three device entry points behind them, called through the C entry points themselves -- the Python wrapper
always passes both out scalars, so the branches for a scalar the caller did not ask for run only here.

Per form: every subset of the optional arguments h_weight, h_valid, h_soft_scale, h_live_mask; per-branch table patterns (a band table, a
symbol table, both, neither, turned through the branches) over 1, 3 and 8 branches; a dead branch given as a null products pointer (by its
scale, by its flag, and alone: an erased frame); both layouts; a table array that is null and one whose entries all are.  Bits, scale and
mask equal the compiled rule (diversity_symbols_model.host_combine_frame) byte for byte; h_bits, h_soft_scale and h_live_mask carry guard
words before and behind them that stay untouched.  Per device entry point: 1 and 3 frames, the default frame stride and a wider one,
runs of 1 and 75 symbols and the planner's choice, against the same rule."""
import ctypes as C
import itertools

import numpy as np
import pytest

import diversity_model as DM
import diversity_symbols_model as M

pytestmark = pytest.mark.gpu

F32 = np.float32
NB = DM.NB_FRAME_BITS
GUARD, MARK = 16, 0xA5C3F00D
FORMS = ["dabgpu_diversity_combine_host_sync", "dabgpu_diversity_combine_banded_host_sync", "dabgpu_diversity_combine_symbols_host_sync"]
CALLS = ["dabgpu_diversity_combine_frames", "dabgpu_diversity_combine_frames_banded", "dabgpu_diversity_combine_frames_symbols"]
KINDS = ("b", "s", "bs", "-")
N_FRAMES = 3


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


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return M.build_host_model(tmp_path_factory.mktemp("diversity_host_forms_model"))


@pytest.fixture(scope="module")
def data():
    """eight branches x three frames: products, scales, scalar weights, band tables over two decades, symbol tables in (0, 1]"""
    rng = np.random.default_rng(9950)
    shape = (8, N_FRAMES, 75, 1536)
    dq = ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.exp(rng.uniform(-1, 1, (8, N_FRAMES, 1, 1)))).astype(np.complex64)
    k = (40 * np.exp(rng.uniform(-1, 1, (8, N_FRAMES)))).astype(F32)
    w = np.exp(rng.uniform(-2, 2, (8, N_FRAMES))).astype(F32)
    band = np.exp(rng.uniform(-2.3, 2.3, (8, N_FRAMES, 128))).astype(F32)
    sym = np.minimum(1.0, np.exp(rng.uniform(-3.0, 3.0, (8, N_FRAMES, 75)))).astype(F32)
    for a in (dq, k, w, band, sym):
        a.setflags(write=False)
    return dict(dq=dq, k=k, w=w, band=band, sym=sym)


class Guarded:
    """n_bytes for the library to write, GUARD marked words before and behind them"""
    def __init__(self, n_bytes):
        self.n = n_bytes
        self.a = np.full(2 * GUARD + (n_bytes + 3) // 4, MARK, np.uint32)

    @property
    def ptr(self):
        return self.a.ctypes.data + 4 * GUARD

    def bytes(self):
        b = self.a.view(np.uint8)
        assert (self.a[:GUARD] == MARK).all() and (b[4 * GUARD + self.n:].view(np.uint32) == MARK).all(), "guard words written"
        return b[4 * GUARD:4 * GUARD + self.n].copy()


def pointers(rows):
    """(the array of addresses, what keeps them alive) of a list of arrays / None; None for no array at all"""
    if rows is None:
        return None, None
    keep = [None if x is None else np.ascontiguousarray(x) for x in rows]
    return (C.c_void_p * len(keep))(*[None if x is None else x.ctypes.data for x in keep]), keep


def host_form(L, ctx, form, dq, k, w, valid, band, sym, layout, want_scale=True, want_mask=True):
    """one call of FORMS[form]; band / sym: a list with an entry or None per branch, or None for a null array (the scalar form takes
    neither, the banded form no sym) -> (bits, scale or None, mask or None)"""
    n = len(dq)
    ptrs, keep = pointers(dq)
    k = np.ascontiguousarray(k, F32)
    w = None if w is None else np.ascontiguousarray(w, F32)
    v = None if valid is None else np.ascontiguousarray(valid, np.int32)
    bits, out_k, out_m = Guarded(NB), Guarded(4), Guarded(4)
    p = lambda x: None if x is None else x.ctypes.data
    args = [ctx._h, ptrs, p(k), p(w), p(v), n, layout, bits.ptr, out_k.ptr if want_scale else None, out_m.ptr if want_mask else None]
    tables = [pointers(band), pointers(sym)][:form]
    st = getattr(L, FORMS[form])(*args, *[t[0] for t in tables])
    assert st == 0, L.dabgpu_last_error()
    gk, gm = out_k.bytes().view(F32)[0], out_m.bytes().view(np.uint32)[0]
    assert want_scale or gk.view(np.uint32) == MARK
    assert want_mask or gm == MARK
    return bits.bytes().view(np.int8), gk if want_scale else None, int(gm) if want_mask else None


def check_form(L, ctx, host, form, dq, k, w, valid, band, sym, layout, want_scale=True, want_mask=True):
    band, sym = (band if form >= 1 else None), (sym if form >= 2 else None)
    bits, gk, gm = host_form(L, ctx, form, dq, k, w, valid, band, sym, layout, want_scale, want_mask)
    eb, ek, em = M.host_combine_frame(host, dq, k, w, valid, band, sym, layout)
    what = (FORMS[form], len(dq), layout, w is not None, valid is not None, want_scale, want_mask)
    assert np.array_equal(bits, eb), what
    assert gk is None or gk.view(np.uint32) == ek.view(np.uint32), what
    assert gm is None or gm == em, what
    return eb, ek, em


def tables_of(data, n, shift, frame=0):
    """branch b: KINDS[(b + shift) % 4] -- a band table, a symbol table, both, neither"""
    kinds = [KINDS[(b + shift) % 4] for b in range(n)]
    return ([data["band"][b][frame] if "b" in kinds[b] else None for b in range(n)],
            [data["sym"][b][frame] if "s" in kinds[b] else None for b in range(n)])


@pytest.mark.parametrize("form", [0, 1, 2])
def test_every_subset_of_the_optional_arguments(ctx, L, host, data, form):
    n = 3
    dq, k = [data["dq"][b][0] for b in range(n)], data["k"][:n, 0] * F32(n)
    names = ["weight", "valid", "scale", "mask"]
    subsets = [frozenset(c) for r in range(5) for c in itertools.combinations(names, r)]
    assert len(subsets) == 16
    seen = set()
    for i, s in enumerate(subsets):
        band, sym = tables_of(data, n, i % 4)
        w = data["w"][:n, 0] if "weight" in s else None
        valid = [1, 0, 1] if "valid" in s else None                      # branch 1 dead by its flag, its products present
        eb, ek, em = check_form(L, ctx, host, form, dq, k, w, valid, band, sym, (i // 4 + i) % 2, "scale" in s, "mask" in s)
        assert em == (5 if valid else 7) and ek > 0 and len(np.unique(eb)) > 200
        seen.add(eb.tobytes())
    assert len(seen) >= 4                                                # weights and flags reach the bits


@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 3, 8])
def test_table_patterns_over_the_branches(ctx, L, host, data, n, form):
    dq, k = [data["dq"][b][1] for b in range(n)], data["k"][:n, 1] * F32(n)
    for shift in range(4):
        band, sym = tables_of(data, n, shift, 1)
        w = data["w"][:n, 1] if shift % 2 else None
        _, ek, em = check_form(L, ctx, host, form, dq, k, w, None, band, sym, (shift // 2) % 2)
        assert em == (1 << n) - 1 and ek > 0


@pytest.mark.parametrize("form", [0, 1, 2])
def test_dead_branches_without_products_and_null_arrays(ctx, L, host, data, form):
    n = 3
    band, sym = tables_of(data, n, 0, 2)                                   # b, s, bs
    for layout in (0, 1):
        # dead by its scale, no flags at all; dead by its flag; the only branch, dead: an erased frame
        dq, k = [data["dq"][0][2], data["dq"][1][2], None], data["k"][:n, 2].copy()
        k[2] = 0.0
        assert check_form(L, ctx, host, form, dq, k, None, None, band, sym, layout)[2] == 3
        dq = [None, data["dq"][1][2], data["dq"][2][2]]
        assert check_form(L, ctx, host, form, dq, data["k"][:n, 2], data["w"][:n, 2], [0, 1, 1], band, sym, layout)[2] == 6
        eb, ek, em = check_form(L, ctx, host, form, [None], [0.0], None, None, band[:1], sym[:1], layout)
        assert not eb.any() and ek == 0 and em == 0
        # a null array is the narrower form, an array of null entries computes the same
        dq = [data["dq"][b][2] for b in range(n)]
        ref = check_form(L, ctx, host, 0, dq, data["k"][:n, 2], data["w"][:n, 2], None, None, None, layout)
        for b_arr, s_arr in ((None, None), ([None] * n, None), (None, [None] * n), ([None] * n, [None] * n)):
            got = check_form(L, ctx, host, form, dq, data["k"][:n, 2], data["w"][:n, 2], None, b_arr, s_arr, layout)
            assert np.array_equal(got[0], ref[0]) and got[1:] == ref[1:]
        if form == 2:
            only = check_form(L, ctx, host, form, dq, data["k"][:n, 2], None, None, None, sym, layout)            # no band array at all
            assert not np.array_equal(only[0], ref[0])


def to_dev(a):
    import torch
    return torch.from_numpy(np.array(a).view(np.uint8).reshape(-1)).cuda()              # (a copy: the fixtures are read-only)


@pytest.mark.parametrize("call", [0, 1, 2])
@pytest.mark.parametrize("frames", [1, 3])
def test_device_entry_points(ctx, L, host, data, frames, call):
    """three branches: a band table (banded and symbols call), a scalar weight and a symbol table (symbols call), sync records of which
    one refuses frame 0.  Strides 0 and 230400 + 16, runs of the planner's choice, 1 and 75 symbols, both layouts"""
    import dabgpu
    import torch
    n = 3
    valid = np.ones(frames, np.int32)
    valid[0] = 0
    rec = np.zeros(frames, np.dtype(dabgpu.SYNC_STATE_DTYPE))
    rec["sync_valid"] = valid
    h = dict(dq=[data["dq"][b][:frames] for b in range(n)], k=data["k"][:n, :frames] * F32(n),
             band=[data["band"][0][:frames] if call >= 1 else None, None, None], sym=[None, data["sym"][1][:frames] if call >= 2 else None, None],
             w=[None, data["w"][1][:frames], None])
    d = {name: [None if x is None else to_dev(x) for x in h[name]] for name in ("dq", "k", "band", "sym", "w")}
    d_sync = to_dev(rec)
    table = dabgpu.diversity_table([(d["dq"][b], d["k"][b], d["w"][b], d_sync if b == 2 else None) for b in range(n)])
    tables = [dabgpu.band_weight_table(d["band"], n), dabgpu.band_weight_table(d["sym"], n, "symbol_weights")][:call]
    exp = {}
    for layout in (0, 1):
        rows = [M.host_combine_frame(host, [x[f] for x in h["dq"]], h["k"][:, f], [F32(1), h["w"][1][f], F32(1)], [1, 1, valid[f]],
                                     [None if x is None else x[f] for x in h["band"]] if call >= 1 else None,
                                     [None if x is None else x[f] for x in h["sym"]] if call >= 2 else None, layout) for f in range(frames)]
        exp[layout] = (np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], F32), np.array([r[2] for r in rows], np.uint32))
        assert exp[layout][2].tolist() == [3, 7, 7][:frames] and (exp[layout][1] > 0).all()
    i = 0
    for stride in (0, NB + 16):
        for spb in (0, 1, 75):
            layout = i % 2
            i += 1
            step = stride or NB
            bits = torch.full((frames * step + 64,), 55, dtype=torch.int8, device="cuda")
            scale = torch.full((frames + 2,), -1.0, dtype=torch.float32, device="cuda")
            mask = torch.full((frames + 2,), -1, dtype=torch.int32, device="cuda")
            st = getattr(L, CALLS[call])(ctx._h, table, n, frames, bits.data_ptr(), stride, layout, spb, scale[1:].data_ptr(), mask[1:].data_ptr(), *tables,
                                         ctx._stream(None))
            assert st == 0, L.dabgpu_last_error()
            torch.cuda.synchronize()
            got, gk, gm = bits.cpu().numpy(), scale.cpu().numpy(), mask.cpu().numpy()
            body = got[:frames * step].reshape(frames, step)
            what = (CALLS[call], frames, stride, spb, layout)
            assert np.array_equal(body[:, :NB], exp[layout][0]), what
            assert (body[:, NB:] == 55).all() and (got[frames * step:] == 55).all(), what
            assert np.array_equal(gk[1:-1].view(np.uint32), exp[layout][1].view(np.uint32)) and gk[0] == -1.0 and gk[-1] == -1.0, what
            assert np.array_equal(gm[1:-1].view(np.uint32), exp[layout][2]) and gm[0] == -1 and gm[-1] == -1, what
