"""-m gpu: dabgpu_ber_frames_layout / dabgpu_ber_ring_layout equal the numpy model (tests/ber_model.py) record for record.  The inputs
need no decoder: random int8 rings with 0, +-127 and -128 among the values and random "decoded" bytes.
Configuration A, 3 ensembles: the shortest EEP sub-channels (4 CU at 4-A, 6 CU at 3-A) at odd start addresses (their class rows are only
4-byte aligned), an EEP-B sub-channel, a four-segment UEP row whose code word is shorter than its capacity units (row 4: 2236 bits in
35 CU), two sub-channels sharing a schedule, a sub-channel ending at CU 864.  Configuration B, 1 ensemble: the 864-CU EEP 4-A
sub-channel, the longest code word (6912 bytes of LDS).  Both layouts, history 5 and 8 with the newest slot at the wrap, the ring form
with ensembles at different slots and one negative slot, FIC only, MSC only, NULL record pointers, and a captured graph replayed on
changed inputs against plain calls."""
import numpy as np
import pytest

import ber_model as M
import tx_encode_cases as T
from ber_cases import Case, as_records, records

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


def test_result_dtype_is_the_models():
    import dabgpu
    assert np.dtype(dabgpu.BER_RESULT_DTYPE) == M.BER_DTYPE


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("name,H,newest", [("A", 5, 0), ("A", 5, 2), ("A", 8, 0), ("A", 8, 7), ("B", 5, 1), ("B", 8, 3)])
def test_frames_equal_the_model(oracle, ctx, name, H, newest, layout):
    import dabgpu
    import torch
    c = Case.get(oracle, name, H)
    ring, fib, msc, gsubs = c.device(dabgpu, torch, layout)
    fic_r, msc_r = records(torch, c.n_ens, 4), records(torch, c.n_ens, 4, len(gsubs))
    ctx.ber_frames(ring, c.n_ens, H * M.FRAME_BITS, H, newest, gsubs, fib, msc, 4 * c.nb, fic_r, msc_r, bits_layout=layout)
    torch.cuda.synchronize()
    exp_fic, exp_msc = c.model([newest] * c.n_ens)
    got_fic, got_msc = as_records(fic_r), as_records(msc_r)
    assert np.array_equal(got_fic, exp_fic), (got_fic, exp_fic)
    bad = np.argwhere(got_msc != exp_msc)
    assert bad.size == 0, (bad[:4], got_msc[tuple(bad[0])], exp_msc[tuple(bad[0])])
    assert (exp_msc["n_errors"] > 0).all() and (exp_msc["n_bits"] > 0).all()


@pytest.mark.parametrize("layout", [0, 1])
def test_ring_form_with_ensembles_at_different_slots_and_one_negative(oracle, ctx, layout):
    import dabgpu
    import torch
    H = 5
    c = Case.get(oracle, "A", H)
    ring, fib, msc, gsubs = c.device(dabgpu, torch, layout)
    slots = [4, -1, 1]
    d_slots = torch.tensor(slots, dtype=torch.int32, device="cuda")
    fic_r, msc_r = records(torch, c.n_ens, 4), records(torch, c.n_ens, 4, len(gsubs))
    ctx.ber_ring(ring, c.n_ens, H * M.FRAME_BITS, H, d_slots, gsubs, fib, msc, 4 * c.nb, fic_r, msc_r, bits_layout=layout)
    torch.cuda.synchronize()
    exp_fic, exp_msc = c.model(slots)
    assert np.array_equal(as_records(fic_r), exp_fic) and np.array_equal(as_records(msc_r), exp_msc)
    assert not as_records(fic_r)[1].view(np.uint32).any() and not as_records(msc_r)[1].view(np.uint32).any()        # all-zero records


@pytest.mark.parametrize("layout", [0, 1])
def test_halves_and_null_pointers(oracle, ctx, layout):
    import dabgpu
    import torch
    H, newest = 5, 0
    c = Case.get(oracle, "A", H)
    ring, fib, msc, gsubs = c.device(dabgpu, torch, layout)
    exp_fic, exp_msc = c.model([newest] * c.n_ens)
    untouched = np.full(16, 0xA5, np.uint8).view(M.BER_DTYPE)[0]
    args = (ring, c.n_ens, H * M.FRAME_BITS, H, newest)
    # FIC only: no sub-channels at all; and the MSC pair NULL
    for subs, m_bytes in (([], None), (gsubs, None)):
        fic_r, msc_r = records(torch, c.n_ens, 4), records(torch, c.n_ens, 4, len(gsubs))
        ctx.ber_frames(*args, subs, fib, m_bytes, 4 * c.nb, fic_r, None, bits_layout=layout)
        torch.cuda.synchronize()
        assert np.array_equal(as_records(fic_r), exp_fic)
        assert (as_records(msc_r) == untouched).all()
    # MSC only
    fic_r, msc_r = records(torch, c.n_ens, 4), records(torch, c.n_ens, 4, len(gsubs))
    ctx.ber_frames(*args, gsubs, None, msc, 4 * c.nb, None, msc_r, bits_layout=layout)
    torch.cuda.synchronize()
    assert np.array_equal(as_records(msc_r), exp_msc) and (as_records(fic_r) == untouched).all()
    # a NULL record pointer skips its half although the bytes are given
    fic_r, msc_r = records(torch, c.n_ens, 4), records(torch, c.n_ens, 4, len(gsubs))
    ctx.ber_frames(*args, gsubs, fib, msc, 4 * c.nb, None, msc_r, bits_layout=layout)
    ctx.ber_frames(*args, gsubs, fib, msc, 4 * c.nb, None, None, bits_layout=layout)          # nothing to do: no launch, no error
    torch.cuda.synchronize()
    assert np.array_equal(as_records(msc_r), exp_msc) and (as_records(fic_r) == untouched).all()
    fic_r, msc_r = records(torch, c.n_ens, 4), records(torch, c.n_ens, 4, len(gsubs))
    ctx.ber_frames(*args, gsubs, fib, msc, 4 * c.nb, fic_r, None, bits_layout=layout)
    torch.cuda.synchronize()
    assert np.array_equal(as_records(fic_r), exp_fic) and (as_records(msc_r) == untouched).all()


def test_refusals_reach_the_caller(oracle, ctx):
    import dabgpu
    import torch
    H = 5
    c = Case.get(oracle, "A", H)
    ring, fib, msc, gsubs = c.device(dabgpu, torch, 0)
    fic_r, msc_r = records(torch, c.n_ens, 4), records(torch, c.n_ens, 4, len(gsubs))
    with pytest.raises(dabgpu.DabGpuError, match="newest_frame_slot"):
        ctx.ber_frames(ring, c.n_ens, H * M.FRAME_BITS, H, H, gsubs, fib, msc, 4 * c.nb, fic_r, msc_r)
    with pytest.raises(dabgpu.DabGpuError, match="history_frames"):
        ctx.ber_frames(ring, c.n_ens, H * M.FRAME_BITS, 4, 0, gsubs, fib, msc, 4 * c.nb, fic_r, msc_r)
    with pytest.raises(dabgpu.DabGpuError, match="aligned"):
        ctx.ber_frames(ring.data_ptr() + 4, 1, H * M.FRAME_BITS, H, 0, gsubs, fib, msc, 4 * c.nb, fic_r, msc_r)
    torch.cuda.synchronize()
    assert (as_records(fic_r).view(np.uint32) == 0xA5A5A5A5).all()


def test_single_code_word_host_forms(oracle, ctx):
    import dabgpu
    c = Case.get(oracle, "A", 5)
    got = ctx.ber_fib_group(c.ring[0, 2, 2304:4608], c.fib[0, 1])
    assert tuple(got) == M.record(c.ring[0, 2, 2304:4608], M.fic_codeword(oracle, c.fib[0, 1]))
    off = 0
    for d, sc in zip(c.dicts, c.osubs):
        nb = oracle.subchannel_plan(sc)[2]
        K = M.kept_bits(oracle, sc)
        bits = c.ring[1, 3, 5000:5000 + 64 * sc.length]
        got = ctx.ber_codeword(T.g_sub(dabgpu, d), bits, c.msc[1, 2, off:off + nb])
        assert tuple(got) == M.record(bits[:K], M.msc_codeword(oracle, sc, c.msc[1, 2, off:off + nb])), d
        off += nb


@pytest.mark.parametrize("layout", [0, 1])
def test_one_captured_graph_replayed_on_changed_inputs_equals_plain_calls(oracle, ctx, layout):
    import dabgpu
    import torch
    H, newest = 8, 7
    c = Case.get(oracle, "A", H)
    other = Case.get(oracle, "A", H, seed=8101)
    ring, fib, msc, gsubs = c.device(dabgpu, torch, layout)
    ring2, fib2, msc2, _ = other.device(dabgpu, torch, layout)
    fic_r, msc_r = records(torch, c.n_ens, 4), records(torch, c.n_ens, 4, len(gsubs))
    side = torch.cuda.Stream()

    def call():
        ctx.ber_frames(ring, c.n_ens, H * M.FRAME_BITS, H, newest, gsubs, fib, msc, 4 * c.nb, fic_r, msc_r, bits_layout=layout)

    with torch.cuda.stream(side):
        call()                                                   # the first call with this multiplex on this stream uploads its tables
    torch.cuda.synchronize()
    plain = []
    for src in ((ring, fib, msc), (ring2, fib2, msc2)):
        with torch.cuda.stream(side):
            if src[0] is not ring:
                ring.copy_(src[0]); fib.copy_(src[1]); msc.copy_(src[2])
            call()
        torch.cuda.synchronize()
        plain.append((as_records(fic_r).copy(), as_records(msc_r).copy()))
    exp = [c.model([newest] * c.n_ens), other.model([newest] * c.n_ens)]
    for (gf, gm), (ef, em) in zip(plain, exp):
        assert np.array_equal(gf, ef) and np.array_equal(gm, em)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        call()
    torch.cuda.synchronize()
    for k, src in enumerate((c, other)):
        r, f, m, _ = src.device(dabgpu, torch, layout)
        ring.copy_(r); fib.copy_(f); msc.copy_(m)
        fic_r.fill_(0xA5); msc_r.fill_(0xA5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(as_records(fic_r), plain[k][0]) and np.array_equal(as_records(msc_r), plain[k][1]), k
