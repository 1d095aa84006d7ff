"""-m gpu: the frame-history ring at the 32-bit edge.  The lane and octet Viterbi mappings keep ring offsets in 32 bits on purpose and
the host sends rings that do not fit to the wave mapping (tests/test_addressing_rules.py holds the rule).  Here the largest ring the
lanes still take (18641 frames, its end 80 896 bytes below 2^32) and the first they must refuse (18642 frames) are decoded on the
device: one ensemble, only the five frames a decode of one frame reads are ever written, everything else of the 4 GiB is untouched.

Expected bytes and path errors come from the oracle (Deinterleaver + msc_decode_logical over the same CIFs), whatever mapping the
planner ends up with; the same five frames in a compact 5-frame ring are a second, independent reading.  The BER call reads the same
ring against tests/ber_model.py, the generic batch reads it through ring-form code words, and the writers (history demodulator,
diversity combiner) put a frame into the top slot of the large ring, with canaries around it and 2^32 bytes below it."""
import numpy as np
import pytest

import ber_model as BM
import big_buffers as BB

pytestmark = pytest.mark.gpu

NB = 230400
SIZES = [18641, 18642]
MAPPINGS = {"auto": 0, "wave": 1, "lane": 2, "octet": 3}


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.viterbi_set_mapping(0)
    c.close()


def noisy(oracle, bits01, rng, gain=0.5, sigma=24.0):
    s = oracle.soft_from_bits(bits01).astype(np.float32) * gain + rng.standard_normal(len(bits01)) * sigma
    return np.clip(np.rint(s), -127, 127).astype(np.int8)


def results_np(t):
    import dabgpu
    return t.cpu().numpy().view(np.dtype(dabgpu.RESULT_DTYPE)).reshape(-1)


@pytest.fixture(scope="module")
def truth(oracle):
    """five frames (20 CIFs) of a three-sub-channel multiplex, and what the oracle makes of the newest frame's four CIFs"""
    import dabgpu
    rng = np.random.default_rng(4242)
    # EEP 3-A of 6 CU at an odd start address (short; its class rows are only 4-byte aligned), UEP index 4 (four segments, padding),
    # EEP 4-A that ends at capacity unit 864: the last bytes of a CIF row, and with them the highest offsets, are read
    subs = [oracle.subchannel(3, 6, eep_level=2, eep_type=0), oracle.subchannel(100, 35, is_uep=True, uep_index=4),
            oracle.subchannel(800, 64, eep_level=3, eep_type=0)]
    gsubs = [dabgpu.SubChannel(s.start_address, s.length, s.is_uep, s.uep_prot_index, s.eep_prot_level, s.eep_type) for s in subs]
    plans = [oracle.subchannel_plan(s) for s in subs]
    n_cif = 20
    cifs = rng.integers(-127, 128, (n_cif, oracle.NB_CIF_BITS), dtype=np.int8)
    for s, p in zip(subs, plans):
        lf = np.stack([oracle.msc_encode_logical(s, rng.integers(0, 256, p[2], dtype=np.uint8)) for _ in range(n_cif)])
        tx = oracle.time_interleave(lf)
        for t in range(n_cif):
            cifs[t, s.start_address * 64:(s.start_address + s.length) * 64] = noisy(oracle, tx[t], rng)
    frames = np.zeros((5, NB), np.int8)
    frames[:, 9216:] = cifs.reshape(5, -1)
    fib = np.zeros((4, 96), np.uint8)
    for f in range(5):
        for g in range(4):
            frames[f, 2304 * g:2304 * (g + 1)] = noisy(oracle, oracle.fic_encode_group(rng.integers(0, 256, 90, dtype=np.uint8)), rng, sigma=30.0)
    for g in range(4):
        fib[g] = oracle.fic_decode_group(frames[4, 2304 * g:2304 * (g + 1)], 0)[0]
    cif_out = sum(p[2] for p in plans)
    out = np.zeros((4, cif_out), np.uint8)
    res = np.zeros((4, len(subs)), np.dtype(dabgpu.RESULT_DTYPE))
    off = 0
    for si, (s, p) in enumerate(zip(subs, plans)):
        d = oracle.Deinterleaver(s.length * 8)
        got = []
        for t in range(n_cif):
            d.consume(cifs[t, s.start_address * 64:(s.start_address + s.length) * 64])
            lfr = d.deinterleave()
            if lfr is not None:
                got.append(oracle.msc_decode_logical(s, lfr, 0))
        assert len(got) == n_cif - 15
        for c in range(4):
            eb, ee = got[len(got) - 4 + c]
            out[c, off:off + p[2]] = eb
            res[c, si]["path_error"], res[c, si]["n_out_bytes"] = ee, p[2]
        off += p[2]
    assert (res["path_error"] > 0).all(), "the noise must leave every code word a path error to compare"
    ber_fic, ber_msc = BM.ber_frames(oracle, frames, 4, subs, fib, out)
    return dict(subs=subs, gsubs=gsubs, plans=plans, frames=frames, classed=BM.to_classed(frames), out=out, res=res, cif_out=cif_out, fib=fib,
                ber_fic=ber_fic, ber_msc=ber_msc)


def slots_of(H, newest):
    """ring slots of the five frames, oldest first"""
    return [(newest - 4 + j) % H for j in range(5)]


def fill_ring(view, H, newest, frames):
    for j, slot in enumerate(slots_of(H, newest)):
        BB.put(view, slot * NB, frames[j])


CASES = [(H, newest, layout) for H in SIZES + [5] for newest in ("top", "wrap") for layout in (0, 1)]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"H{c[0]}-{c[1]}-{'classed' if c[2] else 'natural'}")
def ring(request, truth):
    """the ring of one case on the device; newest = H - 1, or 1: the five frames then wrap from the top of the ring to its bottom, so
    one code word reads offsets near 2^32 and near 0.  H = 5 is the compact second reading (no lead, plain allocation)."""
    import torch
    H, where, layout = request.param
    newest = H - 1 if where == "top" else 1
    view = BB.big(H * NB) if H > 5 else torch.empty(H * NB, dtype=torch.uint8, device="cuda")
    if H > 5:
        # what a read 2^32 bytes too low would see: erasures, not whatever an earlier allocation left there
        BB.region(view, -BB.CANARY_BYTES * 64, BB.CANARY_BYTES * 64).zero_()
    fill_ring(view, H, newest, truth["classed"] if layout else truth["frames"])
    torch.cuda.synchronize()
    yield dict(view=view, H=H, newest=newest, layout=layout)
    del view
    BB.release()


def check_decoded(truth, d_out, d_res, what):
    out, res = d_out.cpu().numpy().reshape(4, -1), results_np(d_res).reshape(4, -1)
    assert np.array_equal(out, truth["out"]), what
    assert np.array_equal(res["path_error"], truth["res"]["path_error"]), what
    assert np.array_equal(res["n_out_bytes"], truth["res"]["n_out_bytes"]), what


@pytest.mark.parametrize("mapping", list(MAPPINGS))
@pytest.mark.parametrize("form", ["frames", "ring"])
def test_msc_decode_reads_the_ring_at_the_edge(ctx, truth, ring, mapping, form):
    import torch
    n_sub, cif_out = len(truth["gsubs"]), truth["cif_out"]
    d_out = torch.full((4, cif_out), 0xC3, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros((4 * n_sub, 16), dtype=torch.uint8, device="cuda")
    ctx.viterbi_set_mapping(MAPPINGS[mapping])
    try:
        if form == "ring":
            d_slots = torch.tensor([ring["newest"]], dtype=torch.int32, device="cuda")
            ctx.msc_decode_ring(ring["view"], 1, ring["H"] * NB, ring["H"], d_slots, truth["gsubs"], d_out, 4 * cif_out, d_res, bits_layout=ring["layout"])
        else:
            ctx.msc_decode_frames(ring["view"], 1, ring["H"] * NB, ring["H"], ring["newest"], truth["gsubs"], d_out, 4 * cif_out, d_res,
                                  bits_layout=ring["layout"])
        torch.cuda.synchronize()
    finally:
        ctx.viterbi_set_mapping(0)
    check_decoded(truth, d_out, d_res, (ring["H"], ring["newest"], ring["layout"], mapping, form))


@pytest.mark.parametrize("mapping", ["lane", "octet", "wave"])
def test_generic_batch_reads_the_ring_through_ring_form_code_words(ctx, truth, ring, mapping):
    """viterbi_decode_batch, one batch per sub-channel (one schedule each): four ring-form code words, the CIFs of the newest frame.
    The large ring must go to the wave mapping whatever is forced, the others may stay with the lanes: the oracle's bytes either way."""
    import dabgpu
    import torch
    H, newest, layout = ring["H"], ring["newest"], ring["layout"]
    base = ring["view"].data_ptr()
    ctx.viterbi_set_mapping(MAPPINGS[mapping])
    try:
        off = 0
        for si, (g, p) in enumerate(zip(truth["gsubs"], truth["plans"])):
            pi, lx, nb = dabgpu.subchannel_plan(g)
            d_o = torch.full((4, nb), 0xC3, dtype=torch.uint8, device="cuda")
            d_res = torch.zeros((4, 16), dtype=torch.uint8, device="cuda")
            cws = []
            for c in range(4):
                cw = dabgpu.Codeword()
                cw.d_src = base + 9216 + g.start_address * (4 if layout else 64)
                cw.d_out = d_o[c].data_ptr()
                for k in range(len(lx)):
                    cw.seg_pi[k], cw.seg_steps[k] = (pi[k], 32 * lx[k]) if lx[k] else (0, 0)
                cw.n_steps = 32 * sum(lx) + 6
                cw.n_slots, cw.newest_slot, cw.cifs_per_frame, cw.frame_stride, cw.cif_stride = 4 * H, 4 * newest + c, 4, NB, 55296
                cw.flags = 4 if layout else 0                        # DABGPU_CW_CLASSED
                cws.append(cw)
            ctx.viterbi_decode_batch(cws, d_res)
            torch.cuda.synchronize()
            res = results_np(d_res)
            what = (H, newest, layout, mapping, si)
            assert np.array_equal(d_o.cpu().numpy(), truth["out"][:, off:off + nb]), what
            assert np.array_equal(res["path_error"], truth["res"]["path_error"][:, si]) and (res["n_out_bytes"] == nb).all(), what
            off += nb
    finally:
        ctx.viterbi_set_mapping(0)


@pytest.mark.parametrize("form", ["frames", "ring"])
def test_ber_reads_the_ring_at_the_edge(ctx, truth, ring, form):
    import dabgpu
    import torch
    n_sub = len(truth["gsubs"])
    dt = np.dtype(dabgpu.BER_RESULT_DTYPE)
    d_fib, d_msc = torch.from_numpy(truth["fib"]).cuda(), torch.from_numpy(truth["out"]).cuda()
    fic_r = torch.full((4 * dt.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    msc_r = torch.full((4 * n_sub * dt.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    args = (truth["gsubs"], d_fib, d_msc, 4 * truth["cif_out"], fic_r, msc_r)
    if form == "ring":
        d_slots = torch.tensor([ring["newest"]], dtype=torch.int32, device="cuda")
        ctx.ber_ring(ring["view"], 1, ring["H"] * NB, ring["H"], d_slots, *args, bits_layout=ring["layout"])
    else:
        ctx.ber_frames(ring["view"], 1, ring["H"] * NB, ring["H"], ring["newest"], *args, bits_layout=ring["layout"])
    torch.cuda.synchronize()
    assert np.array_equal(fic_r.cpu().numpy().view(dt), truth["ber_fic"])
    assert np.array_equal(msc_r.cpu().numpy().view(dt).reshape(4, n_sub), truth["ber_msc"])
    assert (truth["ber_msc"]["n_errors"] > 0).sum() >= 8, "the noise must leave channel errors to count"


# ---- writers into the top slot of the 18642-frame ring ----

@pytest.fixture()
def top_slot():
    """(view of the ring, byte offset of its top slot, canaries): the slot lies past 2^32 - 230400, its end past 2^32"""
    H = 18642
    view = BB.big(H * NB)
    off = (H - 1) * NB
    assert off < BB.WRAP < off + NB
    can = BB.Canaries()
    can.at(view, off - BB.CANARY_BYTES)                                  # the end of the slot below
    can.at(view, off + NB - BB.WRAP)                                     # where the part of the slot past 2^32 would wrap to
    can.at(view, off - BB.WRAP)                                          # the slot as a whole, 2^32 lower (inside the lead)
    can.at(view, off - BB.WRAP + NB - BB.CANARY_BYTES)
    BB.region(view, off, NB).fill_(0x5A)
    yield view, off, H, can
    del view, can
    BB.release()


@pytest.mark.parametrize("layout", [0, 1], ids=["natural", "classed"])
def test_history_demodulator_writes_the_top_slot(ctx, top_slot, layout):
    import dabgpu
    import torch
    view, off, H, can = top_slot
    fmt = dabgpu.IQ_FORMATS.index("raw_u8")
    g = torch.Generator(device="cuda").manual_seed(77)
    raw = torch.randint(0, 256, (dabgpu.NB_FRAME_SAMPLES * 2,), dtype=torch.uint8, device="cuda", generator=g)
    packed = torch.full((NB,), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.ofdm_demod_frames_history(raw, fmt, 1, packed, bits_layout=layout)
    ctx.ofdm_demod_frames_history(raw, fmt, 1, BB.region(view, off, NB), bits_frame_stride=H * NB, bits_layout=layout)
    torch.cuda.synchronize()
    assert not bool((packed == 0x5A).all())
    assert torch.equal(BB.region(view, off, NB), packed)
    can.check()


@pytest.mark.parametrize("layout", [0, 1], ids=["natural", "classed"])
def test_diversity_combiner_writes_the_top_slot(ctx, top_slot, layout):
    import torch
    view, off, H, can = top_slot
    g = torch.Generator(device="cuda").manual_seed(78)
    dq = [torch.randn((1, 75, 1536, 2), dtype=torch.float32, device="cuda", generator=g) for _ in range(2)]
    scale = [torch.full((1,), 40.0 + 9 * b, dtype=torch.float32, device="cuda") for b in range(2)]
    table = [(dq[b], scale[b]) for b in range(2)]
    packed = torch.full((NB,), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.diversity_combine(table, 1, packed, bits_layout=layout)
    ctx.diversity_combine(table, 1, BB.region(view, off, NB), bits_frame_stride=H * NB, bits_layout=layout)
    torch.cuda.synchronize()
    assert not bool((packed == 0x5A).all())
    assert torch.equal(BB.region(view, off, NB), packed)
    can.check()


def test_weighted_stream_bank_ring_form_writes_the_second_streams_ring(ctx, oracle):
    """the stream bank chooses the ring slot itself (frame count mod hist_frames), so the top slot of a large ring cannot be placed; but
    with two streams and hist_frames = 18642 the second stream's ring begins 18642 * 230400 >= 2^32 bytes behind the first's after a
    single frame, and its scale words at [18642 + slot].  Against the same blocks into rings of 5 frames (the streams hold four; a ring
    call takes at most 191400 samples, one frame per stream)."""
    import dabgpu
    import stream_soft_model as SSM
    import torch
    S = SSM.float_streams(oracle)[:2]
    n = S.shape[1] // 8 * 8
    d_x = torch.from_numpy(np.ascontiguousarray(S[:, :n])).cuda()
    fmt = dabgpu.IQ_FORMATS.index("raw_f32l")
    H = 18642
    view = BB.big(2 * H * NB)
    can = BB.Canaries()
    can.at(view, -BB.CANARY_BYTES)
    can.at(view, H * NB - BB.CANARY_BYTES)                               # the end of stream 0's ring, never reached
    can.at(view, H * NB + 5 * NB)                                        # behind the slots four frames can reach
    can.at(view, H * NB - BB.WRAP + 5 * NB)                              # ... and 2^32 below (stream 0's slots 0 .. 4 are compared)
    got = []
    for hist, h in ((view, H), (torch.full((2, 5, NB), 0x5A, dtype=torch.uint8, device="cuda"), 5)):
        if hist is view:
            for s in range(2):
                BB.region(view, s * H * NB, 5 * NB).fill_(0x5A)
        bank = dabgpu.StreamBank(ctx, 2)
        scale = torch.full((2 * h,), -1.0, dtype=torch.float32, device="cuda")
        bank.set_soft(dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0), scale)
        slot = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        for k in range(0, n, 191400):
            bank.process_ring(d_x[:, k:].data_ptr(), fmt, n, min(191400, n - k), hist, h, slot)
        torch.cuda.synchronize()
        bank.close()
        got.append((slot.cpu().numpy(), scale))
    can.check()
    assert got[0][0].tolist() == got[1][0].tolist() and 1 <= min(got[0][0]) and max(got[0][0]) <= 4, got[0][0]
    for s in range(2):
        assert torch.equal(BB.region(view, s * H * NB, 5 * NB), hist[s].reshape(-1)), s
        assert torch.equal(got[0][1][s * H:s * H + 5].view(torch.int32), got[1][1][s * 5:s * 5 + 5].view(torch.int32)), s
    assert not torch.equal(hist[0, 0], hist[1, 0]) and not bool((hist[:, 0] == 0x5A).all())
    del view, can
    BB.release()
