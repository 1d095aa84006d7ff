"""The synchroniser kernel at its edges, bit for bit against the oracle: the table of tests/sync_cases.py (position, scale, non-finite,
coarse-edge, tracking, cfg) of every transmission mode in ONE launch per configuration and tracking step, n_streams = len(table),
stride nb_fft + 3 (8-byte but not 16-byte aligned rows, the padding NaN), every stream with its own incoming record.  The quirks of the
reference that the kernel must share: dB values weighted by distance (below 0 dB the weight prefers far positions), the scan starting from
the unweighted index 0, and a NaN response passing the !((max - avg) < threshold) test."""
import numpy as np
import pytest

import sync_cases as SC

pytestmark = pytest.mark.gpu
MODES = [1, 2, 3, 4]
SENTINEL = 0x7FC5A5A5                 # a NaN pattern the kernel never produces: a response row that still holds it was not written
VALID_IN = 77                         # incoming sync_valid: an out field, must always be overwritten
_RUNS = {}


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    """float32 arrays as uint32 patterns (-inf equals -inf that way), NaN matched as NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return bool(np.all((u32(a) == u32(b)) | (np.isnan(a) & np.isnan(b))))


def incoming(dabgpu, cases):
    st = np.zeros(len(cases), dtype=np.dtype(dabgpu.SYNC_STATE_DTYPE))
    for i, c in enumerate(cases):
        st[i] = (c.state[0], c.state[1], c.state[2], c.state[3], VALID_IN, 1000 + i)
    return st


def launch(ctx, mode, d_syms, n, stride, d_st, cfg, d_imp, d_frq):
    import dabgpu
    if mode == 1:
        ctx.ofdm_sync(d_syms, n, stride, d_st, cfg=cfg, impulse=d_imp, freq_response=d_frq)
    else:
        import ctypes as C
        dabgpu.check(dabgpu.lib().dabgpu_ofdm_sync_mode(ctx._h, mode, dabgpu._ptr(d_syms), n, stride, C.byref(cfg), dabgpu._ptr(d_st),
                                                        dabgpu._ptr(d_imp), dabgpu._ptr(d_frq), ctx._stream(None)), "dabgpu_ofdm_sync_mode")


def run_batch(ctx, mode, want_imp=True, want_frq=True):
    """-> per case, per step: (record, impulse row or None, freq row or None).  One launch per configuration and step over ALL streams;
    only the streams of that configuration are kept, the tracking sequences are consecutive launches on the same state buffer."""
    key = (mode, want_imp, want_frq)
    if key in _RUNS:
        return _RUNS[key]
    import dabgpu
    import torch
    cases = SC.table(mode)
    n, N = len(cases), SC.expected(mode)[0][0].impulse.size
    stride = N + 3
    n_steps = max(len(c.symbols) for c in cases)
    d_syms = []
    for k in range(n_steps):
        syms = np.full((n, stride), np.complex64(complex(np.nan, np.nan)), dtype=np.complex64)
        for i, c in enumerate(cases):
            syms[i, :N] = c.symbols[min(k, len(c.symbols) - 1)]
        d_syms.append(torch.from_numpy(syms.view(np.float32)).cuda())
    fill = np.full((n, N), SENTINEL, dtype=np.uint32).view(np.float32)
    out = [[] for _ in cases]
    for cfg_key in SC.configs(cases):
        sel = [i for i, c in enumerate(cases) if c.cfg == cfg_key]
        cfg = SC.make_cfg(dabgpu, cfg_key)
        d_st = torch.from_numpy(incoming(dabgpu, cases).view(np.uint8)).cuda()
        for k in range(max(len(cases[i].symbols) for i in sel)):
            d_imp = torch.from_numpy(fill.copy()).cuda() if want_imp else None
            d_frq = torch.from_numpy(fill.copy()).cuda() if want_frq else None
            launch(ctx, mode, d_syms[k], n, stride, d_st, cfg, d_imp, d_frq)
            torch.cuda.synchronize()
            st = d_st.cpu().numpy().view(np.dtype(dabgpu.SYNC_STATE_DTYPE)).copy()
            imp = d_imp.cpu().numpy() if want_imp else None
            frq = d_frq.cpu().numpy() if want_frq else None
            for i in sel:
                if k < len(cases[i].symbols):
                    out[i].append((st[i].copy(), imp[i].copy() if want_imp else None, frq[i].copy() if want_frq else None))
    _RUNS[key] = out
    return out


def as_steps(cases, rows):
    """the device's records in the shape sync_cases.kinds_of reads"""
    out = []
    for c, steps in zip(cases, rows):
        prev = (np.float32(c.state[0]), np.float32(c.state[1]), c.state[2], c.state[3])
        conv = []
        for rec, imp, frq in steps:
            written = not np.all(u32(frq) == SENTINEL)
            conv.append(SC.Step(rec["freq_coarse"], rec["freq_fine"], int(rec["is_found_coarse"]), int(rec["sync_valid"]),
                                int(rec["fine_time_offset"]), frq if written else None, imp, *prev))
            prev = (rec["freq_coarse"], rec["freq_fine"], int(rec["is_found_coarse"]), int(rec["fine_time_offset"]))
        out.append(conv)
    return out


@pytest.mark.parametrize("mode", MODES)
def test_sync_edge_table_matches_oracle(ctx, oracle, mode):
    cases, exp, got = SC.table(mode), SC.expected(mode), run_batch(ctx, mode)
    bad = []
    for i, (c, e_steps, g_steps) in enumerate(zip(cases, exp, got)):
        assert len(e_steps) == len(g_steps) == len(c.symbols)
        for k, (e, (rec, imp, frq)) in enumerate(zip(e_steps, g_steps)):
            what = []
            if not same_bits(rec["freq_coarse"], e.coarse):
                what.append(f"freq_coarse {rec['freq_coarse']!r} != {e.coarse!r}")
            if not same_bits(rec["freq_fine"], e.fine):
                what.append(f"freq_fine {rec['freq_fine']!r} != {e.fine!r}")
            ints = (int(rec["is_found_coarse"]), int(rec["sync_valid"]), int(rec["fine_time_offset"]), int(rec["reserved"]))
            if ints != (e.found, e.valid, e.offset, 1000 + i):
                what.append(f"(found, valid, offset, reserved) {ints} != {(e.found, e.valid, e.offset, 1000 + i)}")
            if not same_bits(imp, e.impulse):
                what.append("impulse response")
            if e.freq_resp is None:
                if not np.all(u32(frq) == SENTINEL):
                    what.append("coarse response written with the coarse stage disabled")
            elif not same_bits(frq, e.freq_resp):
                what.append("coarse response")
            if what:
                bad.append((c.name, k, what))
    assert not bad, (mode, len(bad), bad[:8])


@pytest.mark.parametrize("mode", MODES)
def test_sync_edge_table_covers_every_kind_on_the_device(ctx, oracle, mode):
    """the (sync_valid, fine_time_offset) pairs, states and responses the DEVICE returned contain every kind of sync_cases.KINDS: a later edit of
    the table cannot silently empty a group"""
    cases = SC.table(mode)
    kinds = SC.kinds_of(mode, cases, as_steps(cases, run_batch(ctx, mode)))
    assert all(kinds[k] for k in SC.KINDS), {k: len(v) for k, v in kinds.items()}
    assert {c.group for c in cases} == set(SC.GROUPS)


@pytest.mark.parametrize("mode", MODES)
def test_sync_optional_outputs_do_not_change_the_records(ctx, oracle, mode):
    """(impulse, freq) given as (ptr, NULL), (NULL, ptr), (NULL, NULL): the records equal the full launch's, and so does the buffer that was passed"""
    full = run_batch(ctx, mode)
    for want_imp, want_frq in ((True, False), (False, True), (False, False)):
        part = run_batch(ctx, mode, want_imp, want_frq)
        for c, f_steps, p_steps in zip(SC.table(mode), full, part):
            assert len(f_steps) == len(p_steps)
            for k, ((rec_f, imp_f, frq_f), (rec_p, imp_p, frq_p)) in enumerate(zip(f_steps, p_steps)):
                where = (mode, want_imp, want_frq, c.name, k)
                assert rec_f.tobytes() == rec_p.tobytes(), where
                assert (imp_p is None) == (not want_imp) and (frq_p is None) == (not want_frq)
                if want_imp:
                    assert np.array_equal(u32(imp_f), u32(imp_p)), where
                if want_frq:
                    assert np.array_equal(u32(frq_f), u32(frq_p)), where


@pytest.mark.parametrize("mode", MODES)
def test_sync_host_form_equals_the_batch_row(ctx, oracle, mode):
    """every case again through dabgpu_ofdm_sync_host_sync / _host_sync_mode: record and both responses bit-identical to the stream's row"""
    import dabgpu
    cases, batch = SC.table(mode), run_batch(ctx, mode)
    dt = np.dtype(dabgpu.SYNC_STATE_DTYPE)
    for i, (c, rows) in enumerate(zip(cases, batch)):
        cfg = SC.make_cfg(dabgpu, c.cfg)
        st = dabgpu.SyncState(c.state[0], c.state[1], c.state[2], c.state[3], VALID_IN, 1000 + i)
        for k, (sym, (rec, imp, frq)) in enumerate(zip(c.symbols, rows)):
            if mode == 1:
                st, h_imp, h_frq = ctx.ofdm_sync_host(sym, st, cfg)
            else:
                h_imp, h_frq = ctx.ofdm_sync_host_mode(mode, sym, st, cfg)
            where = (mode, c.name, k)
            assert bytes(st) == rec.tobytes(), where + (np.frombuffer(bytes(st), dt), rec)
            assert np.array_equal(u32(h_imp), u32(imp)), where
            if cfg.is_coarse_freq_correction:                    # (disabled: the coarse response is not produced)
                assert np.array_equal(u32(h_frq), u32(frq)), where
