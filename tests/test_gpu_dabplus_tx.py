"""-m gpu: the DAB+ super-frame encoder on the device (dabgpu_dabplus_tx_*, dab-radio_amd/csrc/dabplus_tx.hip).  Integer work: every
comparison is byte equality -- against the committed vectors (tests/golden/dabplus_tx_vectors.npz: the model's bytes, accepted by the
reference's own AAC_Frame_Processor when they were made), against the numpy model on a mixed batch, through the library's own DAB+ decoder
with and without damage, through the whole transmit and receive chain, through the C++ mirror class, and replayed from a HIP graph."""
import os
import subprocess

import numpy as np
import pytest

import dabplus_tx_model as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
FILL = 0xC3
DESCRIPTORS = (0x13, 0x3A, 0x51, 0x6F)


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vectors():
    v = np.load(os.path.join(ROOT, "tests", "golden", "dabplus_tx_vectors.npz"))
    cases = []
    for i, name in enumerate(str(s) for s in v["names"]):
        n, d, lens = int(v["frame_bytes"][i]), int(v["descriptor"][i]), [int(x) for x in v["au_len"][i]]
        blob, aus, off = v[f"au_{i}"], [], 0
        for a in range(T.num_aus_of(d)):
            aus.append(blob[off:off + lens[a]]); off += lens[a]
        cases.append(dict(name=name, n=n, d=d, aus=aus, frames=v[f"frames_{i}"], status=int(v["status"][i])))
    return cases


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def run_encode(ctx, streams, stream_offsets, stride, total_bytes, stream=None):
    """streams: [(frame_bytes, [(descriptor, aus), ...])] -> (uint8 [total_bytes] as the device left it (pre-filled with FILL), status [S][K]);
    the output sits between two guard patterns"""
    import dabgpu
    import torch
    S, K = len(streams), len(streams[0][1])
    au, offs, lens, desc, fbytes = T.pack_call(streams)
    whole = torch.full((GUARD + total_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    view = whole[GUARD:GUARD + total_bytes]
    status = torch.full((S, K), -7, dtype=torch.int32, device="cuda")
    dabgpu.DabPlusTx(ctx).encode(S, K, dev(au), dev(offs), dev(lens), dev(desc), dev(fbytes), view, dev(np.asarray(stream_offsets, np.uint64)), stride,
                                 status, stream=stream)
    torch.cuda.synchronize()
    h = whole.cpu().numpy()
    assert (h[:GUARD] == FILL).all() and (h[-GUARD:] == FILL).all(), "the encoder wrote outside its output"
    return h[GUARD:GUARD + total_bytes], status.cpu().numpy()


def expected_image(streams, stream_offsets, stride, total_bytes):
    """what the call leaves in a buffer pre-filled with FILL, by the model: only a stream's own bytes change"""
    img = np.full(total_bytes, FILL, np.uint8)
    status = np.zeros((len(streams), len(streams[0][1])), np.int32)
    for s, (n, sfs) in enumerate(streams):
        for k, (d, aus) in enumerate(sfs):
            frames, status[s, k] = T.encode(d, aus, n)
            w = min(n, T.MAX_FRAME_BYTES)                 # (a refused frame size: the first min(n, 1536) bytes of each frame are zeroed)
            for j in range(5):
                at = int(stream_offsets[s]) + (5 * k + j) * stride
                img[at:at + w] = frames[j * n:j * n + w]
    return img, status


def test_golden_cases_device_and_host_entry_points(ctx, vectors):
    import dabgpu
    tx = dabgpu.DabPlusTx(ctx)
    seen = set()
    for c in vectors:
        n, stride = c["n"], (max(c["n"], 4) + 3) & ~3
        got, st = run_encode(ctx, [(n, [(c["d"], c["aus"])])], [0], stride, 5 * stride)
        exp, est = expected_image([(n, [(c["d"], c["aus"])])], [0], stride, 5 * stride)
        assert int(st[0, 0]) == c["status"] == int(est[0, 0]), c["name"]
        w = min(n, T.MAX_FRAME_BYTES)
        for j in range(5):
            assert np.array_equal(got[j * stride:j * stride + w], c["frames"][j * n:j * n + w]), (c["name"], "frame", j)
        assert np.array_equal(got, exp), (c["name"], "bytes outside the frames")
        frames, hst = tx.encode_host(n, [(c["d"], c["aus"])])
        assert int(hst[0]) == c["status"], c["name"]
        assert np.array_equal(frames[:, :w].reshape(5, w), c["frames"].reshape(5, n)[:, :w]), (c["name"], "host form")
        seen.add(c["status"])
    assert seen == {0, 1, 2, 3}


def mixed_streams(rng, n_streams, K):
    sizes = (24, 48, 72, 768, 792, 816, 1512, 1536)
    streams = []
    for s in range(n_streams):
        n = sizes[s % len(sizes)]
        sfs = []
        for k in range(K):
            d = DESCRIPTORS[(s + k) % 4] | (int(rng.integers(0, 2)) << 7)
            shape = ("random", "zeros", "random")[(s // 8 + k) % 3]
            lens = T.split_lengths(rng, d, n, shape)
            sfs.append((d, [rng.integers(0, 256, l, dtype=np.uint8) for l in lens]))
        streams.append((n, sfs))
    return streams


@pytest.mark.parametrize("K", [1, 2, 5])
def test_mixed_batch_equals_the_model(ctx, K):
    """67 streams (more blocks than a wavefront has lanes), frame sizes around every threshold of the parity mapping, in two layouts: each
    stream's frames back to back, and all streams interleaved in shared records (stride = sum of the sizes) where a stream's neighbours' bytes
    lie between its frames"""
    rng = np.random.default_rng(6100 + K)
    S = 67
    streams = mixed_streams(rng, S, K)
    sizes = np.array([n for n, _ in streams], np.uint64)
    # dense per stream, 8 spare bytes behind each frame
    stride = 1536 + 8
    offs = np.arange(S, dtype=np.uint64) * np.uint64(5 * K * stride)
    total = int(S * 5 * K * stride)
    got, st = run_encode(ctx, streams, offs, stride, total)
    exp, est = expected_image(streams, offs, stride, total)
    assert np.array_equal(st, est) and not st.any()
    assert np.array_equal(got, exp), f"first difference at byte {int(np.argmax(got != exp))}"
    # records shared by all streams, like the CIF records of a multiplex
    record = int(sizes.sum())
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    total = 5 * K * record
    got, st = run_encode(ctx, streams, offs, record, total)
    exp, est = expected_image(streams, offs, record, total)
    assert np.array_equal(st, est)
    assert np.array_equal(got, exp), f"first difference at byte {int(np.argmax(got != exp))}"


def test_invalid_super_frames_between_valid_ones(ctx):
    rng = np.random.default_rng(6200)

    def valid(n, d):
        return (d, [rng.integers(0, 256, l, dtype=np.uint8) for l in T.split_lengths(rng, d, n)])

    def with_lengths(d, lens):
        return (d, [rng.integers(0, 256, l, dtype=np.uint8) for l in lens])
    good = T.split_lengths(rng, 0x6F, 96)
    short = list(good)
    short[int(np.argmax(good))] -= 1
    room = 110 * 64 - 5 - 4
    streams = [
        (96, [valid(96, 0x13), with_lengths(0x6F, short), valid(96, 0x51), with_lengths(0x6F, [good[0], good[1] + 1, good[2]]),
              valid(96, 0x3A)]),
        (1536, [valid(1536, 0x3A), with_lengths(0x3A, [4096 - 7, room - (4096 - 7)]), with_lengths(0x3A, [4095 - 7, room - (4095 - 7)]), valid(1536, 0x51),
                with_lengths(0x51, [0xFFFF, 0, 0, 0, 0, 0])]),
        (100, [valid(96, 0x13)] * 5),                       # a frame size that is no multiple of 24: every super frame refused
        (1560, [valid(96, 0x13)] * 5),                      # above 1536: 1536 bytes of each frame zeroed, the other 24 untouched
        (48, [valid(48, 0x6F) for _ in range(5)]),
    ]
    stride = 1560
    offs = np.arange(len(streams), dtype=np.uint64) * np.uint64(25 * stride)
    total = len(streams) * 25 * stride
    got, st = run_encode(ctx, streams, offs, stride, total)
    exp, est = expected_image(streams, offs, stride, total)
    assert st.tolist() == [[0, 2, 0, 2, 0], [0, 3, 0, 0, 2], [1] * 5, [1] * 5, [0] * 5] == est.tolist()
    assert np.array_equal(got, exp), f"first difference at byte {int(np.argmax(got != exp))}"
    # the refused ones are five zero frames
    assert not got[int(offs[0]) + 5 * stride:int(offs[0]) + 5 * stride + 96].any() and not got[int(offs[2]):int(offs[2]) + 100].any()
    assert (got[int(offs[3]) + 1536:int(offs[3]) + 1560] == FILL).all()


def decode_streams(ctx, frames_dev, offs, stride, sizes, n_frames):
    """dabgpu_dabplus_bank_process over fresh decoder states -> (records [S][max_sf], super frames [S][max_sf][7680], counts [S][4])"""
    import dabgpu
    import torch
    S = len(sizes)
    bank = dabgpu.DabPlusBank(ctx, S)
    max_sf = (n_frames + 4) // 5
    d_sf = torch.zeros((S, max_sf, 7680), dtype=torch.uint8, device="cuda")
    rdt = np.dtype(dabgpu.SUPERFRAME_RESULT_DTYPE)
    d_res = torch.zeros((S, max_sf, rdt.itemsize), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros((S, 4), dtype=torch.int32, device="cuda")
    bank.process(frames_dev, dev(np.asarray(offs, np.uint64)), stride, dev(np.asarray(sizes, np.uint32)), n_frames, d_sf, 7680, d_res, max_sf, d_cnt)
    torch.cuda.synchronize()
    out = d_res.cpu().numpy().view(rdt).reshape(S, max_sf), d_sf.cpu().numpy(), d_cnt.cpu().numpy()
    bank.close()
    return out


def test_round_trip_through_the_device_decoder_clean_and_damaged(ctx):
    import dabplus_model as M
    import torch
    rng = np.random.default_rng(6300)
    sizes = [24, 72, 192, 264, 792, 1536]
    K = 3
    streams = []
    for s, n in enumerate(sizes):
        sfs = []
        for k in range(K):
            d = DESCRIPTORS[(s + k) % 4]
            sfs.append((d, [rng.integers(0, 256, l, dtype=np.uint8) for l in T.split_lengths(rng, d, n)]))
        streams.append((n, sfs))
    stride = 1536
    offs = np.arange(len(sizes), dtype=np.uint64) * np.uint64(5 * K * stride)
    total = len(sizes) * 5 * K * stride
    got, st = run_encode(ctx, streams, offs, stride, total)
    assert not st.any()
    res, sfs, cnt = decode_streams(ctx, torch.from_numpy(got.copy()).cuda(), offs, stride, sizes, 5 * K)
    clean = {}
    for s, (n, lst) in enumerate(streams):
        assert cnt[s, 0] == K and cnt[s, 1] == 0, (n, cnt[s])
        for k, (d, aus) in enumerate(lst):
            r, na = res[s, k], T.num_aus_of(d)
            assert r["firecode_ok"] and r["rs_corrected"] == 0 and r["rs_failed_index"] == -1 and int(r["au_crc_ok_mask"]) == (1 << na) - 1, (n, k, r)
            sent = np.concatenate([got[int(offs[s]) + (5 * k + j) * stride:][:n] for j in range(5)])
            assert np.array_equal(sfs[s, k, :5 * n], sent)
            start = r["au_start"]
            for a in range(na):
                assert np.array_equal(sfs[s, k, start[a]:start[a] + len(aus[a])], aus[a]), (n, k, a)
            clean[s, k] = sent
    # 1..5 damaged symbols per code word: the decoder returns the encoder's bytes and counts exactly the damage.  (The first super frame
    # stays clean: an unsynchronised decoder tests the fire code of a frame BEFORE any correction, aac_frame_processor.cpp:162-166.)
    bad = got.copy()
    damage = {(s, 0): 0 for s in range(len(sizes))}
    for s, (n, lst) in enumerate(streams):
        for k in range(1, K):
            e = 1 + (s + 2 * k) % 5
            hurt = M.corrupt(rng, clean[s, k], e)
            damage[s, k] = e * (n // 24)
            for j in range(5):
                at = int(offs[s]) + (5 * k + j) * stride
                bad[at:at + n] = hurt[j * n:(j + 1) * n]
    res, sfs, cnt = decode_streams(ctx, torch.from_numpy(bad).cuda(), offs, stride, sizes, 5 * K)
    for (s, k), sent in clean.items():
        r = res[s, k]
        assert r["rs_failed_index"] == -1 and int(r["rs_corrected"]) == damage[s, k] and r["firecode_ok"], (s, k, r)
        assert np.array_equal(sfs[s, k, :sent.size], sent), (s, k)


def test_whole_chain_access_units_to_iq_and_back(ctx):
    """DabPlusTx into a TxBank payload -> transmit_frames -> demodulator -> dabgpu_decode_frames_layout -> DabPlusBank, two blocks of 5 frames
    (20 CIFs = 4 super frames each) so that the 16-CIF interleaver has flushed: the super frames that came through whole hand back the
    transmitted access units; the plain sub-channel between the two DAB+ ones is not touched by the encoder and arrives as sent"""
    import dabgpu
    import torch
    import tx_encode_cases as X
    subs = [dict(start=0, length=12, is_uep=0, uep_index=0, eep_level=2, eep_type=0),          # 16 kbit/s: 48-byte logical frames
            dict(start=12, length=24, is_uep=0, uep_index=0, eep_level=2, eep_type=0),         # plain data, 96 bytes per CIF
            dict(start=40, length=48, is_uep=0, uep_index=0, eep_level=2, eep_type=0)]         # 64 kbit/s: 192-byte logical frames
    gsubs = [X.g_sub(dabgpu, d) for d in subs]
    E, F, H, BLOCKS = 2, 5, 8, 2
    bank = dabgpu.TxBank(ctx, E, gsubs)
    nb = bank.cif_in_bytes
    plus = [0, 2]
    offs, stride, fbytes = dabgpu.dabplus_tx_offsets(bank, plus, F)
    assert stride == nb and list(fbytes) == [48, 192] * E and nb == 48 + 96 + 192
    rng = np.random.default_rng(6400)
    tx = dabgpu.DabPlusTx(ctx)
    fmt = dabgpu.IQ_FORMATS.index("raw_f32l")
    hist = torch.zeros((E, H, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
    fib = torch.zeros((E, 4, 96), dtype=torch.uint8, device="cuda"); fres = torch.zeros((E * 4, 16), dtype=torch.uint8, device="cuda")
    out = torch.zeros((E, 4, nb), dtype=torch.uint8, device="cuda"); res = torch.zeros((E * 4 * 3, 16), dtype=torch.uint8, device="cuda")
    sent_units, sent_plain, received = {}, [], []
    for b in range(BLOCKS):
        streams = []
        for e in range(E):
            for si in plus:
                n = int(fbytes[plus.index(si)])
                sfs = []
                for k in range(4):
                    d = DESCRIPTORS[(b + e + si + k) % 4]
                    sfs.append((d, [rng.integers(0, 256, l, dtype=np.uint8) for l in T.split_lengths(rng, d, n)]))
                    sent_units[e, si, 4 * b + k] = sfs[-1]
                streams.append((n, sfs))
        fib_in, pay = X.random_input(rng, E, F, nb)
        d_pay = dev(pay)
        au, au_offs, lens, desc, fb = T.pack_call(streams)
        status = torch.full((len(streams), 4), -7, dtype=torch.int32, device="cuda")
        tx.encode(len(streams), 4, dev(au), dev(au_offs), dev(lens), dev(desc), dev(fb), d_pay, dev(offs), stride, status)
        torch.cuda.synchronize()
        assert not status.cpu().numpy().any()
        after = d_pay.cpu().numpy().reshape(E, 4 * F, nb)
        assert np.array_equal(after[:, :, 48:144], pay.reshape(E, 4 * F, nb)[:, :, 48:144]), "the encoder touched the plain sub-channel"
        sent_plain.append(after[:, :, 48:144].copy())
        iq = torch.zeros((E, F, 196608, 2), dtype=torch.float32, device="cuda")
        bank.transmit_frames(dev(fib_in), d_pay, F, iq)
        for j in range(F):
            frame = torch.zeros((E, 196608, 2), dtype=torch.float32, device="cuda")
            frame[:, :196608 - 2656] = iq[:, j, 2656:]
            g = b * F + j
            ctx.ofdm_demod_frames_history(frame, fmt, E, hist[:, g % H], bits_frame_stride=H * dabgpu.NB_FRAME_BITS)
            ctx.decode_frames(hist, E, H * dabgpu.NB_FRAME_BITS, H, g % H, gsubs, fib, fres, out, 4 * nb, res)
            torch.cuda.synchronize()
            o = out.cpu().numpy()
            for c in range(4):
                if 4 * g + c >= 15:
                    received.append(o[:, c].copy())
    rx = np.stack(received, axis=1)                          # [E][25][nb]: transmitted CIFs 0..24
    n_rx = rx.shape[1]
    assert n_rx == 4 * F * BLOCKS - 15 == 25
    plain = np.concatenate(sent_plain, axis=1)
    assert np.array_equal(rx[:, :, 48:144], plain[:, :n_rx])
    rx_offs = [e * n_rx * nb + bank.plan["subs"][si].in_offset for e in range(E) for si in plus]
    recs, sfs, cnt = decode_streams(ctx, dev(rx), rx_offs, nb, [48, 192] * E, n_rx)
    for s, (e, si) in enumerate((e, si) for e in range(E) for si in plus):
        assert cnt[s, 0] == 5 and cnt[s, 1] == 0, cnt[s]
        for k in range(5):
            d, aus = sent_units[e, si, k]
            r, na = recs[s, k], T.num_aus_of(d)
            assert r["firecode_ok"] and r["rs_corrected"] == 0 and int(r["descriptor"]) == d and int(r["au_crc_ok_mask"]) == (1 << na) - 1, (e, si, k, r)
            for a in range(na):
                st = int(r["au_start"][a])
                assert np.array_equal(sfs[s, k, st:st + len(aus[a])], aus[a]), (e, si, k, a)
    bank.close()


def test_mirror_class_equals_the_vectors(tmp_path, vectors):
    harness = os.path.join(ROOT, "tests", "cpp", "dabplus_tx_harness")
    if not os.path.exists(harness):
        import __graft_entry__ as g
        g.build()
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "dab-radio_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    by_name = {c["name"]: c for c in vectors}
    picked = [by_name[k] for k in ("rand_192_13", "rand_192_51", "rand_192_6f")]
    # a fourth super frame the class must refuse: the lengths of another frame size
    blob = np.array([192, 4], np.uint32).tobytes()
    for c in picked + [dict(by_name["rand_72_3a"])]:
        blob += bytes([c["d"], len(c["aus"])]) + np.array([len(a) for a in c["aus"]], np.uint16).tobytes() + b"".join(bytes(a) for a in c["aus"])
    (tmp_path / "in.bin").write_bytes(blob)
    res = subprocess.run([harness, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, env=env, timeout=300)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.uint8).reshape(4, 2 + 5 * 192)
    for k, c in enumerate(picked):
        assert got[k, 0] == 1 and got[k, 1] == 0 and np.array_equal(got[k, 2:], c["frames"]), c["name"]
    assert got[3, 0] == 0 and got[3, 1] == 2 and not got[3, 2:].any()


def test_captured_call_replays_on_new_contents(ctx):
    import dabgpu
    import torch
    rng = np.random.default_rng(6500)
    S, K, stride = 9, 2, 792
    sizes = (24, 192, 792)

    def make():
        streams = []
        for s in range(S):
            n = sizes[s % 3]
            streams.append((n, [(DESCRIPTORS[(s + k) % 4], None) for k in range(K)]))
        # the same descriptors and frame sizes every time, other lengths and bytes
        return [(n, [(d, [rng.integers(0, 256, l, dtype=np.uint8) for l in T.split_lengths(rng, d, n)]) for d, _ in sfs]) for n, sfs in streams]
    first, second = make(), make()
    offs = np.arange(S, dtype=np.uint64) * np.uint64(5 * K * stride)
    total = S * 5 * K * stride
    au, au_offs, lens, desc, fb = T.pack_call(first)
    cap = max(au.size, T.pack_call(second)[0].size)
    d_au = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_au[:au.size] = dev(au)
    d_offs, d_lens, d_desc, d_fb, d_so = dev(au_offs), dev(lens), dev(desc), dev(fb), dev(offs)
    whole = torch.full((GUARD + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    view = whole[GUARD:GUARD + total]
    status = torch.full((S, K), -7, dtype=torch.int32, device="cuda")
    tx = dabgpu.DabPlusTx(ctx)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        tx.encode(S, K, d_au, d_offs, d_lens, d_desc, d_fb, view, d_so, stride, status, stream=side.cuda_stream)       # once eagerly
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        tx.encode(S, K, d_au, d_offs, d_lens, d_desc, d_fb, view, d_so, stride, status, stream=side.cuda_stream)
    for streams in (first, second):
        au, au_offs, lens, desc, fb = T.pack_call(streams)
        d_au[:au.size] = dev(au); d_offs.copy_(dev(au_offs)); d_lens.copy_(dev(lens)); d_desc.copy_(dev(desc))
        view.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        h = whole.cpu().numpy()
        exp, est = expected_image(streams, offs, stride, total)
        assert (h[:GUARD] == FILL).all() and (h[-GUARD:] == FILL).all()
        assert np.array_equal(h[GUARD:GUARD + total], exp) and not status.cpu().numpy().any()


def test_arguments_are_checked_before_any_device_call(ctx):
    import dabgpu
    import torch
    L = dabgpu.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    args = lambda **kw: [kw.get("ctx", ctx._h), kw.get("S", 1), kw.get("K", 1), kw.get("au", p), p, p, p, p, kw.get("frames", p), p, kw.get("stride", 24), p, None]
    assert L.dabgpu_dabplus_tx_encode(*args(ctx=None)) == 2
    assert L.dabgpu_dabplus_tx_encode(*args(K=-1)) == 2
    assert L.dabgpu_dabplus_tx_encode(*args(stride=26)) == 2
    assert L.dabgpu_dabplus_tx_encode(*args(frames=p + 2)) == 2
    assert L.dabgpu_dabplus_tx_encode(*args(au=None)) == 2
    assert L.dabgpu_dabplus_tx_encode(*args(S=0, au=None)) == 0 and L.dabgpu_dabplus_tx_encode(*args(K=0, au=None)) == 0
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any()


def test_stream_offset_off_the_dword_grid_costs_nothing_but_speed(ctx):
    """the precondition says stream offsets are multiples of 4; they live on the device, so the host cannot refuse one that is not: the
    kernel then stores bytes instead of dwords and writes the same frames"""
    rng = np.random.default_rng(6600)
    streams = []
    for n, d in ((24, 0x13), (192, 0x6F), (1536, 0x51)):
        streams.append((n, [(d, [rng.integers(0, 256, l, dtype=np.uint8) for l in T.split_lengths(rng, d, n)]) for _ in range(2)]))
    stride = 1540
    offs = np.array([1, 10 * stride + 2, 20 * stride + 7], np.uint64)
    total = 30 * stride + 8
    got, st = run_encode(ctx, streams, offs, stride, total)
    exp, est = expected_image(streams, offs, stride, total)
    assert not st.any() and np.array_equal(got, exp)
