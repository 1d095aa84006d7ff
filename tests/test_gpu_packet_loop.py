"""-m gpu: a packet-mode data service through the whole chain on the device: data groups -> PacketTx into a TxBank payload (a 288 CU EEP 3-A
sub-channel, 1152 bytes per CIF, beside a DAB+ sub-channel filled by DabPlusTx) -> transmit_frames -> channel kernel ->
dabgpu_ofdm_sync_demod_frames -> dabgpu_decode_frames_layout -> PacketBank.  Six transmission frames = 24 CIFs, of which the time
interleaver hands back the first nine logical frames: four whole FEC frames.
Leg 1, clean channel: every row count 0, every packet's CRC good, every data group back.
Leg 2: a fixed pattern of 1..8 byte errors per row is XORed into the decoded sub-channel bytes on the device in front of the bank: the groups
are all back again and rs_count is the pattern.
(The leg with channel noise at a level found on the CPU is not here: DESIGN.md 4.21.)"""
import numpy as np
import pytest

import channel_model as CM
import dabplus_tx_model as T
import packet_fec_model as M
import tx_encode_cases as X

pytestmark = pytest.mark.gpu
SUBS = [dict(start=0, length=12, is_uep=0, uep_index=0, eep_level=2, eep_type=0),           # DAB+, 48 bytes per CIF
        dict(start=12, length=288, is_uep=0, uep_index=0, eep_level=2, eep_type=0)]         # packet mode with FEC, 1152 bytes per CIF
F, K, FB, ADDRESS, LENGTH = 6, 4, 1152, 0x155, 96
P = 700
STRIDE = P + 1544 + 196608


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype.fields is not None:
        a = a.view(np.uint8)
    return torch.from_numpy(a).cuda()


def test_data_groups_through_transmitter_channel_receiver_and_fec():
    import dabgpu
    import torch
    ctx = dabgpu.Context(0)
    rng = np.random.default_rng(8100)
    gsubs = [X.g_sub(dabgpu, d) for d in SUBS]
    bank = dabgpu.TxBank(ctx, 1, gsubs)
    nb = bank.cif_in_bytes
    assert nb == 48 + FB
    fib, pay = X.random_input(rng, 1, F, nb)
    pay = pay.reshape(1, 4 * F, nb).copy()
    pay[:, :, 48:] = 0                                 # behind the FEC frames the sub-channel carries zero bytes
    d_pay = dev(pay)
    # the packet-mode sub-channel: K FEC frames of seeded data groups
    lens = [int(x) for x in rng.integers(0, 500, 60)]
    groups = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
    st, table, first, consumed, end_start, _ = dabgpu.packet_tx_layout(lens, ADDRESS, LENGTH, FB, 0, 0, K)
    assert st == 0 and consumed >= 20 and end_start == K * M.RING
    offs, stride, fbytes = dabgpu.packet_tx_offsets(bank, [1], F)
    assert list(fbytes) == [FB] and stride == nb and list(offs) == [48]
    goffs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    tab = np.zeros((1, 94 * K), np.dtype(dabgpu.PACKET_TX_ENTRY_DTYPE))
    tab[0, :len(table)] = table
    status = torch.full((1, K), -7, dtype=torch.int32, device="cuda")
    dabgpu.PacketTx(ctx).encode(1, K, dev(np.concatenate(groups + [np.zeros(16, np.uint8)])), dev(goffs), dev(np.array([0, len(lens)], np.uint32)), dev(tab),
                                94 * K, dev(first.reshape(1, -1)), dev(np.array([ADDRESS], np.uint16)), dev(np.array([FB], np.uint32)),
                                dev(np.zeros(1, np.uint64)), d_pay, dev(offs), stride, status)
    # the DAB+ sub-channel beside it: four super frames in the first 20 CIFs
    sfs = []
    for k in range(4):
        d = (0x13, 0x3A, 0x51, 0x6F)[k]
        sfs.append((d, [rng.integers(0, 256, l, dtype=np.uint8) for l in T.split_lengths(rng, d, 48)]))
    au, au_offs, au_lens, desc, fb48 = T.pack_call([(48, sfs)])
    st_plus = torch.full((1, 4), -7, dtype=torch.int32, device="cuda")
    dabgpu.DabPlusTx(ctx).encode(1, 4, dev(au), dev(au_offs), dev(au_lens), dev(desc), dev(fb48), d_pay, dev(np.zeros(1, np.uint64)), nb, st_plus)
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any() and not st_plus.cpu().numpy().any()
    sent = d_pay.cpu().numpy().reshape(4 * F, nb)
    model_bytes = M.encode(groups, [dict(group=int(e["group"]), offset=int(e["offset"]), position=int(e["position"]), length=int(e["length"]),
                                         useful=int(e["useful"]), flags=int(e["flags"]), ci=int(e["continuity_index"])) for e in table],
                           [int(x) for x in first], ADDRESS)
    assert np.array_equal(sent[:, 48:].reshape(-1)[:K * M.RING], model_bytes) and not sent[:, 48:].reshape(-1)[K * M.RING:].any()
    # transmitter -> channel (one path, no noise) -> receiver
    S = dabgpu.NB_FRAME_SAMPLES
    d_iq = torch.zeros((F * S, 2), dtype=torch.float32, device="cuda")
    bank.transmit_frames(dev(fib), d_pay, F, d_iq)
    n_out = F * S + 4096
    ch = dabgpu.Channel(ctx, [CM.to_struct(CM.params_dict(taps=[(0, 1.0, 0.0)], freq_q64=0, start=0, seed=1, noise_sigma=0.0), dabgpu.ChannelStream)])
    d_rx = torch.zeros((n_out, 2), dtype=torch.float32, device="cuda")
    ch.apply(d_iq, F * S, n_out, d_rx)
    H = 8
    sdt, rdt = np.dtype(dabgpu.SYNC_STATE_DTYPE), np.dtype(dabgpu.RESULT_DTYPE)
    d_st = torch.zeros(sdt.itemsize, dtype=torch.uint8, device="cuda")
    hist = torch.zeros((1, H, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
    d_fib = torch.zeros((1, 4, 96), dtype=torch.uint8, device="cuda"); fres = torch.zeros((4, 16), dtype=torch.uint8, device="cuda")
    msc = torch.zeros((1, 4, nb), dtype=torch.uint8, device="cuda"); mres = torch.zeros((4 * len(gsubs), 16), dtype=torch.uint8, device="cuda")
    n_rx = 4 * F - 15
    d_cifs = torch.zeros((n_rx, nb), dtype=torch.uint8, device="cuda")       # the logical frames the time interleaver has handed back
    for j in range(F):
        a = 2656 + j * S - P
        d_slice = torch.zeros((1, STRIDE, 2), dtype=torch.float32, device="cuda")
        seg = d_rx[a:a + STRIDE]
        d_slice[0, :seg.shape[0]] = seg
        ctx.ofdm_sync_demod_frames(d_slice, 1, STRIDE, P, d_st, hist[:, j % H], bits_frame_stride=H * dabgpu.NB_FRAME_BITS)
        ctx.decode_frames(hist, 1, H * dabgpu.NB_FRAME_BITS, H, j % H, gsubs, d_fib, fres, msc, 4 * nb, mres)
        torch.cuda.synchronize()
        assert (fres.cpu().numpy().view(rdt)["crc_ok_mask"] == 7).all(), f"frame {j}: FIB CRCs"
        for c in range(4):
            if 4 * j + c >= 15:
                d_cifs[4 * j + c - 15].copy_(msc[0, c])
    rx = d_cifs.cpu().numpy()
    assert np.array_equal(rx, sent[:n_rx]), "sub-channel bytes differ from the transmitted ones"          # both sub-channels, the DAB+ one included
    assert n_rx * FB >= K * M.RING
    # the error pattern of leg 2: e(t, y) byte errors in row y of FEC frame t, 1..8, at symbols spread over data and parity; row 0's errors
    # stay off the length and address bits of byte 0 (packet_fec_model.damage_rows)
    pattern = [[1 + (3 * t + y) % 8 for y in range(12)] for t in range(K)]
    stream = np.zeros(n_rx * FB, np.uint8)
    for t in range(K):
        clean = np.zeros(M.RING, np.uint8)
        stream[t * M.RING:(t + 1) * M.RING] = M.damage_rows(np.random.default_rng(8200 + t), clean, pattern[t])
    flips = np.zeros((n_rx, nb), np.uint8)
    flips[:, 48:] = stream.reshape(n_rx, FB)
    assert int((stream != 0).sum()) == sum(map(sum, pattern))
    pb = dabgpu.PacketBank(ctx, 1)
    cap = M.RING + n_rx * FB
    rec_dt, fec_dt = np.dtype(dabgpu.PACKET_RECORD_DTYPE), np.dtype(dabgpu.PACKET_FEC_FRAME_DTYPE)
    for leg, want in ((1, [[0] * 12] * K), (2, pattern)):
        d_in = d_cifs if leg == 1 else torch.bitwise_xor(d_cifs, dev(flips))
        d_pk = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        d_rec = torch.zeros(600 * 16, dtype=torch.uint8, device="cuda")
        d_fec = torch.zeros(8 * 20, dtype=torch.uint8, device="cuda")
        d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
        pb.reset()
        pb.process(d_in, dev(np.array([48], np.uint64)), nb, dev(np.array([FB], np.uint32)), n_rx, d_pk, cap, d_rec, 600, d_fec, 8, d_cnt)
        torch.cuda.synchronize()
        cnt = d_cnt.cpu().numpy()
        rec, fec, pk = d_rec.cpu().numpy().view(rec_dt)[:cnt[0]], d_fec.cpu().numpy().view(fec_dt)[:cnt[2]], d_pk.cpu().numpy()
        assert cnt[2] == K and fec["rs_count"].tolist() == want, (leg, fec["rs_count"].tolist())
        assert cnt[0] == len(table) and rec["is_corrected"].all() and rec["crc_ok"].all(), leg
        assert np.array_equal(pk[:cnt[1]], np.concatenate([model_bytes[t * M.RING:t * M.RING + M.APP] for t in range(K)])), leg
        ra = M.Reassembler(ADDRESS)
        ra.last_ci = 3
        got = ra.feed(pk, [dict(offset=int(r["offset"]), length=int(r["length"])) for r in rec])
        assert got == [bytes(g) for g in groups[:consumed]], leg
    pb.close(); ch.close(); bank.close(); ctx.close()
