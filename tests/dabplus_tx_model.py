"""Test infrastructure: numpy model of the DAB+ super-frame ENCODER, written from ETSI TS 102 563 (clauses 5.2, 5.3.2 and 6) with its own
GF(2^8) arithmetic, fire code and CRC -- nothing of it comes from the oracle, which tests/test_dabplus_tx_model.py compares it with.
It takes what the device entry point takes (descriptor, access-unit payloads, bytes per logical frame) and returns what that writes:
the five logical frames and the status word (include/dabgpu.h, "DAB+ super-frame encoder")."""
import numpy as np

MAX_FRAME_BYTES = 1536
STATUS_OK, STATUS_FRAME_SIZE, STATUS_FILL, STATUS_START_FIELD = 0, 1, 2, 3

# ---- GF(2^8), p(x) = x^8 + x^4 + x^3 + x^2 + 1 (TS 102 563 clause 6.1) ----
GF_EXP = np.zeros(510, np.int64)
GF_LOG = np.zeros(256, np.int64)
_x = 1
for _i in range(255):
    GF_EXP[_i] = GF_EXP[_i + 255] = _x
    GF_LOG[_x] = _i
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x11D


def gf_mul(a, b):
    return 0 if a == 0 or b == 0 else int(GF_EXP[GF_LOG[a] + GF_LOG[b]])


def rs_generator():
    """g(x) = prod_{r = 0..9} (x + alpha^r), coefficients highest power first (11 of them, g[0] = 1)"""
    g = [1]
    for r in range(10):
        root = int(GF_EXP[r])
        g = [a ^ gf_mul(b, root) for a, b in zip(g + [0], [0] + g)]
    return g


RS_GEN = rs_generator()


def rs_parity(data110):
    """the ten parity bytes of RS(120,110) = RS(255,245) shortened by 135: remainder of d(x) x^10 by g(x), highest power first"""
    rem = [0] * 10
    for d in data110:
        fb = int(d) ^ rem[0]
        rem = rem[1:] + [0]
        if fb:
            for k in range(10):
                rem[k] ^= gf_mul(fb, RS_GEN[k + 1])
    return np.array(rem, np.uint8)


def firecode(data9):
    """x^16 + x^14 + x^13 + x^12 + x^11 + x^5 + x^3 + x^2 + x + 1 over the 72 bits of bytes 2..10, zero start value, MSB first (clause 5.2)"""
    reg = 0
    for b in data9:
        for k in range(7, -1, -1):
            top = ((reg >> 15) & 1) ^ ((int(b) >> k) & 1)
            reg = (reg << 1) & 0xFFFF
            if top:
                reg ^= 0x782F
    return reg


def au_crc(payload):
    """CRC-16-CCITT x^16 + x^12 + x^5 + 1, start value 0xFFFF, result inverted, MSB first (clause 5.3.2)"""
    reg = 0xFFFF
    for b in payload:
        for k in range(7, -1, -1):
            top = ((reg >> 15) & 1) ^ ((int(b) >> k) & 1)
            reg = (reg << 1) & 0xFFFF
            if top:
                reg ^= 0x1021
    return reg ^ 0xFFFF


def num_aus_of(descriptor):
    dac_rate, sbr_flag = (descriptor >> 6) & 1, (descriptor >> 5) & 1
    return {(0, 1): 2, (1, 1): 3, (0, 0): 4, (1, 0): 6}[(dac_rate, sbr_flag)]


def layout(frame_bytes, descriptor, au_len):
    """-> (status, au_start[7] (zeros behind num_aus), num_aus, n_rs); au_len: at least num_aus lengths"""
    if frame_bytes < 24 or frame_bytes > MAX_FRAME_BYTES or frame_bytes % 24:
        return STATUS_FRAME_SIZE, None, 0, 0
    n_rs = frame_bytes // 24
    na = num_aus_of(descriptor)
    start = [3 + (12 * (na - 1) + 7) // 8]
    for i in range(na):
        start.append(start[-1] + int(au_len[i]) + 2)
    if start[na] != 110 * n_rs:
        return STATUS_FILL, None, na, n_rs
    if any(s > 4095 for s in start[1:na]):
        return STATUS_START_FIELD, None, na, n_rs
    return STATUS_OK, start + [0] * (6 - na), na, n_rs


def encode(descriptor, aus, frame_bytes):
    """-> (uint8[5 * frame_bytes] = the five logical frames back to back, status); a super frame that is refused gives zeros"""
    status, start, na, n_rs = layout(frame_bytes, descriptor, [len(a) for a in aus] + [0] * 6)
    if status:
        return np.zeros(5 * frame_bytes, np.uint8), status
    sf = np.zeros(120 * n_rs, np.uint8)
    sf[2] = descriptor
    bits = []
    for v in start[1:na]:
        bits += [(v >> (11 - b)) & 1 for b in range(12)]
    bits += [0] * (8 * (start[0] - 3) - len(bits))
    sf[3:start[0]] = np.packbits(np.array(bits, np.uint8))
    for i in range(na):
        a, n = start[i], len(aus[i])
        sf[a:a + n] = np.asarray(aus[i], np.uint8)
        crc = au_crc(aus[i])
        sf[a + n], sf[a + n + 1] = crc >> 8, crc & 0xFF
    fc = firecode(sf[2:11])
    sf[0], sf[1] = fc >> 8, fc & 0xFF
    for i in range(n_rs):
        sf[i + 110 * n_rs::n_rs] = rs_parity(sf[i:i + 110 * n_rs:n_rs])
    return sf, STATUS_OK


def split_lengths(rng, descriptor, frame_bytes, shape="random"):
    """access-unit lengths that fill a super frame: "random", "first_big" (one unit takes nearly all the room), "zeros" (every unit but the
    last is empty)"""
    na, n_rs = num_aus_of(descriptor), frame_bytes // 24
    room = 110 * n_rs - (3 + (12 * (na - 1) + 7) // 8) - 2 * na
    assert room >= 0
    if shape == "first_big":
        rest = [int(rng.integers(0, 2)) for _ in range(na - 1)]
        rest = rest if sum(rest) <= room else [0] * (na - 1)
        return [room - sum(rest)] + rest
    if shape == "zeros":
        return [0] * (na - 1) + [room]
    # every start but the last has to fit its 12-bit header field: from 38 code words on not every split does
    cuts = np.sort(rng.integers(0, min(room, 4095 - 11 - 2 * na) + 1, na - 1))
    return [int(v) for v in np.diff(np.concatenate([[0], cuts, [room]]))]


def pack_call(cases):
    """cases: list (streams) of (frame_bytes, [(descriptor, aus), ...]) with the same number of super frames each -> the arrays of one
    dabgpu_dabplus_tx_encode call: au_bytes, au_offsets [S][K], au_len [S][K][6], descriptor [S][K], frame_bytes [S]"""
    S, K = len(cases), len(cases[0][1])
    blob, off = [], 0
    au_offsets = np.zeros((S, K), np.uint64)
    au_len = np.zeros((S, K, 6), np.uint16)
    desc = np.zeros((S, K), np.uint8)
    fbytes = np.zeros(S, np.uint32)
    for s, (n, sfs) in enumerate(cases):
        assert len(sfs) == K
        fbytes[s] = n
        for k, (d, aus) in enumerate(sfs):
            desc[s, k] = d
            au_offsets[s, k] = off
            for a, p in enumerate(aus):
                au_len[s, k, a] = len(p)
                blob.append(np.asarray(p, np.uint8))
                off += len(p)
    au_bytes = np.concatenate(blob + [np.zeros(4, np.uint8)]) if blob else np.zeros(4, np.uint8)
    return au_bytes, au_offsets, au_len, desc, fbytes
