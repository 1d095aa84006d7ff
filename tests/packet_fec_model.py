"""Plain model of MSC packet mode with its FEC scheme (EN 300 401 clauses 5.3.2 and 5.3.5), independent of the library's sources: the
packet walk, the 2472-byte ring, the FEC-packet counter rules and the RS(204,188) row decoder as the reference's
MSC_Reed_Solomon_Data_Packet_Processor runs them, the packet CRC, and the transmit direction (packet layout of data groups, packets, parity,
FEC packets) that the reference does not have.  tests/golden/packet_fec_vectors.npz pins the receive half to the reference itself
(tests/golden/make_golden_packet_fec.py); the encoder's pin is that the reference's decoder returns 0 for every row of its output."""
import numpy as np

LENGTHS = (24, 48, 72, 96)
RS_K, RS_P, RS_N, ROWS, PAD = 188, 16, 204, 12, 51
APP, RING, FEC_ADDR, N_FEC = 2256, 2472, 0x3FE, 9

# ---- GF(2^8), p(x) = x^8 + x^4 + x^3 + x^2 + 1 ----
EXP = [0] * 512
LOG = [0] * 256
_x = 1
for _i in range(255):
    EXP[_i] = EXP[_i + 255] = _x
    LOG[_x] = _i
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x11D
EXP[510], EXP[511] = EXP[0], EXP[1]


def gmul(a, b):
    return EXP[LOG[a] + LOG[b]] if a and b else 0


def gdiv(a, b):
    return EXP[LOG[a] + 255 - LOG[b]] if a else 0


def gpow(e):
    return EXP[e % 255]


def poly_eval(p, x):
    """p[0] + p[1] x + ..."""
    v = 0
    for c in reversed(p):
        v = gmul(v, x) ^ c
    return v


def generator():
    g = [1]
    for r in range(RS_P):
        g = [0] + g                                   # times x
        for k in range(len(g) - 1):
            g[k] ^= gmul(g[k + 1], EXP[r])            # plus alpha^r times the old polynomial
    return g                                          # ascending powers, g[16] = 1


GEN = generator()


def rs_parity(data):
    """the 16 parity symbols of 188 data symbols: remainder of data(x) x^16 by g(x), highest power first (an LFSR, symbol by symbol)"""
    reg = [0] * RS_P                                  # reg[k] = coefficient of x^k
    for d in data:
        fb = int(d) ^ reg[RS_P - 1]
        for k in range(RS_P - 1, 0, -1):
            reg[k] = reg[k - 1] ^ gmul(fb, GEN[k])
        reg[0] = gmul(fb, GEN[0])
    return [reg[RS_P - 1 - r] for r in range(RS_P)]


_EXP_NP = np.array(EXP[:255], np.uint8)
_LOG_NP = np.array(LOG, np.int64)


def syndromes(word):
    """S_r = word(alpha^r), word[0] the highest power: the sum of the terms c_j alpha^(r (n - 1 - j)) over the non-zero symbols"""
    w = np.asarray(word, np.int64)
    nz = np.nonzero(w)[0]
    logs, e = _LOG_NP[w[nz]], len(w) - 1 - nz
    return [int(np.bitwise_xor.reduce(_EXP_NP[(logs + r * e) % 255])) if nz.size else 0 for r in range(RS_P)]


def rs_decode(word):
    """Karn's decoder as constructed (8, 0x11D, first root 0, primitive 1, 16 roots, padding 51), without erasures:
    -> (count, positions with the padding added -- in the order of the Chien search --, corrected word)"""
    word = [int(v) for v in word]
    S = syndromes(word)
    if not any(S):
        return 0, [], word
    lam = [1] + [0] * RS_P
    B = [1] + [0] * RS_P
    el = 0
    for r in range(1, RS_P + 1):
        d = 0
        for i in range(r):
            d ^= gmul(lam[i], S[r - 1 - i])
        if d == 0:
            B = [0] + B[:-1]
        else:
            T = [lam[0]] + [lam[i + 1] ^ gmul(d, B[i]) for i in range(RS_P)]
            if 2 * el <= r - 1:
                el = r - el
                B = [gdiv(c, d) for c in lam]
            else:
                B = [0] + B[:-1]
            lam = T
    deg = max(i for i in range(RS_P + 1) if lam[i])
    roots, locs = [], []
    for i in range(1, 256):                           # candidate alpha^i; location i - 1
        if poly_eval(lam[:deg + 1], EXP[i % 255]) == 0:
            roots.append(i)
            locs.append(i - 1)
            if len(roots) == deg:
                break
    if len(roots) != deg:
        return -1, [], word
    omega = []
    for i in range(deg):
        t = 0
        for j in range(i + 1):
            t ^= gmul(S[i - j], lam[j])
        omega.append(t)
    out = list(word)
    for root, loc in zip(roots, locs):
        num1 = 0
        for i, o in enumerate(omega):
            num1 ^= gmul(o, gpow(i * root))
        num2 = gpow(255 - root)
        den = 0
        for i in range(0, min(deg, RS_P - 1) + 1, 2):
            den ^= gmul(lam[i + 1], gpow(i * root)) if i + 1 <= RS_P else 0
        if num1 != 0 and loc >= PAD:
            out[loc - PAD] ^= gdiv(gmul(num1, num2), den) if den else gmul(num1, num2)
    return deg, locs, out


# ---- packet CRC ----
def crc16(data):
    c = 0xFFFF
    for b in data:
        c ^= int(b) << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x1021) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c ^ 0xFFFF


def packet_crc_ok(p):
    return crc16(p[:-2]) == (int(p[-2]) << 8 | int(p[-1]))


def record_of(p, corrected):
    """the fields the device records per packet handed out"""
    b0, b1, b2 = int(p[0]), int(p[1]), int(p[2])
    return dict(length=len(p), address=((b0 & 3) << 8) | b1, continuity_index=(b0 >> 4) & 3, first_last=(b0 >> 2) & 3, command=b2 >> 7,
                useful_length=b2 & 0x7F, is_corrected=int(corrected), crc_ok=int(packet_crc_ok(p)))


# ---- receive: MSC_Reed_Solomon_Data_Packet_Processor ----
def row_offsets():
    """[12][204] byte offsets behind the ring's read head of the symbols of every row"""
    m = np.zeros((ROWS, RS_N), np.int64)
    for y in range(ROWS):
        for i in range(RS_K):
            m[y, i] = i * ROWS + y
        for i in range(RS_P):
            t = i * ROWS + y
            m[y, RS_K + i] = APP + (t // 22) * 24 + 2 + t % 22
    return m


ROW_OFFSETS = row_offsets()


class Processor:
    def __init__(self):
        self.ring = np.zeros(RING, np.uint8)
        self.read = self.write = self.size = 0
        self.last = None
        self.log = []                                 # (packet bytes, is_corrected) in callback order
        self.fec_frames = []                          # (index of the frame's first packet in log, [12 counts])
        self.discarded = 0                            # packets dropped without callback, over the processor's life
        self.trace = []

    def _pop(self):
        if self.size == 0:
            return None
        n = LENGTHS[self.ring[self.read] >> 6]
        p = self.ring[(self.read + np.arange(n)) % RING].copy()
        self.size -= n
        self.read = (self.read + n) % RING
        return p

    def _clear(self):
        while True:
            p = self._pop()
            if p is None:
                break
            self.log.append((p, False))

    def _push(self, packet, length_id):
        n = LENGTHS[length_id]
        while RING - self.size < n:
            other = LENGTHS[self.ring[self.read] >> 6]
            self.size -= other
            self.read = (self.read + other) % RING
            self.discarded += 1
        idx = (self.write + np.arange(n)) % RING
        self.ring[idx] = packet
        self.ring[self.write] = (int(packet[0]) & 0x3F) | (length_id << 6)
        self.size += n
        self.write = (self.write + n) % RING

    def _correct(self):
        counts = []
        for y in range(ROWS):
            idx = (self.read + ROW_OFFSETS[y]) % RING
            count, locs, fixed = rs_decode(self.ring[idx])
            counts.append(count)
            if count < 0:
                continue
            for loc in locs:
                x = loc - PAD
                if 0 <= x < RS_K:
                    self.ring[idx[x]] = fixed[x]
        self.fec_frames.append((len(self.log), counts))
        total = 0
        while total < APP:
            p = self._pop()
            if p is None:
                break
            self.log.append((p, True))
            total += len(p)

    def read_packet(self, buf):
        """-> bytes consumed; appends (consumed, stored, is_fec, ring fill, read head, event) to self.trace, event 1 = everything handed
        out uncorrected, 2 = frame corrected"""
        n, stored, fec, event = self._read_packet(buf)
        self.trace.append((n, int(stored), int(fec), self.size, self.read, event))
        return n

    def _read_packet(self, buf):
        if len(buf) < 2:
            return len(buf), False, False, 0
        b0, b1 = int(buf[0]), int(buf[1])
        length_id, counter, address = b0 >> 6, (b0 >> 2) & 15, ((b0 & 3) << 8) | b1
        fec = address == FEC_ADDR
        if fec:
            length_id = 0
        n = LENGTHS[length_id]
        if len(buf) < n:
            return len(buf), False, False, 0
        self._push(np.asarray(buf[:n], np.uint8), length_id)
        if not fec:
            return n, True, False, 0
        invalid = (self.last + 1 != counter) if self.last is not None else (counter != 0)
        if invalid:
            self.last = None
            self._clear()
            return n, True, True, 1
        self.last = counter
        if counter != N_FEC - 1:
            return n, True, True, 0
        if self.size != RING:
            self._clear()
            event = 1
        else:
            self._correct()
            event = 2
        self.last = None
        self.read = self.write = self.size = 0
        return n, True, True, event

    def read_buffer(self, buf):
        """Basic_Data_Packet_Channel::ProcessFECPackets over one logical frame -> the ReadPacket return values"""
        buf = np.asarray(buf, np.uint8)
        at, used = 0, []
        while at < len(buf):
            n = self.read_packet(buf[at:])
            used.append(n)
            at += n
        return used


def run_frames(frames, proc=None):
    """frames: iterable of uint8 arrays (logical frames) -> dict of what a bank call over them reports for the stream"""
    proc = proc or Processor()
    n0, f0, d0 = len(proc.log), len(proc.fec_frames), proc.discarded
    fec_frame_index = []
    for f, frame in enumerate(frames):
        before = len(proc.fec_frames)
        proc.read_buffer(frame)
        fec_frame_index += [f] * (len(proc.fec_frames) - before)
    log = proc.log[n0:]
    packets = np.concatenate([p for p, _ in log]) if log else np.zeros(0, np.uint8)
    records, off = [], 0
    for p, c in log:
        r = record_of(p, c)
        r["offset"] = off
        off += len(p)
        records.append(r)
    fec = [dict(frame_index=fi, first_record=first - n0, rs_count=list(cnt)) for fi, (first, cnt) in zip(fec_frame_index, proc.fec_frames[f0:])]
    return dict(packets=packets, records=records, fec_frames=fec, counts=[len(log), int(packets.size), len(fec), proc.discarded - d0], proc=proc)


# ---- transmit ----
BAD_ADDRESS, BAD_LENGTH, BAD_FRAME_BYTES, FRAME_TOO_SMALL, BAD_GROUP, BAD_START, BAD_TABLE = 1, 2, 3, 4, 5, 6, 7


def layout(group_len, address, length, frame_bytes, start_byte=0, ci=0, n_fec_frames=1):
    """-> (status, entries, frame_first, groups consumed, end start_byte, end continuity index); an entry is a dict of group (-1 padding),
    offset, position (from the start of the call), length, useful, flags (bit 1 first, bit 0 last), ci"""
    if not 1 <= address <= 1021:
        return BAD_ADDRESS, [], [], 0, start_byte, ci
    if length not in LENGTHS:
        return BAD_LENGTH, [], [], 0, start_byte, ci
    if frame_bytes == 0 or frame_bytes % 24:
        return BAD_FRAME_BYTES, [], [], 0, start_byte, ci
    if frame_bytes < length:
        return FRAME_TOO_SMALL, [], [], 0, start_byte, ci
    if any(g > 8191 for g in group_len):
        return BAD_GROUP, [], [], 0, start_byte, ci
    if start_byte % 24:
        return BAD_START, [], [], 0, start_byte, ci
    entries, first = [], [0]
    t, used, ci = 0, 0, ci & 3

    def fits(n):
        at = start_byte + t * RING + used
        return used + n <= APP and at % frame_bytes + n <= frame_bytes

    def place(group, offset, n, useful, flags, c):
        nonlocal t, used
        entries.append(dict(group=group, offset=offset, position=t * RING + used, length=n, useful=useful, flags=flags, ci=c))
        used += n
        if used == APP:
            t, used = t + 1, 0
            first.append(len(entries))
    consumed = 0
    for g, glen in enumerate(group_len):
        if t >= n_fec_frames:
            break
        keep = (len(entries), len(first), t, used, ci)
        done, begun, whole = 0, False, False
        while t < n_fec_frames:
            if not fits(length):
                place(-1, 0, 24, 0, 0, 0)
                continue
            take = min(glen - done, length - 5)
            last = take == glen - done
            place(g, done, length, take, (0 if begun else 2) | (1 if last else 0), ci)
            ci = (ci + 1) & 3
            done += take
            begun = True
            if last:
                whole = True
                break
        if not whole:
            del entries[keep[0]:]
            del first[keep[1]:]
            t, used, ci = keep[2], keep[3], keep[4]
            break
        consumed = g + 1
    while t < n_fec_frames:
        place(-1, 0, 24, 0, 0, 0)
    return 0, entries, first, consumed, start_byte + n_fec_frames * RING, ci


def build_packet(e, groups, address):
    n = e["length"]
    a = address if e["group"] >= 0 else 0
    p = np.zeros(n, np.uint8)
    p[0] = ((n // 24 - 1) << 6) | (e["ci"] << 4) | (e["flags"] << 2) | (a >> 8)
    p[1] = a & 0xFF
    p[2] = e["useful"]
    if e["useful"]:
        p[3:3 + e["useful"]] = np.frombuffer(bytes(groups[e["group"]]), np.uint8)[e["offset"]:e["offset"] + e["useful"]]
    c = crc16(p[:-2])
    p[-2], p[-1] = c >> 8, c & 0xFF
    return p


def fec_packets(app):
    """the nine FEC packets behind 2256 application bytes"""
    app = np.asarray(app, np.uint8)
    table = np.zeros(RS_P * ROWS, np.uint8)
    for y in range(ROWS):
        par = rs_parity(app[y::ROWS])
        for i in range(RS_P):
            table[i * ROWS + y] = par[i]
    out = np.zeros(N_FEC * 24, np.uint8)
    padded = np.concatenate([table, np.zeros(6, np.uint8)])
    for m in range(N_FEC):
        out[24 * m] = (m << 2) | (FEC_ADDR >> 8)
        out[24 * m + 1] = FEC_ADDR & 0xFF
        out[24 * m + 2:24 * m + 24] = padded[22 * m:22 * m + 22]
    return out


def encode(groups, entries, frame_first, address):
    """-> uint8 [n_fec_frames * 2472]: the stream bytes of the call"""
    K = len(frame_first) - 1
    out = np.zeros(K * RING, np.uint8)
    for t in range(K):
        for e in entries[frame_first[t]:frame_first[t + 1]]:
            out[e["position"]:e["position"] + e["length"]] = build_packet(e, groups, address)
        out[t * RING + APP:(t + 1) * RING] = fec_packets(out[t * RING:t * RING + APP])
    return out


def padding_frame():
    """what a refused FEC frame is written as: 94 padding packets and their FEC packets"""
    ent = [dict(group=-1, offset=0, position=24 * i, length=24, useful=0, flags=0, ci=0) for i in range(94)]
    return encode([], ent, [0, 94], 1)


def to_logical_frames(stream_bytes, frame_bytes, start_byte=0, fill=0):
    """the call's bytes through the logical-frame mapping -> uint8 [n_frames][frame_bytes] (bytes the call does not write = fill)"""
    lead = start_byte % frame_bytes
    n = (lead + len(stream_bytes) + frame_bytes - 1) // frame_bytes
    flat = np.full(n * frame_bytes, fill, np.uint8)
    flat[lead:lead + len(stream_bytes)] = stream_bytes
    return flat.reshape(n, frame_bytes)


def rx_buffers(stream_bytes, frame_bytes, start_byte=0):
    """the call's bytes as the receiver meets them: cut at the logical-frame boundaries (the first buffer is the rest of the frame that
    holds start_byte)"""
    cuts = [0] + list(range(frame_bytes - start_byte % frame_bytes, len(stream_bytes), frame_bytes)) + [len(stream_bytes)]
    return [stream_bytes[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


class Reassembler:
    """test-side MSC_Data_Packet_Processor (msc_data_packet_processor.cpp:52-133) up to the data groups"""

    def __init__(self, address):
        self.address, self.last_ci, self.buf, self.groups = address, 0, None, []

    def packet(self, p):
        b0 = int(p[0])
        if (((b0 & 3) << 8) | int(p[1])) != self.address:
            return
        useful = int(p[2]) & 0x7F
        if useful > len(p) - 5 or not packet_crc_ok(p):
            return
        ci, fl = (b0 >> 4) & 3, (b0 >> 2) & 3
        ok = ((self.last_ci + 1) & 3) == ci
        self.last_ci = ci
        piece = bytes(p[3:3 + useful])
        if fl == 3:
            self.groups.append(piece)
        elif fl == 2:
            self.buf = piece
        elif self.buf is None or not ok:
            self.buf = None
        elif fl == 0:
            self.buf += piece
        else:
            self.groups.append(self.buf + piece)
            self.buf = None

    def feed(self, packets, records):
        for r in records:
            self.packet(packets[r["offset"]:r["offset"] + r["length"]])
        return self.groups


def pack_tx_call(streams):
    """streams: [(groups, entries, frame_first)] -> the device call's arrays (data, group_offsets, group_base, table [S][94 K], frame_first [S][K + 1])"""
    import dabgpu
    K = len(streams[0][2]) - 1
    dt = np.dtype(dabgpu.PACKET_TX_ENTRY_DTYPE)
    table = np.zeros((len(streams), 94 * K), dt)
    first = np.zeros((len(streams), K + 1), np.uint32)
    blob, offs, base = [], [0], [0]
    for s, (groups, entries, ff) in enumerate(streams):
        for g in groups:
            blob.append(np.asarray(g, np.uint8))
            offs.append(offs[-1] + len(g))
        base.append(len(offs) - 1)
        for i, e in enumerate(entries):
            table[s, i] = (e["group"], e["offset"], e["position"], e["length"], e["useful"], e["flags"], e["ci"])
        first[s, :len(ff)] = ff
    data = np.concatenate(blob + [np.zeros(16, np.uint8)])
    return data, np.array(offs, np.uint64), np.array(base, np.uint32), table, first


# ---- inputs of tests/golden/packet_fec_vectors.npz (make_golden_packet_fec.py) and of the device tests ----
def random_fec_frame(rng, lengths=LENGTHS, max_useful=6):
    """one FEC frame (2472 bytes) of random packets with addresses 1..767 (never the FEC address, whatever happens to the low byte), short
    useful fields (the rest is zero padding: the fixture compresses) and valid CRCs -> (bytes, packet starts)"""
    app, at, starts, ci = np.zeros(APP, np.uint8), 0, [], 0
    while at < APP:
        n = int(rng.choice([v for v in lengths if at + v <= APP] or [24]))
        a, useful = int(rng.integers(1, 768)), int(rng.integers(0, max_useful + 1))
        p = np.zeros(n, np.uint8)
        p[0] = ((n // 24 - 1) << 6) | (ci << 4) | (int(rng.integers(0, 4)) << 2) | (a >> 8)
        p[1], p[2] = a & 0xFF, useful
        p[3:3 + useful] = rng.integers(0, 256, useful)
        c = crc16(p[:-2])
        p[-2], p[-1] = c >> 8, c & 0xFF
        app[at:at + n] = p
        starts.append(at)
        at, ci = at + n, (ci + 1) & 3
    return np.concatenate([app, fec_packets(app)]), starts


def damage_rows(rng, frame, errs, where="any"):
    """errs[y] symbol errors in row y of a 2472-byte frame; where = any / data / parity.  Errors on row 0's data symbols (byte 0 of every
    packet lies there) only touch bits 2..5: the length and address fields stay, so the walk does"""
    frame = frame.copy()
    cols = dict(any=np.arange(RS_N), data=np.arange(RS_K), parity=np.arange(RS_K, RS_N))[where]
    for y, e in enumerate(errs):
        for x in rng.choice(cols, min(e, len(cols)), replace=False):
            v = int(rng.integers(1, 16)) << 2 if (y == 0 and x < RS_K) else int(rng.integers(1, 256))
            frame[ROW_OFFSETS[y, x]] ^= v
    return frame


def golden_sequences(seed=7100):
    """-> (names, [list of buffers])"""
    rng = np.random.default_rng(seed)
    out = []

    def add(name, bufs):
        out.append((name, [np.asarray(b, np.uint8) for b in bufs]))
    add("clean_mixed", [random_fec_frame(rng)[0], random_fec_frame(rng)[0]])
    add("errors_1_to_8", [damage_rows(rng, random_fec_frame(rng)[0], [1, 2, 3, 4, 5, 6, 7, 8, 1, 2, 3, 4])])
    add("errors_9_plus", [damage_rows(rng, random_fec_frame(rng)[0], [0, 9, 10, 12, 2, 0, 8, 16, 1, 0, 11, 3])])
    add("errors_fec_only", [damage_rows(rng, random_fec_frame(rng)[0], [3] * 12, "parity")])
    f = random_fec_frame(rng)[0]
    f[APP + 4 * 24] |= 0x80
    f[APP + 7 * 24] |= 0xC0
    add("fec_length_field", [f])
    f = random_fec_frame(rng, (24,))[0]
    f[10 * 24] ^= 0x40                                # 24 -> 48: the walk swallows the next packet; row 0 puts it right before the pop walk
    add("data_length_longer", [f])
    f = random_fec_frame(rng, (48,))[0]
    f[5 * 48] ^= 0x40                                 # 48 -> 24: the walk goes on inside the packet's body
    add("data_length_shorter", [f])
    f = random_fec_frame(rng, (24,))[0]
    f[20 * 24] ^= 0x40
    f = damage_rows(rng, f, [10] + [1] * 11, "data")  # row 0 stays uncorrectable: the wrong length header is still there at the pop walk
    add("uncorrectable_row0_wrong_header", [f])
    f, _ = random_fec_frame(rng, (24,))
    other = f[:APP].copy()
    other[APP - 24] |= 0xC0                           # parity of a frame whose LAST header says 96: row 0 "corrects" the received 24 into it and
    f[APP:] = fec_packets(other)                      # the pop walk runs 72 bytes into the FEC packets; row 5 is left uncorrectable
    add("pop_into_fec_region", [damage_rows(rng, f, [0, 0, 0, 0, 0, 12, 0, 0, 0, 0, 0, 0], "data")])
    f, g = random_fec_frame(rng)[0], random_fec_frame(rng)[0]
    add("counter_skipped", [np.concatenate([f[:APP + 4 * 24], f[APP + 5 * 24:]]), g])
    f, g = random_fec_frame(rng)[0], random_fec_frame(rng)[0]
    add("counter_repeated", [np.concatenate([f[:APP + 3 * 24], f[APP + 2 * 24:]]), g])
    f, g = random_fec_frame(rng)[0], random_fec_frame(rng)[0]
    add("counter_starts_at_3", [f[APP + 3 * 24:], g])
    f, g = random_fec_frame(rng)[0], random_fec_frame(rng)[0]
    add("starts_mid_frame_short_ring", [f[APP - 40 * 24:], g])
    junk = np.concatenate([random_fec_frame(rng, (24,))[0][:APP], random_fec_frame(rng, (24,))[0][:36 * 24]])
    add("starts_mid_frame_discards", [junk, damage_rows(rng, random_fec_frame(rng)[0], [2] * 12)])
    f, g = random_fec_frame(rng)[0], random_fec_frame(rng)[0]
    add("ends_in_1_byte", [np.concatenate([f, [0x55]]), g])
    s = np.concatenate([random_fec_frame(rng)[0], random_fec_frame(rng)[0]])
    add("ends_in_truncated_packet", [s[:1007], s[1007:]])
    groups = [rng.integers(0, 256, int(n), dtype=np.uint8) for n in (0, 5, 40, 300, 91, 44, 1)]
    st, ent, first, consumed, _, _ = layout([len(x) for x in groups], 0x155, 48, 96, 0, 1, 2)
    assert st == 0 and consumed == len(groups)
    s = encode(groups, ent, first, 0x155)
    s[RING:] = damage_rows(rng, s[RING:], [4] * 12)
    add("layout_48_in_96", list(to_logical_frames(s, 96)))
    return [n for n, _ in out], [b for _, b in out]


def golden_rs_words(seed=7200):
    """-> (words [N][204], kinds [N])"""
    rng = np.random.default_rng(seed)
    words, kinds = [], []

    def codeword():
        data = np.zeros(RS_K, np.uint8)
        k = int(rng.integers(0, 31))
        data[rng.choice(RS_K, k, replace=False)] = rng.integers(1, 256, k)
        return np.concatenate([data, np.array(rs_parity(data), np.uint8)])

    def hurt(w, e, cols):
        for x in rng.choice(cols, e, replace=False):
            w[x] ^= int(rng.integers(1, 256))
        return w
    for e in range(11):
        for _ in range(24):
            words.append(hurt(codeword(), e, np.arange(RS_N)))
            kinds.append(f"errors_{e}")
    for _ in range(12):
        words.append(rng.integers(0, 256, RS_N, dtype=np.uint8))
        kinds.append("random")
    for k in range(12):
        words.append(hurt(codeword(), 1 + k % 8, np.arange(RS_K, RS_N)))
        kinds.append("parity_only")
    for k in range(8):
        # the full-length code word whose only non-zero data symbol sits in the padding, received with that symbol (never sent) as zero: the
        # decoder finds it at a position below 51 and reports it without applying it
        full = [0] * (RS_K + PAD)
        full[int(rng.integers(0, PAD))] = int(rng.integers(1, 256))
        w = np.concatenate([np.zeros(RS_K, np.uint8), np.array(rs_parity(full), np.uint8)])
        words.append(hurt(w, k, np.arange(RS_K)))
        kinds.append("padding_position")
    return words, kinds


def parse_log(log):
    """the fixture's callback log -> [(packet bytes, flag)]"""
    out, at = [], 0
    while at < len(log):
        flag, n = int(log[at]), int(np.asarray(log[at + 1:at + 5], np.uint8).view("<u4")[0])
        out.append((np.asarray(log[at + 5:at + 5 + n], np.uint8), bool(flag)))
        at += 5 + n
    return out


def apply_patterns(frame, rows):
    """XOR error patterns (204 symbols each, 0 = the row's first data byte) onto rows of a 2472-byte FEC frame: rows = {row: pattern} or a
    list of 12 patterns (None: the row stays) -> a damaged copy"""
    frame = np.array(frame, np.uint8)
    items = rows.items() if isinstance(rows, dict) else [(y, p) for y, p in enumerate(rows) if p is not None]
    for y, p in items:
        p = np.asarray(p, np.uint8)
        assert p.shape == (RS_N,)
        frame[ROW_OFFSETS[y]] ^= p
    return frame
