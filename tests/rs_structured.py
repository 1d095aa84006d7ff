"""Structured error patterns for the two Reed-Solomon codes the device decodes: RS(120,110) (DAB+, padding 135, t = 5) and RS(204,188)
(packet mode, padding 51, t = 8), both over GF(2^8) with p(x) = x^8+x^4+x^3+x^2+1 and first root alpha^0.  Plain numpy, nothing of the
library, nothing of the oracle.  words(code) is deterministic: the same patterns on every call, on every machine.

A pattern is an ERROR pattern: N symbols to be XORed onto a valid code word (the all-zero word included).  The code is linear, so the
decoder's count, the positions it reports and the values it applies depend on the pattern alone; tests/golden/rs_structured_vectors.npz
records what the reference's own decoder answers for every pattern (tests/golden/make_golden_rs_structured.py).

Families (the part of a kind before the colon), built in closed form so that the cases no random draw reaches are there:
  single        one error at every position 0..N-1, values cycling 0x01, 0x80, 0xFF: every share of every lane-dealt Chien search and every
                seam between two shares holds a root once
  exactly_t     t errors: at the word's start, at its end, inside the parity, straddling data|parity, on both sides of the seams between
                the shares of the device's searches, with one value, and 8 seeded random placements
  beyond_t      t + 1 errors (8), ROOTS errors (4), more (4), all-random words (4)
  miscorrect    t + 1 of the ROOTS + 1 non-zero symbols of a unit message's code word: t away from THAT code word, so the decoder lands on it
  padding_root  the parity of a full-length unit message in the padding, with m - 1 of its symbols removed (m = 1..t): the decoder finds one
                root inside the padding, which it counts and does not apply, and m - 1 real ones
  degenerate    two errors of one value (S_0 = 0: the first discrepancy is zero); three errors whose locators add up to zero (sigma_1 = 0, a
                zero inner coefficient of the locator polynomial); t errors whose locator has two zero inner coefficients; one error alone;
                and the zero pattern (count 0)
"""
import numpy as np

CODES = {120: dict(N=120, K=110, ROOTS=10, T=5, PAD=135), 204: dict(N=204, K=188, ROOTS=16, T=8, PAD=51)}
# lanes per code word of the DAB+ kernel's Chien search, 64 // n_rs for the numbers of code words per super frame the device tests use
# (with 2 lanes the one seam lies inside the padding, with 1 there is none: only padding_root reaches across the former)
DAB_PER = (64, 32, 21, 12, 8, 2, 1)

EXP = np.zeros(512, np.uint8)
LOG = np.zeros(256, np.int64)
_x = 1
for _i in range(255):
    EXP[_i] = EXP[_i + 255] = _x
    LOG[_x] = _i
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x11D
EXP[510], EXP[511] = EXP[0], EXP[1]


_E, _L = EXP.tolist(), LOG.tolist()


def _mul(a, b):
    return _E[_L[a] + _L[b]] if a and b else 0


def gmul(a, b):
    """element-wise product of two uint8 arrays (or scalars)"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.where((a != 0) & (b != 0), EXP[LOG[a] + LOG[b]], 0).astype(np.uint8)


MUL = gmul(np.arange(256)[:, None], np.arange(256)[None, :])       # the whole multiplication table, [a][b]


def generator(roots):
    """g(x) = prod (x + alpha^r), r = 0..roots-1, ascending powers"""
    g = [1]
    for r in range(roots):
        g = [0] + g
        for k in range(len(g) - 1):
            g[k] ^= _mul(g[k + 1], _E[r])
    return g


def parity_matrix(n_data, roots):
    """[n_data][roots]: row j = x^(n_data + roots - 1 - j) mod g(x), highest power first -- the parity symbols of the unit message at j"""
    g = generator(roots)
    rem = list(g[:roots])                               # x^roots mod g
    rows = [None] * n_data
    for j in range(n_data - 1, -1, -1):
        rows[j] = rem[::-1]
        top = rem[-1]
        rem = [_mul(top, g[0])] + [rem[k - 1] ^ _mul(top, g[k]) for k in range(1, roots)]
    return np.array(rows, np.uint8)


_PM = {}


def _pm(code):
    """parity matrix of the unshortened code's 255 - ROOTS message symbols; rows PAD.. are the shortened code's"""
    if code not in _PM:
        _PM[code] = parity_matrix(255 - CODES[code]["ROOTS"], CODES[code]["ROOTS"])
    return _PM[code]


def encode(code, data):
    """data uint8 [n][K] (or [K]) -> code words [n][N]: the data and its parity"""
    c = CODES[code]
    d = np.atleast_2d(np.asarray(data, np.uint8))
    assert d.shape[1] == c["K"]
    pm = _pm(code)[c["PAD"]:]
    par = np.bitwise_xor.reduce(MUL[d[:, :, None], pm[None, :, :]], axis=1)
    return np.concatenate([d, par], axis=1)


def locator_of(code, positions):
    """coefficients sigma_0..sigma_e of prod (1 + X_i x), X_i = alpha^(N - 1 - position_i): what Berlekamp-Massey finds for errors there"""
    N = CODES[code]["N"]
    sig = [1]
    for p in positions:
        X = _E[(N - 1 - int(p)) % 255]
        nxt = sig + [0]
        for k in range(len(sig)):
            nxt[k + 1] ^= _mul(sig[k], X)
        sig = nxt
    return sig


def dab_seams(per):
    """word positions p such that p - 1 and p lie in different lanes' shares of the DAB+ kernel's Chien search at `per` lanes per code word"""
    span = (255 + per - 1) // per
    pad = CODES[120]["PAD"]
    return [loc - pad for loc in range(span, 255, span) if 1 <= loc - pad < 120]


def words(code):
    """-> (patterns uint8 [n][N], kinds [n] of str)"""
    c = CODES[code]
    N, K, ROOTS, T, PAD = c["N"], c["K"], c["ROOTS"], c["T"], c["PAD"]
    rng = np.random.Generator(np.random.PCG64(88000 + code))          # (not default_rng: the suite may shift that one's seeds)
    pats, kinds = [], []

    def add(kind, positions, values):
        p = np.zeros(N, np.uint8)
        positions = [int(v) for v in positions]
        assert len(set(positions)) == len(positions) and all(0 <= v < N for v in positions)
        p[positions] = values
        assert np.count_nonzero(p) == len(positions)
        pats.append(p)
        kinds.append(kind)

    def values(n):
        return rng.integers(1, 256, n).astype(np.uint8)

    # ---- single ----
    for p in range(N):
        add("single", [p], [(0x01, 0x80, 0xFF)[p % 3]])
    # ---- exactly_t ----
    add("exactly_t:first", range(T), values(T))
    add("exactly_t:last", range(N - T, N), values(T))
    add("exactly_t:parity", range(K, K + T), values(T))
    add("exactly_t:data_parity", range(K - T // 2, K - T // 2 + T), values(T))
    if code == 204:
        add("exactly_t:seams", [0, 50, 51, 101, 102, 152, 153, 203], values(T))
    else:
        for per in DAB_PER:
            flat = sorted({q for s in dab_seams(per) for q in (s - 1, s)})
            for a in range(0, len(flat), T):
                group = flat[a:a + T]
                group += [q for q in flat if q not in group][:T - len(group)]
                if len(group) == T:
                    add(f"exactly_t:seams_per{per}", group, values(T))
    add("exactly_t:one_value", rng.choice(N, T, replace=False), [0x5A] * T)
    for _ in range(8):
        add("exactly_t:random", rng.choice(N, T, replace=False), values(T))
    # ---- beyond_t ----
    for _ in range(8):
        add("beyond_t:t_plus_1", rng.choice(N, T + 1, replace=False), values(T + 1))
    for _ in range(4):
        add("beyond_t:roots", rng.choice(N, ROOTS, replace=False), values(ROOTS))
    for e in (ROOTS + 1, ROOTS + 5, 2 * ROOTS, N // 2):
        add("beyond_t:more", rng.choice(N, e, replace=False), values(e))
    for _ in range(4):
        pats.append(rng.integers(0, 256, N).astype(np.uint8))
        kinds.append("beyond_t:random_word")
    # ---- miscorrect ----
    for j in (0, K // 2, K - 1):
        for v in range(1, 256):                           # (the code is linear: the first value serves unless the word is lighter)
            d = np.zeros(K, np.uint8)
            d[j] = v
            cw = encode(code, d)[0]
            if np.count_nonzero(cw) == ROOTS + 1:
                break
        assert np.count_nonzero(cw) == ROOTS + 1, (code, j)
        par = K + rng.permutation(ROOTS)
        with_data = [j] + [int(q) for q in par[:T]]
        add("miscorrect:with_data", with_data, cw[with_data])
        add("miscorrect:parity_only", par[:T + 1], cw[par[:T + 1]])
    # ---- padding_root ----
    for p in (0, PAD // 2, PAD - 1):
        par = _pm(code)[p].copy()                         # the unit message (value 1) at padding symbol p of the unshortened block
        assert np.count_nonzero(par) == ROOTS, (code, p)
        for m in range(1, T + 1):
            keep = np.sort(rng.permutation(ROOTS)[m - 1:])
            add(f"padding_root:m{m}", K + keep, par[keep])
    # ---- degenerate ----
    for a, b in ((0, 1), (10, 10 + K // 2), (0, N - 1)):
        add("degenerate:two_equal", [a, b], [0xA7, 0xA7])
    found, with_parity, tries = 0, 0, 0
    while (found < 6 or with_parity < 1) and tries < 100000:
        tries += 1
        a, b = (int(v) for v in rng.choice(N, 2, replace=False))
        if found >= 6:                                    # still missing: a triple with a member in the parity
            a = int(rng.integers(K, N))
            if a == b:
                continue
        X3 = int(EXP[(N - 1 - a) % 255]) ^ int(EXP[(N - 1 - b) % 255])
        c3 = N - 1 - int(LOG[X3])
        if not 0 <= c3 < N or c3 in (a, b):
            continue
        assert locator_of(code, [a, b, c3])[1] == 0
        in_parity = max(a, b, c3) >= K
        if found >= 6 and not in_parity:
            continue
        add("degenerate:sigma1_zero", [a, b, c3], values(3))
        found += 1
        with_parity += in_parity
    assert found >= 6 and with_parity >= 1, (code, found, with_parity)
    for _ in range(100000):                               # t errors whose locator has two zero coefficients among sigma_1..sigma_(t-1)
        pos = rng.choice(N, T, replace=False)
        if sum(1 for s in locator_of(code, pos)[1:T] if s == 0) >= 2:
            add("degenerate:two_zero_coefficients", pos, values(T))
            break
    add("degenerate:weight_1", [N // 3], [0x3C])
    pats.append(np.zeros(N, np.uint8))
    kinds.append("degenerate:clean")
    return np.stack(pats), kinds


def family(kind):
    return kind.split(":")[0]
