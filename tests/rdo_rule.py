"""The rule of the rate-aware symbol choice at encode (IC_PC_DECODE_RDO, Codec.compress(rdo=...)), spelled out position by position
(helper module; plain Python integers, float64 and numpy float32 scalars, a loop per position): what codec.ilog2_q16 /
rdo_lambda_q / rdo_choose / rdo_record must equal and what the device's sweep must produce.  The rule of a position takes (z, the
position's table row, the centres, Lambda) to a symbol; a sweep decides the positions of a coded volume in wavefront order, every
chosen symbol final.  Both forms of the sweep are here: sequential (decide, then derive the later rows from what was decided) and
teacher-forced (given the final symbols, every position's symbol equals the rule on its row) -- by induction over T they agree."""
import struct

import numpy as np

MAX_TOTAL = (1 << 30) + 2
HARD_SIGMA = np.float32(1e7)


def ilog2_q16(v):
    """log2 v in 2^-16 units for an integer 1 <= v < 2^32, in integers only"""
    v = int(v)
    assert 1 <= v < (1 << 32)
    e = v.bit_length() - 1
    m = v << (31 - e)
    r = e
    for _ in range(16):
        m = (m * m) >> 31
        assert m < (1 << 64)
        r = 2 * r
        if m >= (1 << 32):
            m >>= 1
            r |= 1
    return r


def lambda_q(lam):
    """Lambda = lam * 1e7 / 65536 in float64: lam is in key units per bit"""
    lam = float(lam)
    if not (lam >= 0.0 and lam < float('inf')):
        raise ValueError(lam)
    return lam * 1e7 / 65536.0


def key(z, c):
    """k = fl32(1e7 * fl32(t * t)), t = fl32(|z - c|): the hard quantiser's key"""
    t = np.abs(np.float32(z) - np.float32(c))
    with np.errstate(over='ignore', invalid='ignore'):
        return np.float32(HARD_SIGMA * np.float32(t * t))


def rates(freqs_row):
    """R_j of a table row, or None for a total above MAX_TOTAL (status 1: the position is decided with all R_j = 0)"""
    f = [int(v) for v in freqs_row]
    T = sum(f)
    if T > MAX_TOTAL:
        return None
    lT = ilog2_q16(T)
    return [lT - ilog2_q16(fj) for fj in f]


def choose(z, freqs_row, centers, lam_q, rated=True):
    """-> (symbol, status).  rated=False: the tile's first position, all R_j = 0"""
    L = len(centers)
    R, status = [0] * L, 0
    if rated:
        R = rates(freqs_row)
        if R is None:
            R, status = [0] * L, 1
    best, sym = float('inf'), 0
    for j in range(L):
        with np.errstate(over='ignore', invalid='ignore'):
            cost = float(np.float64(key(z, centers[j])) + np.float64(np.float64(lam_q) * np.float64(R[j])))
        if cost < best:
            best, sym = cost, j
    return sym, status


def hard(z, centers):
    """quantize_hard: the first argmax of fl32(-1e7 * fl32(t * t))"""
    best, sym = -float('inf'), 0
    for j in range(len(centers)):
        lh = float(-key(z, centers[j]))
        if lh > best:
            best, sym = lh, j
    return sym


def order(C, th, tw):
    """the positions of a tile front by front, (c, y, x) order within a front"""
    return sorted(((x + 2 * y + 4 * c, c, y, x) for c in range(C) for y in range(th) for x in range(tw)))


def sweep_sequential(z_chw, centers, lam_q, row_of, choose=choose):
    """row_of(symbols so far as a (C, th, tw) int array with -1 where undecided, (c, y, x)) -> the table row of that position, which
    may look only at positions of smaller T.  choose: the rule of one position (this module's, or the product's statement of it).
    -> (symbols, status)"""
    C, th, tw = z_chw.shape
    sym = -np.ones((C, th, tw), np.int64)
    status = 0
    for T, c, y, x in order(C, th, tw):
        rated = (c, y, x) != (0, 0, 0)
        s, st = choose(z_chw[c, y, x], row_of(sym, (c, y, x)) if rated else None, centers, lam_q, rated)
        sym[c, y, x] = s
        status |= st
    return sym, status


def sweep_holds(sym_chw, z_chw, centers, lam_q, rows_chwl, choose=choose):
    """teacher-forced: rows_chwl[c, y, x] is the table row of (c, y, x) given the FINAL symbols -> the positions (c, y, x) whose
    symbol is not the rule's on (z, its row), and the status the sweep must report"""
    C, th, tw = z_chw.shape
    bad, status = [], 0
    for c in range(C):
        for y in range(th):
            for x in range(tw):
                rated = (c, y, x) != (0, 0, 0)
                s, st = choose(z_chw[c, y, x], rows_chwl[c, y, x] if rated else None, centers, lam_q, rated)
                status |= st
                if s != int(sym_chw[c, y, x]):
                    bad.append((c, y, x))
    return bad, status


def record(lam_q, z_chw):
    """a tile's record: Lambda as a little-endian f64, then z as float32 in (c, y, x) order"""
    return struct.pack('<d', float(lam_q)) + np.ascontiguousarray(z_chw, dtype='<f4').tobytes()


def record_bytes(C, th, tw):
    return 8 + 4 * C * th * tw
