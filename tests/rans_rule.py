"""The rule of the lane-parallel rANS tiles (container format 12), spelled out position by position (helper module; plain loops over
every (c, y, x) and every symbol, no array tricks): what codec.rans_table / rans_slot / rans_rounds / rans_encode / rans_decode must
equal, and what the device encoder and decoder must produce.  The encoder here is written from the CODER's definition (it runs the
rounds backwards and reverses what it emitted), the decoder from the STREAM's definition (states first, then words in the order it
takes them): that the one reads what the other wrote is the statement about the word order."""
import numpy as np

M = 1 << 16
MAX_TOTAL = (1 << 30) + 2
LANES = (8, 16, 32, 64)


def table(freqs_row):
    """g of a row f of the arithmetic coder's table, as Python integers"""
    f = [int(v) for v in freqs_row]
    L, T = len(f), sum(int(v) for v in freqs_row)
    g = []
    for fj in f:
        q = (fj * (M - L)) // T
        g.append(q if q >= 1 else 1)
    deficit = M - sum(g)
    assert deficit >= 1
    first_max = 0
    for j in range(L):
        if f[j] > f[first_max]:
            first_max = j
    g[first_max] += deficit
    return g


def fronts(C, th, tw):
    """{t: [(c, y, x)] in (c, y, x) order} of a tile"""
    out = {}
    for c in range(C):
        for y in range(th):
            for x in range(tw):
                out.setdefault(x + 2 * y + 4 * c, []).append((c, y, x))
    return out


def slot(C, th, tw, c, y, x):
    """the candidate index of (c, y, x) on its front, from the enumeration's definition: channels from the first that has a position
    on the front, iw slots each, rows from the first that has one -- found by search, not by the closed form"""
    t = x + 2 * y + 4 * c
    iw = min(th, (tw + 1) // 2)
    c_lo = 0                                                  # the first channel whose last position lies on the front or behind it
    while t - 4 * c_lo > (tw - 1) + 2 * (th - 1):
        c_lo += 1
    # the first row of channel c with x <= tw - 1; rows below it would need x beyond the tile (x >= 0 is not asked for here: the
    # enumeration runs upwards from this row and leaves the candidates with x < 0 as holes)
    y_lo = 0
    while t - 4 * c - 2 * y_lo > tw - 1:
        y_lo += 1
    return (c - c_lo) * iw + (y - y_lo)


def rounds(C, th, tw, W):
    """[[raster index or -1] * W] in round order, the rounds that hold only -1 dropped"""
    out = []
    for t, positions in sorted(fronts(C, th, tw).items()):
        by_round = {}
        for (c, y, x) in positions:
            e = slot(C, th, tw, c, y, x)
            row = by_round.setdefault(e // W, [-1] * W)
            assert row[e % W] == -1, 'two positions in one slot'
            if (c, y, x) != (0, 0, 0):
                row[e % W] = (c * th + y) * tw + x
        for r in sorted(by_round):
            if any(v >= 0 for v in by_round[r]):
                out.append(by_round[r])
    return out


def encode(freq_rows, symbols, W):
    """freq_rows[i] / symbols[i] for i = r W + l in round order, symbol -1: a hole -> (bytes or None, status).  Status 3: a symbol
    outside [0, L); 1: a total above MAX_TOTAL; the later round decides, and within a round 3 comes before 1, as on the device."""
    n = len(symbols)
    assert n % W == 0
    state = [M] * W
    emitted = []                                              # in the order the encoder emits: the reverse of the stream
    for r in range(n // W - 1, -1, -1):
        bad = set()
        for l in range(W):
            s = int(symbols[r * W + l])
            if s == -1:
                continue
            if not 0 <= s < len(freq_rows[r * W + l]):
                bad.add(3)
            elif sum(int(v) for v in freq_rows[r * W + l]) > MAX_TOTAL:
                bad.add(1)
        if bad:
            return None, 3 if 3 in bad else 1
        for l in range(W - 1, -1, -1):                       # backwards within the round too
            i = r * W + l
            s = int(symbols[i])
            if s == -1:
                continue
            g = table(freq_rows[i])
            cg = sum(g[:s])
            x = state[l]
            if x >= g[s] << 16:
                emitted.append(x & 0xffff)
                x >>= 16
            assert x < g[s] << 16                            # at most one word per symbol
            state[l] = ((x // g[s]) << 16) + x % g[s] + cg
            assert M <= state[l] < 1 << 32
    out = bytearray()
    for x in state:
        out += bytes([x & 255, x >> 8 & 255, x >> 16 & 255, x >> 24 & 255])
    for word in reversed(emitted):
        out += bytes([word & 255, word >> 8])
    return bytes(out), 0


def decode(data, round_rows, W, freqs_of, out, full=True, stop=None):
    """round_rows as `rounds` gives them; freqs_of(out, index) -> the row of that position; out is written in place -> status (1 and
    4 OR-ed; decoding goes on behind a total that is too large).  stop: rounds to decode."""
    data = bytes(data)

    def byte(i):
        return data[i] if i < len(data) else 0                # past its end a stream reads as zeros

    state = [byte(4 * l) + (byte(4 * l + 1) << 8) + (byte(4 * l + 2) << 16) + (byte(4 * l + 3) << 24) for l in range(W)]
    words, status = 0, 0
    for r, row in enumerate(round_rows):
        if stop is not None and r >= stop:
            break
        got = []
        for l in range(W):
            if row[l] < 0:
                continue
            f = [int(v) for v in freqs_of(out, row[l])]
            if sum(f) > MAX_TOTAL:
                status |= 1
            g = table(f)
            s = state[l] & 0xffff
            k, cg = 0, 0
            while not cg <= s < cg + g[k]:
                cg += g[k]
                k += 1
            x = g[k] * (state[l] >> 16) + s - cg
            assert 0 <= x < 1 << 32
            if x < M:
                x = (x << 16) | byte(4 * W + 2 * words) | (byte(4 * W + 2 * words + 1) << 8)
                words += 1
            state[l] = x
            got.append((row[l], k))
        for i, k in got:
            out[i] = k
    if full and stop is None:
        if any(x != M for x in state) or 4 * W + 2 * words != len(data):
            status |= 4
    return status


def preview_rounds(C, th, tw, W, channels):
    """how many rounds a sweep steps through that stops behind the last front of channel `channels` - 1"""
    t_last = (tw - 1) + 2 * (th - 1) + 4 * (channels - 1)
    n = 0
    for row in rounds(C, th, tw, W):
        i = max(row)
        c, rest = divmod(i, th * tw)
        if (rest % tw) + 2 * (rest // tw) + 4 * c <= t_last:
            n += 1
    return n
