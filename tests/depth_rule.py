"""The rule of the depth-mapped tiles (container format 10), spelled out position by position (helper module; loops over every
(c, y, x), no array tricks): what codec.depth_plane / depth_live_mask must equal, and a host model of the coded stream -- the host
coder over the live positions of the wavefront order, and the host decoder that steps over the dead ones."""
import numpy as np

from tests import codec_cases as cc


def wavefront_positions(C, th, tw):
    """[(c, y, x)] sorted by (x + 2 y + 4 c, c, y, x): the coding order of format 5, from its definition"""
    return sorted(((c, y, x) for c in range(C) for y in range(th) for x in range(tw)), key=lambda p: (p[2] + 2 * p[1] + 4 * p[0],) + p)


def depth_plane(sym, fill, B):
    C, h, w = sym.shape
    nby, nbx = (h + B - 1) // B, (w + B - 1) // B
    out = np.zeros((nby, nbx), np.uint8)
    for c in range(C):
        for y in range(h):
            for x in range(w):
                if sym[c, y, x] != fill:
                    out[y // B, x // B] = max(out[y // B, x // B], c + 1)
    return out


def live(C, th, tw, depth, B):
    """bool (C, th, tw): c < depth[y // B][x // B], a depth above C counting as C"""
    out = np.zeros((C, th, tw), bool)
    for c in range(C):
        for y in range(th):
            for x in range(tw):
                out[c, y, x] = c < min(int(depth[y // B][x // B]), C)
    return out


def live_mask(C, th, tw, depth, B):
    """the keep-mask in coding order"""
    lv = live(C, th, tw, depth, B)
    return np.array([lv[p] for p in wavefront_positions(C, th, tw)], bool)


def front_steps(C, th, tw, depth):
    """the steps of the decoder's front sweep: T = 7 .. the front of the last position of channel dmax - 1 in the padded volume"""
    dmax = min(int(np.max(depth)), C)
    return 0 if dmax == 0 else (tw + 3) + 2 * (th + 3) + 4 * (dmax + 3) - 6


def coded_positions(C, th, tw, depth, B):
    """the positions the coder sees, in order: the wavefront order without the first position and without the dead ones"""
    lv = live(C, th, tw, depth, B)
    return [p for p in wavefront_positions(C, th, tw)[1:] if lv[p]]


def host_encode(sym, freqs_chw, depth, B):
    """the coder's bytes of a tile: host_encode over the kept subsequence.  freqs_chw: (C, th, tw, L) table rows by position"""
    C, th, tw = sym.shape
    pos = coded_positions(C, th, tw, depth, B)
    rows = np.asarray([freqs_chw[p] for p in pos], np.int64).reshape(len(pos), np.shape(freqs_chw)[-1])     # (0, L) when nothing is live
    return cc.host_encode(np.asarray([int(sym[p]) for p in pos], np.int64), rows)[0]


def host_decode(data, freqs_of, shape, depth, B, first, fill, channels=None):
    """the depth-aware host decoder.  freqs_of(volume so far, (c, y, x)) -> table row of that position; dead positions are `fill`
    without a coder step, the first position is `first` unless dead; channels=K: the coder stops behind the last front of channel
    min(K, dmax) - 1 and every position of the channels from there on is `fill` -> (C, th, tw) int64"""
    import io
    from imgcomp_cvpr_amd import arithmetic_coding as ac
    C, th, tw = shape
    lv = live(C, th, tw, depth, B)
    dmax = min(int(np.max(depth)), C)
    cdec = dmax if channels is None else min(int(channels), dmax)
    t_last = (tw - 1) + 2 * (th - 1) + 4 * (cdec - 1)
    out = np.full(shape, fill, np.int64)
    dec = ac.ArithmeticDecoder(ac.BitInputStream(io.BytesIO(bytes(data))))
    for i, p in enumerate(wavefront_positions(C, th, tw)):
        if p[2] + 2 * p[1] + 4 * p[0] > t_last:
            break
        if not lv[p]:
            continue
        out[p] = first if i == 0 else dec.read(ac.SimpleFrequencyTable([int(v) for v in freqs_of(out, p)]))
    out[cdec:] = fill
    return out


def planted(shape, fill, L, cell_depths, seed):
    """a (C, h, w) volume whose cell (y, x) holds non-fill symbols in channel cell_depths[y][x] - 1 (so that the rule's depth is
    exact), random symbols below it and `fill` from there up; cell depth 0: all fill"""
    C, h, w = shape
    rs = np.random.RandomState(seed)
    sym = rs.randint(0, L, size=shape).astype(np.int64)
    other = (fill + 1) % L
    for y in range(h):
        for x in range(w):
            d = int(cell_depths[y][x])
            sym[d:, y, x] = fill
            if d > 0:
                sym[d - 1, y, x] = other
    return sym
