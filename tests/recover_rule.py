"""The rules of the recovery of layered files, stated in NumPy (a test helper: the product has no host path for them).

conceal_channels -- ic_pc_conceal_tiles_channels.  have[t] is the number of leading channels tile t holds, 0 .. C.  For a tile T with
have[T] < C and a channel c >= have[T] the candidates are the symbols of channel c directly above T's top row, below its bottom row,
left of its left column and right of its right column (no corners) that lie inside the volume and in a tile whose `have` exceeds c.
Every position of T in channel c gets the most frequent candidate, ties to the smallest symbol, or `fallback` where there is none.
Channels below have[T] are not touched.

preview_per_tile -- ic_pc_decode_tiles_batch_layers_pertile_f32 on a full decode: codec.preview_symbols applied to every tile with
that tile's own number of channels."""
import numpy as np

from tests.conceal_rule import grid


def conceal_channels(symbols, have, th, tw, L, fallback):
    """symbols: (C, h, w) int64; have: per tile in the raster order of grid(h, w, th, tw) -> the concealed copy"""
    src = np.asarray(symbols)
    C, h, w = src.shape
    tiles = grid(h, w, th, tw)
    gw = -(-w // tw)
    have = [int(v) for v in have]
    assert len(have) == len(tiles) and all(0 <= v <= C for v in have)
    out = src.copy()
    for t, (y0, x0, a, b) in enumerate(tiles):
        ring = [(y0 - 1, x) for x in range(x0, x0 + b)] + [(y0 + a, x) for x in range(x0, x0 + b)] + \
               [(y, x0 - 1) for y in range(y0, y0 + a)] + [(y, x0 + b) for y in range(y0, y0 + a)]
        ring = [(y, x) for y, x in ring if 0 <= y < h and 0 <= x < w]
        for c in range(have[t], C):
            counts = np.zeros(L, np.int64)
            for y, x in ring:
                if have[(y // th) * gw + x // tw] > c:
                    counts[src[c, y, x]] += 1                # always the ORIGINAL volume: channel c is written only where it is not read
            out[c, y0:y0 + a, x0:x0 + b] = int(np.argmax(counts)) if counts.max() > 0 else fallback      # argmax: the first maximum
    return out


def preview_per_tile(symbols, channels, th, tw, fill):
    """symbols: the full (C, h, w) decode; channels[t] in 0 .. C per tile -> a copy, tile t with [channels[t]:] = fill"""
    from imgcomp_cvpr_amd.codec import preview_symbols
    out = np.array(symbols, copy=True)
    for (y0, x0, a, b), k in zip(grid(out.shape[1], out.shape[2], th, tw), channels):
        out[:, y0:y0 + a, x0:x0 + b] = preview_symbols(out[:, y0:y0 + a, x0:x0 + b], k, fill)
    return out


def recover(symbols, channels, th, tw, L, fill):
    """what Codec.recover_symbols gives for a file whose full decode is `symbols` and whose tile t holds channels[t] leading channels"""
    return conceal_channels(preview_per_tile(symbols, channels, th, tw, fill), channels, th, tw, L, fill)
