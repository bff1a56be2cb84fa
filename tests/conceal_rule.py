"""The concealment rule of ic_pc_conceal_tiles, stated in NumPy (a test helper: the product has no host path for it).

For a damaged tile T and a channel c the candidates are the symbols of channel c directly above T's top row, below its bottom
row, left of its left column and right of its right column (no corners) that lie inside the volume and in a tile that is not
damaged.  Every position of T in channel c gets the most frequent candidate, ties to the smallest symbol, or `fallback` where
there is none."""
import numpy as np


def grid(h, w, th, tw):
    return [(y0, x0, min(th, h - y0), min(tw, w - x0)) for y0 in range(0, h, th) for x0 in range(0, w, tw)]


def fallback_symbol(centers):
    """the centre of smallest magnitude, ties to the smallest index"""
    return int(np.argmin(np.abs(np.asarray(centers, dtype=np.float64))))


def conceal(symbols, damaged, th, tw, L, fallback):
    """symbols: (C, h, w) int64; damaged: tile indices in the raster order of grid(h, w, th, tw) -> the concealed copy"""
    src = np.asarray(symbols)
    C, h, w = src.shape
    tiles = grid(h, w, th, tw)
    gw = -(-w // tw)
    bad = set(int(t) for t in damaged)
    out = src.copy()
    for t in sorted(bad):
        y0, x0, a, b = tiles[t]
        ring = [(y0 - 1, x) for x in range(x0, x0 + b)] + [(y0 + a, x) for x in range(x0, x0 + b)] + \
               [(y, x0 - 1) for y in range(y0, y0 + a)] + [(y, x0 + b) for y in range(y0, y0 + a)]
        ring = [(y, x) for y, x in ring if 0 <= y < h and 0 <= x < w and (y // th) * gw + x // tw not in bad]
        for c in range(C):
            counts = np.zeros(L, np.int64)
            for y, x in ring:
                counts[src[c, y, x]] += 1                    # always the ORIGINAL volume: damaged tiles never read each other
            out[c, y0:y0 + a, x0:x0 + b] = int(np.argmax(counts)) if counts.max() > 0 else fallback      # argmax: the first maximum
    return out
