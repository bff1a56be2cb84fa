"""The importance-map cap in NumPy float32, two ways (the rule of ic_heatmap_quantize_cap_f32):

    h2  = fl32(sigmoid(z0) * C);  h2' = min(h2, cap);  m' = max(min(h2' - ch, 1), 0);  z' = fl32(m' * zc)

`direct` is that, from (bottleneck, cap).  `from_heatmap` is m' = min(m, clamp(fl32(cap - ch), 0, 1)) from the UNCAPPED heatmap m:
subtraction of ch, rounding and the clamp are monotone, so they commute with the min -- the two agree bit for bit, and a test on
the device needs no sigmoid of its own (expf differs between libraries): it applies from_heatmap to the uncapped kernel's heatmap."""
import numpy as np

F = np.float32


def heatmap2d(bottleneck):
    """(N, C+1, h, w) float32 -> h2 (N, h, w) float32"""
    b = np.asarray(bottleneck, F)
    C = b.shape[1] - 1
    s = F(1.0) / (F(1.0) + np.exp(-b[:, 0]).astype(F))
    return (s.astype(F) * F(C)).astype(F)


def _ch(C):
    return np.arange(C, dtype=F)[None, :, None, None]


def direct(bottleneck, cap, h2=None):
    """bottleneck (N, C+1, h, w), cap (N, h, w) -> (m', z'), both (N, C, h, w) float32"""
    b = np.asarray(bottleneck, F)
    C = b.shape[1] - 1
    h2 = heatmap2d(b) if h2 is None else np.asarray(h2, F)
    h2c = np.minimum(h2, np.asarray(cap, F))
    m = np.maximum(np.minimum((h2c[:, None] - _ch(C)).astype(F), F(1.0)), F(0.0)).astype(F)
    return m, (m * b[:, 1:]).astype(F)


def from_heatmap(m, cap, zc):
    """m: the uncapped heatmap (N, C, h, w); cap (N, h, w); zc = bottleneck[:, 1:] -> (m', z')"""
    m = np.asarray(m, F)
    lim = np.clip((np.asarray(cap, F)[:, None] - _ch(m.shape[1])).astype(F), F(0.0), F(1.0)).astype(F)
    m2 = np.minimum(m, lim).astype(F)
    return m2, (m2 * np.asarray(zc, F)).astype(F)


def ulp_neighbours(values):
    """every value with its two float32 neighbours"""
    v = np.asarray(values, F)
    return np.concatenate([np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))]).astype(F)
