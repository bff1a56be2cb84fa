"""Shared helpers for the parity tests."""
import numpy as np
import torch

# Parity bar.  BASELINE.json north_star asks for "within 1e-4 fp32"; the kernels achieve far better, and an assert with
# 10-100x of slack would hide a regression, so the default bound is what is measured with a 2x margin: the HIP result
# must agree with the float64 evaluation of the oracle to 2e-5 relative to the tensor's scale, max(1, max|ref|)
# (round-2 GPU runs: single ops <= 3e-6, whole-network z / x_out / bit cost <= 1e-5).  Every comparison is recorded --
# absolute and relative maximum error -- and printed in the terminal summary (tests/conftest.py), so the log of a run shows
# the achieved accuracy, not just "passed".
RTOL = 2e-5                 # a single op
NET_RTOL = 5e-5             # a whole network (35 layers deep): the errors of the layers add up (measured <= 2.7e-5)
HEATMAP_RTOL = 1e-4         # heatmap = clip(sigmoid(z0) * C - c, 0, 1): amplifies the error of z0 by up to C / 4 (8 .. 16 x)
NORTH_STAR_RTOL = 1e-4
REPORT = []          # (label, max abs error, relative error, bound)
FLIPS = []           # (label, flipped symbols, total symbols)
# The clamp in max(1, max|ref|) turns the bound into an ABSOLUTE one for a tensor whose reference is much smaller than 1 (a
# gradient of order 1e-3 passes 1e-3 "relative" when half of it is missing), so assert_close asserts a second time against the
# reference's own scale: max|got - ref| <= true_rtol * max|ref| ("Parity scale").  SCALES keeps that yardstick per call.
SCALES = []          # (label, yardstick = max|ref64|, or the call's scale=)


def rel_err(got, ref64):
    got = got.detach().double().cpu() if torch.is_tensor(got) else torch.as_tensor(got).double()
    ref64 = ref64.detach().double().cpu() if torch.is_tensor(ref64) else torch.as_tensor(ref64).double()
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    scale = max(1.0, float(ref64.abs().max()))
    return float((got - ref64).abs().max()) / scale


def abs_err(got, ref64):
    got = got.detach().double().cpu() if torch.is_tensor(got) else torch.as_tensor(got).double()
    ref64 = ref64.detach().double().cpu() if torch.is_tensor(ref64) else torch.as_tensor(ref64).double()
    return float((got - ref64).abs().max())


def ref_scale(ref64):
    """max|ref64|: the scale-true yardstick of a comparison (0.0 for a reference that is identically zero)."""
    ref64 = ref64.detach().double().cpu() if torch.is_tensor(ref64) else torch.as_tensor(ref64).double()
    return float(ref64.abs().max()) if ref64.numel() else 0.0


def true_rel_err(got, ref64):
    """max|got - ref64| / max|ref64|: rel_err without the clamp at 1.  A reference that is identically zero has no scale of its
    own; the absolute error is returned for it, as rel_err does."""
    y = ref_scale(ref64)
    e = rel_err(got, ref64)            # checks the shapes
    return abs_err(got, ref64) / y if y > 0.0 else e


def assert_close(got, ref64, what, rtol=RTOL, true_rtol=None, scale=None):
    """two assertions: max|got - ref| <= rtol * max(1, max|ref|), the bar the report prints, and max|got - ref| <= true_rtol *
    yardstick with yardstick = max|ref| (skipped when the reference is identically zero: the first check is absolute there).
    true_rtol defaults to rtol.  scale= replaces max|ref| where another quantity sets the rounding error (a displacement p_new -
    p_old rounds like |p|): it comes from the operation's inputs or the reference, never from `got`, and may not exceed
    max(1, max|ref|), so the second check is never looser than the first at the same tolerance."""
    e = rel_err(got, ref64)
    a = abs_err(got, ref64)
    REPORT.append((what, a, e, rtol))
    y = ref_scale(ref64)
    if scale is not None:
        scale = float(scale)
        assert 0.0 < scale <= max(1.0, y), '{}: scale={:.3e} exceeds max(1, max|ref|) = {:.3e}'.format(what, scale, max(1.0, y))
        y = scale
    SCALES.append((what, y))
    t = rtol if true_rtol is None else true_rtol
    te = a / y if y > 0.0 else 0.0
    assert e <= rtol and te <= t, ('{}: max error {:.3e} absolute; {:.3e} of max(1, max|ref|), bound {:.1e}; {:.3e} of the yardstick '
                                   '{:.3e}, bound {:.1e}').format(what, a, e, rtol, te, y, t)
    return e


def record_flips(what, flips):
    """symbol flips between the fp32 device path and the float64 oracle (they are only legitimate inside the fp32 error band
    of a quantiser decision midpoint); the rate goes into the terminal summary."""
    flips = np.asarray(flips)
    FLIPS.append((what, int(flips.sum()), int(flips.size)))
    return float(flips.mean())


def _boundary_margin(z64, centers):
    """distance of every z to the nearest quantiser decision midpoint (float64)."""
    c = np.sort(np.asarray(centers, np.float64))
    mids = (c[1:] + c[:-1]) / 2
    return np.min(np.abs(z64[..., None] - mids), axis=-1)


def dev(a, device, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(device)


MSSSIM_CASES = {'a': (176, 208, 0), 'b': (256, 256, 1), 'c': (192, 320, 2)}


def msssim_case(name):
    """seeded NHWC uint8 image pair shared by tests/golden/make_golden.py and the metric tests."""
    h, w, k = MSSSIM_CASES[name]
    rs = np.random.RandomState(100 + k)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 60 * np.sin(xx / (7.0 + c) + yy / 11.0) + 30 * np.cos(yy / (5.0 + c))
                     for c in range(3)], -1)
    img1 = np.clip(base + rs.normal(0, 6, base.shape), 0, 255).astype(np.uint8)[None]
    img2 = np.clip(img1.astype(np.float64) + rs.normal(0, 3 + 4 * k, img1.shape), 0, 255).astype(np.uint8)
    return img1, img2
