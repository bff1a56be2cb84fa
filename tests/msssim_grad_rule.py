"""The MS-SSIM distortion gradient taken apart by scale (helper module, no device code; tests/test_cpu_msssim_grad_rule.py is its
self-test, tests/test_gpu_msssim_grad.py holds csrc/msssim.hip to it).

d = K (1 - MS), MS = S_4^w_4 prod_{l<4} S_l^w_l, S_l the contrast-structure mean of scale l (the SSIM mean for l = 4), so

    dd/db = sum_l g_l,     g_l = -K w_l MS / S_l * dS_l/db,     s_l = -K w_l MS / S_l / count_l   (what the kernel keeps in scalars[8 + l])

with b the reconstruction and count_l the positions of scale l over all planes.  The five g_l differ by orders of magnitude in
the maximum norm (at 160 x 160 scale 0 is a seventh of the whole), so a maximum-norm bound -- even one relative to max|dd/db| --
says little about the small ones.  fit() therefore projects a gradient on the five parts: the least-squares c_l of
got ~ sum_l c_l g_l.  A kernel that mis-scales, mis-weights or drops scale l moves c_l away from 1 whatever that scale's share.
The fit is only meaningful where the five parts are well separated: cond() of the 5-column matrix, used where it is <= MAX_COND.
"""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

GTOL = 2e-4              # the project's gradient bound (tests/test_gpu_training.py), here of max|dd/db| itself: no clamp at 1
MAX_COND = 100.0         # the fit is asserted where the parts' condition number is at most this
# |c_l - 1| of the kernel's gradient: measured on the MI355X at most 3.84e-6 (33 x 47, scale 4; DESIGN.md, "Parity scale"); twice that.
# A hundredth of a scale (1e-2) is what the self-test's mutants are rejected at.
C_TOL = 8e-6
# the float32 oracle on the CPU does not centre its moments as the kernel does and reaches 4.9e-5 (64 x 64): its own bound, twice that
F32_ORACLE_C_TOL = 1e-4
SHAPES = ((2, 3, 128, 128), (3, 3, 64, 64), (1, 3, 160, 160), (2, 3, 72, 136), (1, 3, 33, 47), (1, 2, 17, 19), (1, 3, 320, 160), (2, 3, 40, 20))
BATCH_SHAPE = (30, 3, 64, 64)     # 90 planes x 4 x 1 tiles = 360 partial sums at scale 0: a second round of the finishing kernel's loop
# condition numbers (asserted by the self-test): 9.9, 50, 3.8, 7.5, 48, 6.2 and 56 for the batch; 1335 at 17 x 19 and 601 at
# 40 x 20, whose two coarsest scales have 2 .. 18 positions per plane -- those two keep the maximum-norm check only
FIT_SHAPES = tuple(s for s in SHAPES if s not in ((1, 2, 17, 19), (2, 3, 40, 20))) + (BATCH_SHAPE,)

Parts = namedtuple('Parts', 'S g s ms count')       # S (5,), g (5, N, C, H, W), s (5,), ms: float64 numpy / float; count (5,) ints


def inputs(shape):
    """the image pair of test_hip_ms_ssim_distortion_value_and_gradient: the synthetic 'natural' image 1 and itself plus noise of
    sigma 9, seed = H, clipped to 0..255 (float64).  Every draw is independent, so every plane has its own noise."""
    from imgcomp_cvpr_amd import weights as W
    rs = np.random.RandomState(shape[2])
    a = (W.synthetic_image((shape[0], 3, shape[2], shape[3]), 'natural', 1)[:, :shape[1]]).astype(np.float64)
    b = np.clip(a + rs.normal(0, 9, a.shape), 0, 255)
    return a, b


def parts(a, b, K, dtype=torch.float64):
    """-> Parts of K (1 - MS-SSIM(a, b)) with respect to b, every operation in `dtype`, the results as float64 numpy"""
    from oracle import train_oracle as T
    w = T.MSSSIM_WEIGHTS
    ta = torch.as_tensor(np.asarray(a)).to(dtype)
    tb = torch.as_tensor(np.asarray(b)).to(dtype).requires_grad_(True)
    S, count = [], []
    xa, xb = ta, tb
    for l in range(len(w)):
        ssim, cs = T._ssim_cs(xa, xb)
        S.append(ssim if l == len(w) - 1 else cs)
        size = min(11, xa.shape[2], xa.shape[3])
        count.append(int(T._gaussian_blur(xa.detach(), size * 1.5 / 11, size).numel()))
        xa, xb = [T._sep_valid(F.pad(t, (0, 1, 0, 1), mode='reflect'), np.ones(2) / 2.0)[:, :, ::2, ::2] for t in (xa, xb)]
    ms = S[0] ** w[0]
    for l in range(1, len(w)):
        ms = ms * S[l] ** w[l]
    g, s = [], []
    for l in range(len(w)):
        dS, = torch.autograd.grad(S[l], tb, retain_graph=True)
        f = -K * w[l] * ms.detach() / S[l].detach()
        g.append((f * dS).double().numpy())
        s.append(float(f.double()) / count[l])
    return Parts(np.array([float(v.detach().double()) for v in S]), np.stack(g), np.array(s), float(ms.detach().double()), np.array(count))


@functools.lru_cache(maxsize=None)
def reference(shape, K):
    """float64 Parts of the shape's own inputs: once per process, shared and left unchanged"""
    a, b = inputs(shape)
    return parts(a, b, K)


def _columns(p):
    return np.asarray(p.g, np.float64).reshape(len(p.g), -1).T


def cond(p):
    """condition number of the 5-column matrix of the parts"""
    return float(np.linalg.cond(_columns(p)))


def fit(got, p):
    """least-squares c_l of got ~ sum_l c_l g_l, float64"""
    got = np.asarray(got.detach().double().cpu() if torch.is_tensor(got) else got, np.float64)
    c, _, rank, _ = np.linalg.lstsq(_columns(p), got.reshape(-1), rcond=None)
    assert rank == len(p.g)
    return c


def max_norm_error(got, p):
    """max|got - sum_l g_l| / max|sum_l g_l|"""
    got = np.asarray(got.detach().double().cpu() if torch.is_tensor(got) else got, np.float64)
    ref = np.asarray(p.g, np.float64).sum(0)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def violations(got, p, fit_it, c_tol=C_TOL):
    """the criteria of tests/test_gpu_msssim_grad.py on a gradient: [] or one line per criterion it misses.  A gradient that is not
    finite misses the first."""
    out = []
    e = max_norm_error(got, p)
    if not e <= GTOL:
        out.append('max error {:.3e} of max|ref| exceeds {:.1e}'.format(e, GTOL))
    if fit_it and np.isfinite(e):
        c = fit(got, p)
        for l, v in enumerate(c):
            if not abs(v - 1.0) <= c_tol:
                out.append('scale {}: fitted coefficient {:.6f}, |c - 1| = {:.3e} exceeds {:.1e}'.format(l, v, abs(v - 1.0), c_tol))
    return out
