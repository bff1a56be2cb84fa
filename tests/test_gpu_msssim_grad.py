"""-m gpu: csrc/msssim.hip (ic_msssim_loss_grad_f32) held to the float64 oracle scale by scale (tests/msssim_grad_rule.py).

The gradient of K (1 - MS-SSIM) is of order 1e-3 at the training crops, so it is judged by its own scale: GTOL of max|ref|, the
second check of util.assert_close.  Where the five scales' parts are well separated (cond <= 100) the gradient is also projected
on them and every coefficient must be 1 within C_TOL: a scale that is mis-weighted, mis-scaled or missing shows there however
small its share of the maximum is.  The per-scale means (scalars[2..6]) and the gradient scales every backward launch reads
(scalars[8..12]) are compared one by one, the value-only call (grad_out = NULL) must leave the same 16 scalars and no trace in
a gradient buffer, a batch with 360 partial sums at scale 0 takes the finishing kernel's strided loop into a second round, and
anti-correlated images give the NaN the reference's pow gives.  Every device buffer is a fenced one (tests/fenced.py).
"""
import numpy as np
import pytest
import torch

from tests import fenced as F
from tests import msssim_grad_rule as R
from tests.util import assert_close

pytestmark = pytest.mark.gpu
S_TOL = 1e-5          # each scalars[2 + l] against the float64 S_l, absolute (S_l is 0.9 .. 1): the bound of the value test
# each scalars[8 + l] against the float64 s_l, relative to s_l itself.  Measured on the GPU: at most 8.03e-8 (128 x 128, scale 4;
# DESIGN.md, "Parity scale") -- the float32 store of a value formed in float64 from means that are right to 8e-8.  Twice that.
SCALE_RTOL = 1.6e-7


def _id(shape):
    return 'x'.join(str(v) for v in shape)


def _K():
    from imgcomp_cvpr_amd import config_parser as cp
    ae, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'med'))
    return float(ae.K_ms_ssim)


class _Call(object):
    """the fenced buffers of one image pair and launches over them"""

    def __init__(self, cuda, a, b, K):
        from imgcomp_cvpr_amd import _lib as L
        self.L, self.K = L, K
        self.shape = N, C, H, W = tuple(int(v) for v in a.shape)
        nb = int(L.lib.ic_msssim_plan_bytes(H, W))
        assert nb > 0
        host = torch.zeros(nb, dtype=torch.uint8)
        L.check(L.lib.ic_msssim_plan_fill(H, W, host.data_ptr(), nb))
        self.plan = F.fenced(host, torch.uint8, cuda, F.IN_FENCE, 'plan')
        self.x, self.x_out = F.fenced(a, torch.float32, cuda, F.IN_FENCE, 'x'), F.fenced(b, torch.float32, cuda, F.IN_FENCE, 'x_out')
        self.need = int(L.lib.ic_msssim_workspace_bytes(N, C, H, W))
        assert self.need > 0
        self.ws = F.poison(F.fenced((self.need,), torch.uint8, cuda, F.OUT_FENCE, 'workspace'), 0xFF)
        self.grad = F.fenced(self.shape, torch.float32, cuda, F.OUT_FENCE, 'grad')
        self.scal = F.fenced((16,), torch.float32, cuda, F.OUT_FENCE, 'scalars')

    def launch(self, with_grad=True):
        L = self.L
        N, C, H, W = self.shape
        self.scal.fill_(float('nan'))
        L.check(L.lib.ic_msssim_loss_grad_f32(L.ptr(self.x), L.ptr(self.x_out), N, C, H, W, self.K, L.ptr(self.plan),
                                              L.ptr(self.grad) if with_grad else None, L.ptr(self.scal), L.ptr(self.ws), self.need,
                                              L.current_stream()))
        torch.cuda.synchronize()
        F.check_fences(self.plan, self.x, self.x_out, self.ws, self.grad, self.scal)
        return self.scal.clone()


def _check_values(scal, p, K, label):
    scal = scal.double().cpu().numpy()
    assert np.isfinite(scal).all(), scal
    assert abs(scal[0] - p.ms) < 1e-5 and abs(scal[1] - K * (1.0 - p.ms)) < 1e-5 * K, (scal[:2], p.ms)
    for l in range(5):
        e_S, e_s = abs(scal[2 + l] - p.S[l]), abs(scal[8 + l] / p.s[l] - 1.0)
        print('{}: scale {}: S_l {:.9f} error {:.3e}; s_l {:.6e} relative error {:.3e}'.format(label, l, p.S[l], e_S, p.s[l], e_s))
        assert e_S <= S_TOL, '{}: scalars[{}] = {!r}, S_{} = {!r}'.format(label, 2 + l, scal[2 + l], l, p.S[l])
        assert e_s <= SCALE_RTOL, '{}: scalars[{}] = {!r}, s_{} = {!r}: relative error {:.3e}'.format(label, 8 + l, scal[8 + l], l, p.s[l], e_s)
    assert (scal[[7, 13, 14, 15]] == 0.0).all()


def _check_gradient(grad, p, label, fitted):
    assert not bool(torch.isnan(grad).any()), '{}: gradient values not written'.format(label)
    print('{}: max error {:.3e} of max|ref| = {:.3e}'.format(label, R.max_norm_error(grad, p), np.abs(p.g.sum(0)).max()))
    if fitted:
        c = R.fit(grad, p)
        print('{}: fitted c_l - 1: {}; cond {:.1f}'.format(label, ' '.join('{:+.2e}'.format(v - 1.0) for v in c), R.cond(p)))
    assert_close(grad, torch.as_tensor(p.g.sum(0)), label, rtol=R.GTOL)
    assert R.violations(grad, p, fitted) == []


@pytest.mark.parametrize('shape', R.SHAPES + (R.BATCH_SHAPE,), ids=_id)
def test_gradient_and_scalars_scale_by_scale(cuda, shape):
    """the eight shapes of test_hip_ms_ssim_distortion_value_and_gradient and its inputs, and 30 x 3 x 64 x 64: 90 planes x 4 x 1
    tiles = 360 partial sums at scale 0, more than the finishing kernel's 256 threads take in one round"""
    K = _K()
    p = R.reference(shape, K)
    call = _Call(cuda, *R.inputs(shape), K=K)
    if shape == R.BATCH_SHAPE:
        assert shape[0] * shape[1] * -(-(shape[2] - 10) // 16) * -(-(shape[3] - 10) // 64) == 360
    label = 'MS-SSIM gradient by scale {}'.format(_id(shape))
    scal = call.launch()
    _check_values(scal, p, K, label)
    _check_gradient(call.grad, p, label, shape in R.FIT_SHAPES)


@pytest.mark.parametrize('shape', [(1, 3, 160, 160), (1, 3, 33, 47)], ids=_id)
def test_value_only_call(cuda, shape):
    """grad_out = NULL: the 16 scalars have the bits of the call with a gradient, and the gradient buffer of the previous call and
    its fences are as that call left them"""
    K = _K()
    call = _Call(cuda, *R.inputs(shape), K=K)
    with_grad = call.launch()
    before = F.snapshot(call.grad)
    F.poison(call.ws, 0x00)
    value_only = call.launch(with_grad=False)
    assert F.same_bits(with_grad, value_only), (with_grad, value_only)
    F.unchanged(before, call.grad)
    _check_values(value_only, R.reference(shape, K), K, 'MS-SSIM value only {}'.format(_id(shape)))


def test_anticorrelated_images(cuda):
    """b = 255 - a at 64 x 64: a negative contrast-structure mean makes the reference NaN (pow of a negative base), and then the
    device's MS-SSIM must be NaN too; were no mean negative for this input, the comparison would be the usual one"""
    K = _K()
    shape = (3, 3, 64, 64)
    a, _ = R.inputs(shape)
    b = 255.0 - a
    p = R.parts(a, b, K)
    call = _Call(cuda, a, b, K)
    scal = call.launch().double().cpu().numpy()
    label = 'MS-SSIM gradient by scale, anti-correlated {}'.format(_id(shape))
    if (p.S < 0.0).any():
        assert np.isnan(p.ms)
        assert np.isnan(scal[0]) and np.isnan(scal[1]), scal
        assert np.abs(scal[2:7] - p.S).max() <= S_TOL, (scal[2:7], p.S)          # the means themselves are finite
    else:
        _check_values(torch.as_tensor(scal), p, K, label)
        _check_gradient(call.grad, p, label, R.cond(p) <= R.MAX_COND)
