"""Self-test of tests/msssim_grad_rule.py, no device: the five parts add up to the autograd gradient, the float32 oracle passes the
criteria tests/test_gpu_msssim_grad.py applies to the kernel, and gradients that are wrong in ways a kernel can be wrong -- built
from the float64 parts -- are rejected by them."""
import numpy as np
import pytest
import torch

from tests import msssim_grad_rule as R

K = 5000.0          # K_ms_ssim of the cvpr configs
ALL_SHAPES = R.SHAPES + (R.BATCH_SHAPE,)


def _id(shape):
    return 'x'.join(str(v) for v in shape)


@pytest.mark.parametrize('shape', ALL_SHAPES, ids=_id)
def test_parts_add_up_to_the_autograd_gradient(shape):
    from oracle import train_oracle as T
    p = R.reference(shape, K)
    a, b = R.inputs(shape)
    tb = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    ms = T.ms_ssim(torch.as_tensor(a).double(), tb)
    (K * (1.0 - ms)).backward()
    ref = tb.grad.numpy()
    assert np.abs(p.g.sum(0) - ref).max() <= 1e-12 * np.abs(ref).max()
    assert abs(p.ms - float(ms.detach())) <= 1e-14 and abs(np.prod(p.S ** np.array(T.MSSSIM_WEIGHTS)) - p.ms) <= 1e-14
    # s_l is g_l's factor per position: count_l restated from the window rule (VALID 11-tap blur; a scale narrower than the
    # window is REFLECT-padded by (total, total // 2), total = window - WIDTH, on both axes)
    h, w = shape[2], shape[3]
    for l in range(5):
        k = 2 * (min(11, h, w) // 2) + 1
        total = max(k - w, 0)
        assert p.count[l] == shape[0] * shape[1] * (h + total + total // 2 - k + 1) * (w + total + total // 2 - k + 1)
        assert p.s[l] == pytest.approx(-K * T.MSSSIM_WEIGHTS[l] * p.ms / p.S[l] / p.count[l], rel=1e-14)
        h, w = (h + 1) // 2, (w + 1) // 2


@pytest.mark.parametrize('shape', ALL_SHAPES, ids=_id)
def test_condition_numbers_decide_where_the_fit_is_used(shape):
    c = R.cond(R.reference(shape, K))
    assert (c <= R.MAX_COND) == (shape in R.FIT_SHAPES), c
    if shape in R.FIT_SHAPES:
        assert c <= 60.0, c          # measured 3.8 .. 56: well inside the limit, not at its edge


@pytest.mark.parametrize('shape', ALL_SHAPES, ids=_id)
def test_float32_oracle_passes_the_criteria(shape):
    """the same expression evaluated in float32 on the CPU passes the kernel's criteria: GTOL of max|ref| (measured 1e-5 .. 1.7e-4) and
    the fit, the latter at the float32 oracle's own bound (measured |c_l - 1| <= 4.9e-5; the kernel centres its moments and is held to
    C_TOL, which the exact gradient passes)"""
    p = R.reference(shape, K)
    a, b = R.inputs(shape)
    g32 = R.parts(a, b, K, torch.float32).g.sum(0)
    assert R.violations(g32, p, shape in R.FIT_SHAPES, R.F32_ORACLE_C_TOL) == []
    assert R.violations(p.g.sum(0), p, shape in R.FIT_SHAPES) == []


def _mutants(p, fitted):
    """(name, gradient) of the wrong gradients that apply to the shape"""
    total = p.g.sum(0)
    for l in range(5):
        yield 'scale {} left out'.format(l), total - p.g[l]
    if fitted:
        # one percent of a scale is below GTOL of the whole wherever the scale's share of the maximum is below 2 %: only the fit
        # sees it there, so this one applies where the fit does
        for l in range(5):
            yield 'scale {} times 1.01'.format(l), total + 0.01 * p.g[l]
    yield 'shifted one pixel along x', np.roll(total, 1, axis=-1)
    planes = total.reshape((-1,) + total.shape[2:]).copy()
    planes[[0, 1]] = planes[[1, 0]]
    yield 'planes 0 and 1 exchanged', planes.reshape(total.shape)
    yield 'a NaN', np.where(np.arange(total.size).reshape(total.shape) == 7, np.nan, total)


@pytest.mark.parametrize('shape', ALL_SHAPES, ids=_id)
def test_wrong_gradients_are_rejected(shape):
    p = R.reference(shape, K)
    fitted = shape in R.FIT_SHAPES
    names = []
    for name, g in _mutants(p, fitted):
        assert R.violations(g, p, fitted), '{} passes at {}'.format(name, shape)
        names.append(name)
    assert len(names) == (13 if fitted else 8)


def test_why_this_file_exists():
    """at 1 x 3 x 160 x 160 a gradient without scale 0, 1, 2 or 3 is within 1e-3 of the reference in absolute terms -- the bound the
    kernel's test asserted, relative to max(1, max|ref|) = 1 -- and so is half the gradient"""
    from tests.util import rel_err
    p = R.reference((1, 3, 160, 160), K)
    total = p.g.sum(0)
    assert np.abs(total).max() < 2e-3
    for l in range(4):
        assert rel_err(total - p.g[l], total) < 1e-3 and np.abs(p.g[l]).max() < 1e-3
        assert R.violations(total - p.g[l], p, True)
    assert rel_err(0.5 * total, total) < 1e-3 and R.violations(0.5 * total, p, True)


def test_fit_recovers_known_coefficients():
    p = R.reference((1, 3, 160, 160), K)
    c = np.array([1.0, 0.5, 1.25, 0.0, -1.0])
    assert np.abs(R.fit(np.tensordot(c, p.g, 1), p) - c).max() <= 1e-10
