"""tests/bn_rule.py on the host: the float64 rule against torch's float64 batch_norm and its autograd, and the sensitivity of
the checks that tests/test_gpu_bn_kernels.py runs on the device -- a NumPy float32 emulation of csrc/train_bn.hip passes every
one of them at every shape of the table, and the same emulation with one subtle fault fails them."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bn_rule as R
from tests import util

f32 = np.float32


def _c(v):
    return np.asarray(v, f32).reshape(1, -1, 1, 1)


def _fma32(x, a, b):
    """fmaf on fp32 arrays: the product is exact in double, one rounding to double and one to float (a double rounding can
    differ from fmaf in the last bit on a few elements in 2^29: nothing the bounds notice, and never the sign)"""
    return (np.asarray(x, np.float64) * np.asarray(a, np.float64) + np.asarray(b, np.float64)).astype(f32)


class Emulation:
    """csrc/train_bn.hip in NumPy: float64 sums per batch slice, totals in slice order, fp32 everywhere else.  `fault` names
    ONE way of being subtly wrong."""
    FAULTS = ('drop one element', 'count one element twice', 'skip the last image of a ragged slice', 'mask >=',
              'biased moving variance', 'count = N HW', 'res2 ignored', 'channel off by one above 64')

    def __init__(self, fault=None):
        assert fault is None or fault in self.FAULTS
        self.fault = fault

    # -- the reductions: bn_partial_kernel + bn_totals
    def _totals(self, t0, t1):
        N, C = t0.shape[:2]
        t0, t1 = t0.copy(), t1.copy()
        # the element the fault hits: the last image, the last channel, a pixel inside the plane, where the term is not 0
        n, c = N - 1, C - 1
        p = int(np.argmax(np.abs(t0[n, c].reshape(-1)) >= 0.5))
        for t in (t0, t1):
            flat = t[n, c].reshape(-1)
            if self.fault == 'drop one element':
                flat[p] = 0.0
            if self.fault == 'count one element twice':
                flat[p] *= 2.0
        per = -(-N // R.BN_SPLIT)
        s0, s1 = np.zeros(C), np.zeros(C)
        for n0, n1 in R.slices(N):
            if self.fault == 'skip the last image of a ragged slice' and 0 < n1 - n0 < per:
                n1 -= 1
            s0 = s0 + t0[n0:n1].sum(axis=(0, 2, 3))
            s1 = s1 + t1[n0:n1].sum(axis=(0, 2, 3))
        return np.stack([self._channels(s0), self._channels(s1)])

    def _channels(self, v):
        """what the finish kernels read for channel c"""
        if self.fault == 'channel off by one above 64':
            idx = np.arange(v.shape[0])
            idx = np.where(idx >= 64, np.minimum(idx + 1, v.shape[0] - 1), idx)
            return v[idx]
        return v

    def moments(self, x):
        x = np.asarray(x, np.float64)
        return self._totals(x, x * x)

    # -- bn_fold_values / bn_fold_channel
    def _fold(self, sums, M, gamma, beta, mm, mv):
        m = sums[0] / M
        v = np.maximum(sums[1] / M - m * m, 0.0)
        mf, vf = m.astype(f32), v.astype(f32)
        inv = f32(1.0) / np.sqrt(vf + f32(R.EPS), dtype=f32)
        sc = np.asarray(gamma, f32) * inv
        out = {'mean': mf, 'var': vf, 'invstd': inv, 'scale': sc, 'shift': np.asarray(beta, f32) - mf * sc}
        decay = f32(R.DECAY)
        unbiased = vf if self.fault == 'biased moving variance' else vf * f32(float(M) / float(M - 1 if M > 1 else 1))
        out['mm'] = np.asarray(mm, f32) * decay + mf * (f32(1) - decay)
        out['mv'] = np.asarray(mv, f32) * decay + unbiased * (f32(1) - decay)
        return out

    def stats(self, x):
        st = self._fold(self.moments(x), x.shape[0] * x.shape[2] * x.shape[3], np.ones(x.shape[1]), np.zeros(x.shape[1]),
                        np.zeros(x.shape[1]), np.zeros(x.shape[1]))
        return st['mean'], st['var']

    def train_stats(self, x, gamma, beta, mm, mv):
        return self._fold(self.moments(x), x.shape[0] * x.shape[2] * x.shape[3], gamma, beta, mm, mv)

    def fold_moments(self, sums, count, gamma, beta, mm, mv):
        return self._fold(np.stack([self._channels(sums[0]), self._channels(sums[1])]), count, gamma, beta, mm, mv)

    # -- the element-wise kernels
    def apply(self, x, scale, shift, res1, res2, relu):
        y = _fma32(x, _c(scale), _c(shift))
        if relu:
            y = np.maximum(y, f32(0))
        if res1 is not None:
            y = y + res1
        if res2 is not None and self.fault != 'res2 ignored':
            y = y + res2
        return y

    def _g(self, dy, x, scale, shift, relu):
        if not relu:
            return np.asarray(dy, f32)
        pre = _fma32(x, _c(scale), _c(shift))
        return np.where(pre >= 0 if self.fault == 'mask >=' else pre > 0, dy, f32(0)).astype(f32)

    def backward_reduce(self, dy, x, scale, shift, mean, invstd, relu):
        g = self._g(dy, x, scale, shift, relu).astype(np.float64)
        xh = ((np.asarray(x, f32) - _c(mean)) * _c(invstd)).astype(np.float64)
        sums = self._totals(g, g * xh)
        return sums, sums[1].astype(f32), sums[0].astype(f32)

    def backward_apply(self, dy, x, scale, shift, mean, invstd, gamma, sums, count, relu):
        N, C, H, W = x.shape
        M = float(N * H * W) if self.fault == 'count = N HW' else float(count)
        g = self._g(dy, x, scale, shift, relu)
        k = np.asarray(gamma, f32) * np.asarray(invstd, f32)
        mg, mgx = (np.asarray(sums[0]) / M).astype(f32), (np.asarray(sums[1]) / M).astype(f32)
        return _c(k) * (g - _c(mg) - (np.asarray(x, f32) - _c(mean)) * _c(invstd) * _c(mgx))

    def backward(self, dy, x, scale, shift, mean, invstd, gamma, relu):
        sums, dgamma, dbeta = self.backward_reduce(dy, x, scale, shift, mean, invstd, relu)
        N, C, H, W = x.shape
        return self.backward_apply(dy, x, scale, shift, mean, invstd, gamma, sums, N * H * W, relu), dgamma, dbeta


# ---- the rule itself against torch, float64 ------------------------------------------------------------------------------

F64_TOL = 1e-12          # float64 against float64, relative to the tensor scale: a few hundred roundings of 1.1e-16


@pytest.mark.parametrize('name', ['c', 'j'])
@pytest.mark.parametrize('relu', [0, 1])
def test_rule_matches_torch_float64_batch_norm(name, relu):
    """outputs, running statistics, dx, dgamma and dbeta of F.batch_norm(training=True, momentum=0.1) under float64 autograd.
    Every stage of the rule gets float64 inputs here (its own fold, unrounded), so only what the rule states is compared; the
    one fp32 expression in it, xhat of the backward sums, has its rounding bounded from the format."""
    d = R.case_data(name)
    x, dy, gamma, beta = d['x'], d['dy'], d['gamma'], d['beta']
    N, C, H, W = x.shape
    M = N * H * W
    assert M > 1
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), requires_grad=g)
    xt, gt, bt = t(x, True), t(gamma, True), t(beta, True)
    rm, rv = t(d['mm']), t(d['mv'])
    y = F.batch_norm(xt, rm, rv, gt, bt, training=True, momentum=0.1, eps=R.EPS)
    if relu:
        y = F.relu(y)
    y = y + t(d['res1']) + t(d['res2'])
    y.backward(t(dy))

    s, ss, _, _ = R.moments(x)
    st = R.fold(s, ss, M, gamma, beta, d['mm'], d['mv'], decay=0.9)          # momentum 0.1 is decay 0.9, not the float of it
    R.assert_scaled(R.apply(x, st['scale'], st['shift'], d['res1'], d['res2'], relu), y.detach().numpy(), F64_TOL, 'rule vs torch: y')
    R.assert_scaled(st['mm'], rm.numpy(), F64_TOL, 'rule vs torch: running mean')
    R.assert_scaled(st['mv'], rv.numpy(), F64_TOL, 'rule vs torch: running variance')
    R.assert_scaled(st['var'], xt.detach().var(dim=(0, 2, 3), unbiased=False).numpy(), F64_TOL, 'rule vs torch: variance')
    # no element within rounding of the ReLU's edge: the two float64 masks are the same mask
    assert float(np.abs(R.apply(x, st['scale'], st['shift'])).min()) > 1e-9
    g, gx, g_abs, _ = R.backward_sums(dy, x, st['scale'], st['shift'], st['mean'], st['invstd'], relu)
    R.assert_scaled(g, bt.grad.numpy(), F64_TOL, 'rule vs torch: dbeta')
    # xhat32 = fl(fl(x - fl(mean)) * fl(invstd)): against the float64 xhat it is off by at most
    # 2^-24 (|mean| invstd + 3 |xhat|) to first order; 1.01 for the second order
    gm = np.abs(R.masked_gradient(dy, x, st['scale'], st['shift'], relu))
    xh = np.abs((x.astype(np.float64) - st['mean'].reshape(1, -1, 1, 1)) * st['invstd'].reshape(1, -1, 1, 1))
    slack = 1.01 * 2.0 ** -24 * (gm * (np.abs(st['mean'] * st['invstd']).reshape(1, -1, 1, 1) + 3 * xh)).sum(axis=(0, 2, 3))
    R.assert_sums(gx, gt.grad.numpy(), slack, 'rule vs torch: dgamma (fp32 xhat)')
    # backward_apply on float64 sums of its own inputs
    gx64 = (R.masked_gradient(dy, x, st['scale'], st['shift'], relu) *
            (x.astype(np.float64) - st['mean'].reshape(1, -1, 1, 1)) * st['invstd'].reshape(1, -1, 1, 1)).sum(axis=(0, 2, 3))
    dx = R.backward_apply(dy, x, st['scale'], st['shift'], st['mean'], st['invstd'], relu, g, gx64, M, gamma)
    R.assert_scaled(dx, xt.grad.numpy(), 1e-11, 'rule vs torch: dx')


def test_the_data_is_what_the_bounds_assume():
    for name in R.SHAPES:
        d = R.case_data(name)
        assert d['x'].dtype == f32 and d['x'].shape == R.SHAPES[name]
        assert float(np.abs(d['x']).min()) >= 0.5 and float(np.abs(d['dy']).min()) >= 0.5
        assert 0.5 <= float(d['gamma'].min()) and float(d['gamma'].max()) <= 1.5
    assert R.slices(5) == [(0, 2), (2, 4), (4, 5), (5, 5)] and R.slices(1) == [(0, 1), (1, 1), (1, 1), (1, 1)]


# ---- the checks pass on the kernels' arithmetic ... -----------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(R.SHAPES))
@pytest.mark.parametrize('relu', [0, 1])
def test_emulated_kernels_pass_every_check(name, relu):
    R.check_case(Emulation(), name, relu)


def test_emulated_kernels_pass_the_relu_tie():
    R.check_relu_tie(Emulation())


# ---- ... and fail them when the arithmetic is subtly wrong ----------------------------------------------------------------

@contextlib.contextmanager
def _caught():
    """the block must fail an assertion; what it recorded is the error of a fault, not of the project: out of the parity report"""
    n = len(util.REPORT)
    with pytest.raises(AssertionError):
        yield
    del util.REPORT[n:]


LARGEST = max(R.SHAPES, key=lambda k: R.SHAPES[k][0] * R.SHAPES[k][2] * R.SHAPES[k][3])       # the most elements per channel


@pytest.mark.parametrize('fault,name,relu', [
    ('drop one element', LARGEST, 0), ('drop one element', LARGEST, 1),
    ('count one element twice', LARGEST, 0), ('count one element twice', LARGEST, 1),
    ('skip the last image of a ragged slice', 'd', 0),
    ('biased moving variance', 'c', 0), ('biased moving variance', LARGEST, 0),
    ('count = N HW', 'c', 0), ('count = N HW', 'a', 1),
    ('res2 ignored', 'c', 1),
    ('channel off by one above 64', 'i', 0),
])
def test_a_subtly_wrong_kernel_is_caught(fault, name, relu):
    with _caught():
        R.check_case(Emulation(fault), name, relu)


def test_one_element_moves_a_sum_far_beyond_its_bound():
    """the margin of the sums check at the largest shape: one element of 66 000 is worth at least 0.5, the bound is below 1e-5"""
    assert LARGEST == 'f'
    x = R.case_data(LARGEST)['x']
    s, ss, s_abs, ss_abs = R.moments(x)
    M = x.shape[0] * x.shape[2] * x.shape[3]
    assert float(R.sum_bound(M, s_abs).max()) < 1e-5 and float(R.sum_bound(M, ss_abs).max()) < 1e-4
    for fault in ('drop one element', 'count one element twice'):
        got = Emulation(fault).moments(x)
        assert float(np.abs(got[0] - s).max()) >= 0.5 and float(np.abs(got[1] - ss).max()) >= 0.25
        with _caught():
            R.assert_sums(got[0], s, R.sum_bound(M, s_abs), 'sum x with a fault')
        with _caught():
            R.assert_sums(got[1], ss, R.sum_bound(M, ss_abs), 'sum x^2 with a fault')
        gsum = Emulation(fault).backward_reduce(R.case_data(LARGEST)['dy'], x, np.ones(2, f32), np.zeros(2, f32), np.zeros(2, f32), np.ones(2, f32), 0)[0]
        g, gx, g_abs, gx_abs = R.backward_sums(R.case_data(LARGEST)['dy'], x, np.ones(2, f32), np.zeros(2, f32), np.zeros(2, f32), np.ones(2, f32), 0)
        with _caught():
            R.assert_sums(gsum[0], g, R.sum_bound(M, g_abs), 'sum g with a fault')
        with _caught():
            R.assert_sums(gsum[1], gx, R.sum_bound(M, gx_abs), 'sum g xhat with a fault')


def test_mask_ge_is_caught_on_the_tie():
    with _caught():
        R.check_relu_tie(Emulation('mask >='))
    # and by nothing else: away from the tie `>=` and `>` are the same kernel
    R.check_case(Emulation('mask >='), 'c', 1)


@pytest.mark.parametrize('fault', ['biased moving variance', 'count = N HW', 'res2 ignored', 'channel off by one above 64', 'mask >='])
def test_each_fault_fails_the_comparison_it_belongs_to(fault):
    """not just `some assertion fails`: the helper that is there for the fault is the one that raises"""
    name = 'i' if fault.startswith('channel') else 'c'
    d = R.case_data(name)
    x, dy, gamma, beta = d['x'], d['dy'], d['gamma'], d['beta']
    N, C, H, W = x.shape
    M = N * H * W
    good, bad = Emulation(), Emulation(fault)
    st = good.train_stats(x, gamma, beta, d['mm'], d['mv'])
    s, ss, _, _ = R.moments(x)
    ref = R.fold(s, ss, M, gamma, beta, d['mm'], d['mv'])
    sc, sh, mu, inv = st['scale'], st['shift'], st['mean'], st['invstd']
    with _caught():
        if fault == 'biased moving variance':
            R.assert_scaled(bad.train_stats(x, gamma, beta, d['mm'], d['mv'])['mv'], ref['mv'], R.STAT_TOL, 'moving variance with a fault')
        elif fault == 'count = N HW':
            sums = good.backward_reduce(dy, x, sc, sh, mu, inv, 0)[0]
            R.assert_scaled(bad.backward_apply(dy, x, sc, sh, mu, inv, gamma, 3 * sums, 3 * M, 0),
                            R.backward_apply(dy, x, sc, sh, mu, inv, 0, 3 * sums[0], 3 * sums[1], 3 * M, gamma), R.OUT_TOL, 'dx with a fault')
        elif fault == 'res2 ignored':
            R.assert_scaled(bad.apply(x, sc, sh, d['res1'], d['res2'], 1), R.apply(x, sc, sh, d['res1'], d['res2'], 1), R.OUT_TOL, 'y with a fault')
        elif fault == 'mask >=':
            t, tie, above, below = R.tie_data()
            g, gx, g_abs, gx_abs = R.backward_sums(t['dy'], t['x'], t['scale'], t['shift'], t['mean'], t['invstd'], 1)
            R.assert_sums(bad.backward_reduce(t['dy'], t['x'], t['scale'], t['shift'], t['mean'], t['invstd'], 1)[0][0], g,
                          R.sum_bound(M, g_abs), 'sum g with a fault')
        else:
            R.assert_scaled(bad.train_stats(x, gamma, beta, d['mm'], d['mv'])['mean'], ref['mean'], R.STAT_TOL, 'mean with a fault')
