"""-m gpu: the training-mode BatchNorm kernels (csrc/train_bn.hip) through the C ABI on every code path, each stage against the
float64 rule of tests/bn_rule.py on that stage's own fp32 inputs (tests/test_cpu_bn_rule.py shows that these very checks fail
on a subtly wrong kernel).  Every launch runs twice into NaN-filled outputs and must give the same bits.

| id | N, C, H x W    | reaches                                                                                              |
| a  | 1, 3, 1 x 1    | M = 1: variance 0, the unbiased guard, three empty batch slices                                      |
| b  | 3, 5, 1 x 1    | HW = 1, scalar path, one empty slice                                                                 |
| c  | 2, 37, 7 x 9   | HW = 63 scalar, N < 4                                                                                |
| d  | 5, 4, 33 x 33  | HW = 1089 scalar, two work-groups per plane in the element-wise kernels, slices of 2, 2, 1, 0 images |
| e  | 300, 2, 6 x 10 | 16-byte path, HW / 4 = 15, 75 images per slice: the carry stepping with dn = 68, dp = 4              |
| f  | 1100, 2, 6 x 10| as (e), 4125 float4 per slice: the four-loads-in-flight loop on small planes                         |
| g  | 8, 3, 80 x 80  | HW / 4 = 1600 > 1024 (dn = 0), the four-in-flight loop for some threads only, 7 work-groups per plane|
| h  | 9, 2, 50 x 82  | HW / 4 = 1025, 3 images per slice: the loop boundary (three threads enter it)                        |
| i  | 4, 130, 6 x 10 | C > 64 and no multiple of 64: three blocks in the finish kernels                                     |
| j  | 4, 6, 8 x 8    | every tensor a view one float into a larger allocation: the alignment fallback, reductions included  |
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bn_rule as R
from tests.test_gpu_train_kernels import _twice

pytestmark = pytest.mark.gpu

NAMES = sorted(R.SHAPES)
KEYS = R.STAT_KEYS


def _L():
    from imgcomp_cvpr_amd import _lib
    return _lib


class Device:
    """the ic_bn_* entry points on NumPy arrays (the interface tests/bn_rule.py checks).  off = 1: every float tensor, input
    and output, starts one float into its allocation (4-byte aligned, not 16); the float64 sums start one double in."""

    def __init__(self, cuda, off=0):
        self.cuda, self.off, self.L = cuda, off, _L()
        self.st = self.L.current_stream()

    def put(self, a, dtype=torch.float32):
        if a is None:
            return None
        return self._place(torch.as_tensor(np.ascontiguousarray(a)).to(dtype))

    def nan(self, shape, dtype=torch.float32):
        return self._place(torch.full(tuple(shape), float('nan'), dtype=dtype))

    def _place(self, t):
        if not self.off:
            return t.to(self.cuda)
        buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=self.cuda)
        v = buf[self.off:self.off + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == self.off * t.element_size() and v.is_contiguous()
        return v

    def ws(self, C):
        return torch.empty(self.L.lib.ic_bn_workspace_bytes(C), dtype=torch.uint8, device=self.cuda)

    def _run(self, launch):
        return [t.cpu() for t in _twice(launch)]

    def moments(self, x):
        L, p = self.L, self.L.ptr
        N, C, H, W = x.shape
        xd, ws = self.put(x), self.ws(C)

        def launch():
            sums = self.nan((2, C), torch.float64)
            L.check(L.lib.ic_bn_moments_f32(p(xd), p(sums), N, C, H * W, p(ws), self.st))
            return (sums,)
        return self._run(launch)[0]

    def stats(self, x):
        L, p = self.L, self.L.ptr
        N, C, H, W = x.shape
        xd, ws = self.put(x), self.ws(C)

        def launch():
            mean, var = self.nan((C,)), self.nan((C,))
            L.check(L.lib.ic_bn_stats_f32(p(xd), p(mean), p(var), N, C, H * W, p(ws), self.st))
            return mean, var
        return self._run(launch)

    def train_stats(self, x, gamma, beta, mm, mv):
        L, p = self.L, self.L.ptr
        N, C, H, W = x.shape
        xd, gd, bd, ws = self.put(x), self.put(gamma), self.put(beta), self.ws(C)

        def launch():
            o = [self.nan((C,)) for _ in range(4)]
            m, v = self.put(mm), self.put(mv)
            L.check(L.lib.ic_bn_train_stats_f32(p(xd), p(gd), p(bd), p(m), p(v), R.DECAY, R.EPS, p(o[0]), p(o[1]), p(o[2]), p(o[3]),
                                                N, C, H * W, p(ws), self.st))
            return o + [t for t in (m, v) if t is not None]
        return self._stats_dict(self._run(launch), mm, mv)

    @staticmethod
    def _stats_dict(out, mm, mv):
        d = dict(zip(('mean', 'invstd', 'scale', 'shift'), out[:4]))
        rest = list(out[4:])
        if mm is not None:
            d['mm'] = rest.pop(0)
        if mv is not None:
            d['mv'] = rest.pop(0)
        return d

    def fold_moments(self, sums, count, gamma, beta, mm, mv):
        L, p = self.L, self.L.ptr
        C = len(gamma)
        sd, gd, bd = self.put(sums, torch.float64), self.put(gamma), self.put(beta)

        def launch():
            o = [self.nan((C,)) for _ in range(4)]
            m, v = self.put(mm), self.put(mv)
            L.check(L.lib.ic_bn_train_fold_moments_f32(p(sd), count, p(gd), p(bd), p(m), p(v), R.DECAY, R.EPS, p(o[0]), p(o[1]), p(o[2]),
                                                       p(o[3]), C, self.st))
            return o + [t for t in (m, v) if t is not None]
        return self._stats_dict(self._run(launch), mm, mv)

    def train_forward(self, x, gamma, beta, mm, mv, res1, res2, relu):
        """-> the statistics dict, y"""
        L, p = self.L, self.L.ptr
        N, C, H, W = x.shape
        xd, gd, bd, r1, r2, ws = self.put(x), self.put(gamma), self.put(beta), self.put(res1), self.put(res2), self.ws(C)

        def launch():
            o = [self.nan((C,)) for _ in range(4)]
            m, v, y = self.put(mm), self.put(mv), self.nan(x.shape)
            L.check(L.lib.ic_bn_train_forward_f32(p(xd), p(gd), p(bd), p(m), p(v), R.DECAY, R.EPS, p(o[0]), p(o[1]), p(o[2]), p(o[3]),
                                                  p(r1), p(r2), p(y), N, C, H * W, relu, p(ws), self.st))
            return o + [t for t in (m, v) if t is not None] + [y]
        out = self._run(launch)
        return self._stats_dict(out[:-1], mm, mv), out[-1]

    def apply(self, x, scale, shift, res1, res2, relu):
        L, p = self.L, self.L.ptr
        N, C, H, W = x.shape
        xd, sc, sh, r1, r2 = self.put(x), self.put(scale), self.put(shift), self.put(res1), self.put(res2)

        def launch():
            y = self.nan(x.shape)
            L.check(L.lib.ic_bn_apply_f32(p(xd), p(sc), p(sh), p(r1), p(r2), p(y), N, C, H * W, relu, self.st))
            return (y,)
        return self._run(launch)[0]

    def backward_reduce(self, dy, x, scale, shift, mean, invstd, relu):
        L, p = self.L, self.L.ptr
        N, C, H, W = x.shape
        dyd, xd, ws = self.put(dy), self.put(x), self.ws(C)
        sc, sh, mu, inv = self.put(scale), self.put(shift), self.put(mean), self.put(invstd)

        def launch():
            sums, dgamma, dbeta = self.nan((2, C), torch.float64), self.nan((C,)), self.nan((C,))
            L.check(L.lib.ic_bn_backward_reduce_f32(p(dyd), p(xd), p(sc), p(sh), p(mu), p(inv), p(sums), p(dgamma), p(dbeta), N, C, H * W,
                                                    relu, p(ws), self.st))
            return sums, dgamma, dbeta
        return self._run(launch)

    def backward(self, dy, x, scale, shift, mean, invstd, gamma, relu):
        L, p = self.L, self.L.ptr
        N, C, H, W = x.shape
        dyd, xd, gd, ws = self.put(dy), self.put(x), self.put(gamma), self.ws(C)
        sc, sh, mu, inv = self.put(scale), self.put(shift), self.put(mean), self.put(invstd)

        def launch():
            dx, dgamma, dbeta = self.nan(x.shape), self.nan((C,)), self.nan((C,))
            L.check(L.lib.ic_bn_backward_f32(p(dyd), p(xd), p(sc), p(sh), p(mu), p(inv), p(gd), p(dx), p(dgamma), p(dbeta), N, C, H * W,
                                             relu, p(ws), self.st))
            return dx, dgamma, dbeta
        return self._run(launch)

    def backward_apply(self, dy, x, scale, shift, mean, invstd, gamma, sums, count, relu):
        L, p = self.L, self.L.ptr
        N, C, H, W = x.shape
        dyd, xd, gd, sd = self.put(dy), self.put(x), self.put(gamma), self.put(sums, torch.float64)
        sc, sh, mu, inv = self.put(scale), self.put(shift), self.put(mean), self.put(invstd)

        def launch():
            dx = self.nan(x.shape)
            L.check(L.lib.ic_bn_backward_apply_f32(p(dyd), p(xd), p(sc), p(sh), p(mu), p(inv), p(gd), p(sd), count, p(dx), N, C, H * W,
                                                   relu, self.st))
            return (dx,)
        return self._run(launch)[0]


def _device(cuda, name):
    return Device(cuda, off=1 if name == 'j' else 0)


def _same(a, b, what):
    assert bool(torch.isfinite(a).all()), what + ': not finite'
    assert torch.equal(a, b), what + ': other bits'


# ---- every shape against the float64 rule ---------------------------------------------------------------------------------

@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('relu', [0, 1])
def test_every_entry_point_against_the_float64_rule(cuda, name, relu):
    """sums within the worst case of a float64 accumulation in any order (computed from the data), float dgamma / dbeta that
    plus one fp32 rounding, statistics and moving averages within 1e-6, y (two, one, no residual) and dx (count N HW and the
    cross-replica count 3 N HW) within 1e-5 of the float64 evaluation on the device's own statistics and sums"""
    R.check_case(_device(cuda, name), name, relu)


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('relu', [0, 1])
def test_fused_forward_is_stats_then_apply_bit_for_bit(cuda, name, relu):
    """ic_bn_train_forward_f32 == ic_bn_train_stats_f32 followed by ic_bn_apply_f32, every output and both moving averages"""
    be, d = _device(cuda, name), R.case_data(name)
    fused, y = be.train_forward(d['x'], d['gamma'], d['beta'], d['mm'], d['mv'], d['res1'], d['res2'], relu)
    st = be.train_stats(d['x'], d['gamma'], d['beta'], d['mm'], d['mv'])
    y2 = be.apply(d['x'], st['scale'].numpy(), st['shift'].numpy(), d['res1'], d['res2'], relu)
    for k in KEYS:
        _same(fused[k], st[k], 'fused forward: ' + k)
    _same(y, y2, 'fused forward: y')


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('relu', [0, 1])
def test_one_rank_split_path_is_the_fused_path_bit_for_bit(cuda, name, relu):
    """moments -> fold == ic_bn_train_stats_f32, and reduce -> apply == ic_bn_backward_f32, with count = N HW"""
    be, d = _device(cuda, name), R.case_data(name)
    x, dy, gamma = d['x'], d['dy'], d['gamma']
    N, C, H, W = x.shape
    st = be.train_stats(x, gamma, d['beta'], d['mm'], d['mv'])
    split = be.fold_moments(be.moments(x).numpy(), N * H * W, gamma, d['beta'], d['mm'], d['mv'])
    for k in KEYS:
        _same(split[k], st[k], 'split forward: ' + k)
    s = [st[k].numpy() for k in ('scale', 'shift', 'mean', 'invstd')]
    dx, dgamma, dbeta = be.backward(dy, x, s[0], s[1], s[2], s[3], gamma, relu)
    sums, dgamma2, dbeta2 = be.backward_reduce(dy, x, s[0], s[1], s[2], s[3], relu)
    dx2 = be.backward_apply(dy, x, s[0], s[1], s[2], s[3], gamma, sums.numpy(), N * H * W, relu)
    _same(dx2, dx, 'split backward: dx')
    _same(dgamma2, dgamma, 'split backward: dgamma')
    _same(dbeta2, dbeta, 'split backward: dbeta')


@pytest.mark.parametrize('relu', [0, 1])
def test_misaligned_tensors_give_the_aligned_bits(cuda, relu):
    """shape (j): the element-wise kernels on tensors one float off 16-byte alignment, given the same scale, shift and sums as the
    aligned tensors (the reductions take the scalar loop there, another order of additions: tests above, within their bounds)"""
    d = R.case_data('j')
    x, dy, gamma = d['x'], d['dy'], d['gamma']
    N, C, H, W = x.shape
    al, mis = Device(cuda), Device(cuda, off=1)
    st = al.train_stats(x, gamma, d['beta'], d['mm'], d['mv'])
    s = [st[k].numpy() for k in ('scale', 'shift', 'mean', 'invstd')]
    for r1, r2 in ((d['res1'], d['res2']), (d['res1'], None), (None, None)):
        _same(mis.apply(x, s[0], s[1], r1, r2, relu), al.apply(x, s[0], s[1], r1, r2, relu), 'misaligned apply')
    sums = al.backward_reduce(dy, x, s[0], s[1], s[2], s[3], relu)[0].numpy()
    for count, k in ((N * H * W, 1.0), (3 * N * H * W, 3.0)):
        _same(mis.backward_apply(dy, x, s[0], s[1], s[2], s[3], gamma, k * sums, count, relu),
              al.backward_apply(dy, x, s[0], s[1], s[2], s[3], gamma, k * sums, count, relu), 'misaligned backward apply')


# ---- against torch's float64 autograd: an independent statement of the whole layer -------------------------------------------

@pytest.mark.parametrize('name', ['c', 'd', 'g', 'i'])
def test_layer_against_torch_float64_autograd(cuda, name):
    """forward output at relu 0 and 1, backward at relu 0, within the bounds of test_bn_train_forward_backward (1e-5; dgamma and
    dbeta too).  The backward with ReLU is checked through the exact mask of the rule: a float64 mask from float64 statistics may
    differ on elements within rounding of zero.  Nothing is excluded from any comparison."""
    be, d = _device(cuda, name), R.case_data(name)
    x, dy, gamma, beta = d['x'], d['dy'], d['gamma'], d['beta']
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), requires_grad=g)
    for relu in (0, 1):
        xt, gt, bt = t(x, True), t(gamma, True), t(beta, True)
        rm, rv = t(d['mm']), t(d['mv'])
        y = F.batch_norm(xt, rm, rv, gt, bt, training=True, momentum=1.0 - R.DECAY, eps=R.EPS)
        if relu:
            y = F.relu(y)
        y = y + t(d['res1']) + t(d['res2'])
        st, yd = be.train_forward(x, gamma, beta, d['mm'], d['mv'], d['res1'], d['res2'], relu)
        at = ' shape {} relu {}'.format(name, relu)
        R.assert_scaled(yd, y.detach().numpy(), R.OUT_TOL, 'bn vs torch autograd: y' + at)
        R.assert_scaled(st['mm'], rm.numpy(), R.STAT_TOL, 'bn vs torch autograd: moving mean' + at)
        R.assert_scaled(st['mv'], rv.numpy(), R.STAT_TOL, 'bn vs torch autograd: moving variance' + at)
        if relu == 0:
            y.backward(t(dy))
            s = [st[k].numpy() for k in ('scale', 'shift', 'mean', 'invstd')]
            dx, dgamma, dbeta = be.backward(dy, x, s[0], s[1], s[2], s[3], gamma, 0)
            R.assert_scaled(dx, xt.grad.numpy(), R.OUT_TOL, 'bn vs torch autograd: dx' + at)
            R.assert_scaled(dgamma, gt.grad.numpy(), R.OUT_TOL, 'bn vs torch autograd: dgamma' + at)
            R.assert_scaled(dbeta, bt.grad.numpy(), R.OUT_TOL, 'bn vs torch autograd: dbeta' + at)


# ---- constructed cases ---------------------------------------------------------------------------------------------------------

def test_relu_tie_is_masked(cuda):
    """scale = 1, shift = -2 and x exactly 2.0: fmaf gives exactly 0, y = 0 + residuals, the gradient is masked there in the
    sums and in dx (the comparison is a strict >); one ulp above passes, one ulp below does not"""
    R.check_relu_tie(Device(cuda))


def test_constant_channel(cuda):
    """one channel all 1.5: variance within 1e-6 of 0 and not negative, invstd within 1e-6 relative of 1 / sqrt(eps), finite y, dx"""
    be, d = Device(cuda), R.case_data('c')
    x = d['x']
    x[:, 5] = np.float32(1.5)
    mean, var = be.stats(x)
    assert float(mean[5]) == 1.5
    assert 0.0 <= float(var[5]) <= 1e-6
    st, y = be.train_forward(x, d['gamma'], d['beta'], d['mm'], d['mv'], d['res1'], d['res2'], 1)
    R.assert_relative(st['invstd'][5:6], np.array([1.0 / np.sqrt(R.EPS)]), 1e-6, 'bn constant channel: invstd')
    assert bool(torch.isfinite(y).all()) and all(bool(torch.isfinite(st[k]).all()) for k in KEYS)
    s = [st[k].numpy() for k in ('scale', 'shift', 'mean', 'invstd')]
    R.assert_scaled(y, R.apply(x, s[0], s[1], d['res1'], d['res2'], 1), R.OUT_TOL, 'bn constant channel: y')
    dx, dgamma, dbeta = be.backward(d['dy'], x, s[0], s[1], s[2], s[3], d['gamma'], 1)
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dgamma).all()) and bool(torch.isfinite(dbeta).all())


def test_variance_under_cancellation(cuda):
    """x ~ N(30, 0.1) at shape (g): E[x^2] is 90 000 times the variance.  The variance is checked relative to ITSELF; the bound,
    from the data: the two float64 sums are off by at most M 2^-53 of themselves, which E[x^2] / var amplifies, and the float
    result is rounded once; times 2."""
    be, d = Device(cuda), R.case_data('g')
    N, C, H, W = R.SHAPES['g']
    M = N * H * W
    x = np.random.RandomState(30).normal(30.0, 0.1, (N, C, H, W)).astype(np.float32)
    s, ss, _, _ = R.moments(x)
    ref = R.fold(s, ss, M, d['gamma'], d['beta'], d['mm'], d['mv'])
    bound = 2.0 * (M * 2.0 ** -53 * (ss / M) / ref['var'] + 2.0 ** -23)
    assert float(bound.max()) < 2e-6 and float((ss / M / ref['var']).min()) > 5e4
    mean, var = be.stats(x)
    R.assert_relative(var, ref['var'], bound, 'bn cancellation: variance relative to itself')
    R.assert_scaled(mean, ref['mean'], R.STAT_TOL, 'bn cancellation: mean')
    st, y = be.train_forward(x, d['gamma'], d['beta'], d['mm'], d['mv'], d['res1'], None, 1)
    R.assert_scaled(y, R.apply(x, st['scale'].numpy(), st['shift'].numpy(), d['res1'], None, 1), R.OUT_TOL, 'bn cancellation: y')


@pytest.mark.parametrize('with_mean,with_var', [(0, 0), (1, 0), (0, 1)])
def test_null_moving_averages(cuda, with_mean, with_var):
    """moving_mean / moving_var are optional: without them the statistics (and y) keep their bits, and the one that is given is
    updated as when both are -- in all three entry points that take them"""
    be, d = Device(cuda), R.case_data('c')
    x, gamma, beta = d['x'], d['gamma'], d['beta']
    N, C, H, W = x.shape
    mm, mv = (d['mm'] if with_mean else None), (d['mv'] if with_var else None)
    full = be.train_stats(x, gamma, beta, d['mm'], d['mv'])
    sums = be.moments(x).numpy()
    full_fused, full_y = be.train_forward(x, gamma, beta, d['mm'], d['mv'], d['res1'], d['res2'], 1)
    part_fused, part_y = be.train_forward(x, gamma, beta, mm, mv, d['res1'], d['res2'], 1)
    _same(part_y, full_y, 'null moving averages: y')
    for what, part in (('train stats', be.train_stats(x, gamma, beta, mm, mv)), ('train forward', part_fused),
                       ('fold moments', be.fold_moments(sums, N * H * W, gamma, beta, mm, mv))):
        assert sorted(part) == sorted(['mean', 'invstd', 'scale', 'shift'] + ['mm'] * with_mean + ['mv'] * with_var)
        for k in part:
            _same(part[k], full[k], 'null moving averages, {}: {}'.format(what, k))
