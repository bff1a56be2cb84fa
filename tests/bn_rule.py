"""Training-mode BatchNorm as csrc/train_bn.hip computes it, stated in NumPy float64 (a test helper: no torch in the rule).

Each stage is a function of that stage's OWN fp32 inputs -- the sums of the tensor, the fold of given sums, the apply of a given
scale and shift, the backward of given statistics and sums -- so a later stage is never blamed for an earlier stage's rounding.
The sums are exact (math.fsum); what a float64 accumulation in any order may lose against them is the bound of sum_bound().

The shape table and the seeded data of tests/test_cpu_bn_rule.py and tests/test_gpu_bn_kernels.py live here too, so both
files look at the same cases."""
import math

import numpy as np

DECAY = float(np.float32(0.9))        # the decay the training loop passes, as the float the C ABI receives
EPS = float(np.float32(1e-5))
BN_SPLIT = 4                          # csrc/train_bn.hip: work-groups (= batch slices) per channel in the reductions

# id -> (N, C, H, W); what each one reaches is in the table of tests/test_gpu_bn_kernels.py
SHAPES = {
    'a': (1, 3, 1, 1),
    'b': (3, 5, 1, 1),
    'c': (2, 37, 7, 9),
    'd': (5, 4, 33, 33),
    'e': (300, 2, 6, 10),
    'f': (1100, 2, 6, 10),
    'g': (8, 3, 80, 80),
    'h': (9, 2, 50, 82),
    'i': (4, 130, 6, 10),
    'j': (4, 6, 8, 8),
}


def slices(N):
    """the images [n0, n1) of the BN_SPLIT batch slices (bn_partial_kernel)"""
    per = -(-N // BN_SPLIT)
    return [(min(s * per, N), min(s * per + per, N)) for s in range(BN_SPLIT)]


def _away_from_zero(a):
    """every |value| at least 0.5: a dropped or doubled element moves a sum by at least 0.5"""
    a = a.astype(np.float32)
    small = np.abs(a) < 0.5
    a[small] = np.where(a[small] < 0, np.float32(-0.5), np.float32(0.5))
    return a


def case_data(name):
    """seeded fp32 data of a shape: x, dy, res1, res2 (N, C, H, W); gamma, beta, moving mean / variance (C).  Every channel
    and every image has its own offset and spread, so a wrong index shows."""
    N, C, H, W = SHAPES[name]
    rs = np.random.RandomState(1000 + ord(name))

    def field(off_c, off_n):
        oc, on = rs.uniform(-off_c, off_c, (1, C, 1, 1)), rs.uniform(-off_n, off_n, (N, 1, 1, 1))
        sc, sn = rs.uniform(0.5, 2.0, (1, C, 1, 1)), rs.uniform(0.8, 1.25, (N, 1, 1, 1))
        return _away_from_zero(oc + on + sc * sn * rs.normal(0, 1, (N, C, H, W)))
    d = {'x': field(2.0, 0.5), 'dy': field(0.5, 0.25)}
    d['res1'] = rs.normal(0, 1, (N, C, H, W)).astype(np.float32)
    d['res2'] = rs.normal(0, 1, (N, C, H, W)).astype(np.float32)
    d['gamma'] = rs.uniform(0.5, 1.5, C).astype(np.float32)
    d['beta'] = rs.normal(0, 0.3, C).astype(np.float32)
    d['mm'] = rs.normal(0.2, 0.5, C).astype(np.float32)
    d['mv'] = rs.uniform(0.5, 2.0, C).astype(np.float32)
    return d


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _bc(v):
    """a per-channel vector against (N, C, H, W)"""
    return _f64(v).reshape(1, -1, 1, 1)


def _channel_fsum(t):
    """exact per-channel sums of a float64 (N, C, ...) array, rounded once"""
    C = t.shape[1]
    rows = np.moveaxis(t, 1, 0).reshape(C, -1)
    return np.array([math.fsum(r) for r in rows], dtype=np.float64)


def moments(x):
    """-> (sum x, sum x^2, sum |x|, sum |x^2|) per channel; x^2 of an fp32 value is exact in float64"""
    x = _f64(x)
    sq = x * x
    return _channel_fsum(x), _channel_fsum(sq), _channel_fsum(np.abs(x)), _channel_fsum(sq)


def sum_bound(M, abs_terms):
    """what a float64 accumulation of M terms, in ANY order, may differ from the exact sum: (M - 1) roundings of at most
    2^-53 of the running sum each, and that never exceeds sum |term|; times 2 for the reference's own last rounding."""
    return 2.0 * M * 2.0 ** -53 * _f64(abs_terms)


def fold(s, ss, M, gamma, beta, mm, mv, decay=DECAY, eps=EPS):
    """what the forward pass makes of a channel's (sum x, sum x^2) over M elements -> dict of mean, var (biased, clamped at 0),
    invstd, scale, shift and the new moving averages (the moving variance takes the unbiased one)"""
    s, ss = _f64(s), _f64(ss)
    mean = s / M
    var = np.maximum(ss / M - mean * mean, 0.0)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = _f64(gamma) * invstd
    out = {'mean': mean, 'var': var, 'invstd': invstd, 'scale': scale, 'shift': _f64(beta) - mean * scale}
    if mm is not None:
        out['mm'] = _f64(mm) * decay + mean * (1.0 - decay)
    if mv is not None:
        out['mv'] = _f64(mv) * decay + var * M / max(M - 1, 1) * (1.0 - decay)
    return out


def apply(x, scale, shift, res1=None, res2=None, relu=0):
    y = _f64(x) * _bc(scale) + _bc(shift)
    if relu:
        y = np.maximum(y, 0.0)
    if res1 is not None:
        y = y + _f64(res1)
    if res2 is not None:
        y = y + _f64(res2)
    return y


def masked_gradient(dy, x, scale, shift, relu):
    """g = dy where the forward ReLU passed.  The mask x * scale + shift > 0 in float64 from the fp32 scale and shift is EXACTLY
    the kernel's fmaf(x, scale, shift) > 0: the product of two fp32 values is exact in double, the sum is rounded once (to double
    here, to float there), and a nonzero sum does not round to zero in either format at these magnitudes -- both have the sign
    of the exact value, and both are 0 exactly where it is 0."""
    g = _f64(dy)
    if relu:
        g = np.where(_f64(x) * _bc(scale) + _bc(shift) > 0, g, 0.0)
    return g


def xhat32(x, mean, invstd):
    """the kernel's fp32 expression (x - mean) * invstd: two roundings"""
    d = np.asarray(x, np.float32) - np.asarray(mean, np.float32).reshape(1, -1, 1, 1)
    return (d * np.asarray(invstd, np.float32).reshape(1, -1, 1, 1)).astype(np.float32)


def backward_sums(dy, x, scale, shift, mean, invstd, relu):
    """-> (sum g, sum g xhat, sum |g|, sum |g xhat|) per channel, xhat the kernel's fp32 value; g * xhat, a product of two fp32
    values, is exact in float64, so the terms are the kernel's terms and only the order of the additions is free"""
    g = masked_gradient(dy, x, scale, shift, relu)
    gx = g * _f64(xhat32(x, mean, invstd))
    return _channel_fsum(g), _channel_fsum(gx), _channel_fsum(np.abs(g)), _channel_fsum(np.abs(gx))


def backward_apply(dy, x, scale, shift, mean, invstd, relu, sum_g, sum_gx, count, gamma):
    """dx = gamma invstd (g - sum g / count - xhat sum g xhat / count), xhat in float64 from the fp32 mean and invstd"""
    g = masked_gradient(dy, x, scale, shift, relu)
    xh = (_f64(x) - _bc(mean)) * _bc(invstd)
    return _bc(gamma) * _bc(invstd) * (g - _bc(sum_g) / count - xh * _bc(sum_gx) / count)


# ---- comparisons: (got, reference, bound) -------------------------------------------------------------------------------

def _np(a):
    return a.detach().double().cpu().numpy() if hasattr(a, 'detach') else _f64(a)


def _label(what):
    """report label of a comparison whose bound is not relative to the tensor scale: its `rel` column is error / bound"""
    head, sep, tail = what.partition(' shape ')
    return head + ' [rel = error / bound]' + sep + tail


def assert_sums(got, ref, bound, what):
    """per channel |got - ref| <= bound (absolute, an array); recorded in the parity report as the worst fraction of the bound"""
    from tests import util
    got, ref, bound = _np(got), _f64(ref), _f64(bound)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), '{}: not finite'.format(what)
    frac = float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0))) if err.size else 0.0
    util.REPORT.append((_label(what), float(err.max()), frac, 1.0))
    bad = np.nonzero(err > bound)[0]
    assert bad.size == 0, '{}: channel {} off by {:.3e}, bound {:.3e} ({} channels beyond their bound)'.format(
        what, int(bad[0]), float(err[bad[0]]), float(bound[bad[0]]), bad.size)


def assert_scaled(got, ref, bound, what):
    """max |got - ref| <= bound * max(1, max |ref|): tests.util.assert_close, so the achieved error is in the parity report"""
    from tests import util
    got = _np(got)
    assert np.isfinite(got).all(), '{}: not finite'.format(what)
    return util.assert_close(got, _f64(ref), what, bound)


def assert_relative(got, ref, bound, what):
    """per element |got - ref| <= bound * |ref| (bound an array or a number): relative to the value ITSELF"""
    from tests import util
    got, ref = _np(got), _f64(ref)
    bound = np.broadcast_to(_f64(bound), ref.shape)
    rel = np.abs(got - ref) / np.abs(ref)
    util.REPORT.append((_label(what), float(np.abs(got - ref).max()), float((rel / bound).max()), 1.0))
    bad = np.nonzero(~(rel <= bound))[0]
    assert bad.size == 0, '{}: element {} off by {:.3e} of itself, bound {:.3e}'.format(what, int(bad[0]), float(rel[bad[0]]), float(bound[bad[0]]))


# ---- the checks of one case, against any implementation of the entry points ---------------------------------------------
# `be` restates the C ABI on NumPy arrays (tests/test_gpu_bn_kernels.py: the library; tests/test_cpu_bn_rule.py: a float32
# emulation of the kernels that can be told to be subtly wrong):
#   be.moments(x) -> sums (2, C) float64                          be.stats(x) -> mean, var
#   be.train_stats(x, gamma, beta, mm, mv) / be.fold_moments(sums, count, gamma, beta, mm, mv)
#       -> dict mean, invstd, scale, shift, mm, mv (the moving averages after the call)
#   be.apply(x, scale, shift, res1, res2, relu) -> y
#   be.backward_reduce(dy, x, scale, shift, mean, invstd, relu) -> sums (2, C) float64, dgamma, dbeta
#   be.backward(dy, x, scale, shift, mean, invstd, gamma, relu) -> dx, dgamma, dbeta
#   be.backward_apply(dy, x, scale, shift, mean, invstd, gamma, sums, count, relu) -> dx

STAT_TOL = 1e-6          # mean, variance, invstd, scale, shift, moving averages: of tests/test_gpu_training.py's BatchNorm test
OUT_TOL = 1e-5           # y and dx, relative to the tensor scale: of the same test
STAT_KEYS = ('mean', 'invstd', 'scale', 'shift', 'mm', 'mv')


def check_case(be, name, relu, data=None):
    """every comparison of one shape with the float64 rule; -> the implementation's statistics and backward sums"""
    d = data if data is not None else case_data(name)
    x, dy, gamma, beta = d['x'], d['dy'], d['gamma'], d['beta']
    N, C, H, W = x.shape
    M = N * H * W
    at = ' shape {} relu {}'.format(name, relu)

    s, ss, s_abs, ss_abs = moments(x)
    got = be.moments(x)
    assert_sums(got[0], s, sum_bound(M, s_abs), 'bn moments: sum x' + at)
    assert_sums(got[1], ss, sum_bound(M, ss_abs), 'bn moments: sum x^2' + at)

    ref = fold(s, ss, M, gamma, beta, d['mm'], d['mv'])
    mean, var = be.stats(x)
    assert_scaled(mean, ref['mean'], STAT_TOL, 'bn stats: mean' + at)
    assert_scaled(var, ref['var'], STAT_TOL, 'bn stats: variance' + at)
    assert float(np.min(_np(var))) >= 0.0
    st = be.train_stats(x, gamma, beta, d['mm'], d['mv'])
    folded = be.fold_moments(np.stack([s, ss]), M, gamma, beta, d['mm'], d['mv'])
    for k in STAT_KEYS:
        assert_scaled(st[k], ref[k], STAT_TOL, 'bn train stats: ' + k + at)
        assert_scaled(folded[k], ref[k], STAT_TOL, 'bn fold moments: ' + k + at)

    # from here on the implementation's own fp32 statistics are the inputs of both sides
    sc, sh, mu, inv = st['scale'], st['shift'], st['mean'], st['invstd']
    for r1, r2, which in ((d['res1'], d['res2'], 'two residuals'), (d['res1'], None, 'one residual'), (None, None, 'no residual')):
        assert_scaled(be.apply(x, sc, sh, r1, r2, relu), apply(x, sc, sh, r1, r2, relu), OUT_TOL, 'bn apply, ' + which + at)

    g, gx, g_abs, gx_abs = backward_sums(dy, x, sc, sh, mu, inv, relu)
    bg, bgx = sum_bound(M, g_abs), sum_bound(M, gx_abs)
    sums, dgamma, dbeta = be.backward_reduce(dy, x, sc, sh, mu, inv, relu)
    assert_sums(sums[0], g, bg, 'bn backward reduce: sum g' + at)
    assert_sums(sums[1], gx, bgx, 'bn backward reduce: sum g xhat' + at)
    # the float outputs: the same sums rounded once more
    assert_sums(dbeta, g, bg + 2.0 ** -24 * np.abs(g), 'bn backward reduce: dbeta' + at)
    assert_sums(dgamma, gx, bgx + 2.0 ** -24 * np.abs(gx), 'bn backward reduce: dgamma' + at)

    dx, dgamma, dbeta = be.backward(dy, x, sc, sh, mu, inv, gamma, relu)
    assert_sums(dbeta, g, bg + 2.0 ** -24 * np.abs(g), 'bn backward: dbeta' + at)
    assert_sums(dgamma, gx, bgx + 2.0 ** -24 * np.abs(gx), 'bn backward: dgamma' + at)
    own = _np(sums)
    assert_scaled(dx, backward_apply(dy, x, sc, sh, mu, inv, relu, own[0], own[1], M, gamma), OUT_TOL, 'bn backward: dx' + at)
    # the cross-replica case: three ranks' worth of sums and count, count != N * HW
    dx3 = be.backward_apply(dy, x, sc, sh, mu, inv, gamma, 3.0 * own, 3 * M, relu)
    assert_scaled(dx3, backward_apply(dy, x, sc, sh, mu, inv, relu, 3.0 * own[0], 3.0 * own[1], 3 * M, gamma), OUT_TOL,
                  'bn backward apply, count 3 N HW: dx' + at)
    return st, sums


def tie_data(name='c'):
    """the ReLU tie: the caller's scale = 1 and shift = -2, several x exactly 2.0 (fmaf gives exactly 0 there), and their
    neighbours one ulp above and below 2.0 -> data, positions (flat indices) of the ties / above / below"""
    d = case_data(name)
    x = d['x']
    N, C, H, W = x.shape
    rs = np.random.RandomState(77)
    pos = rs.choice(x.size, 60, replace=False)
    tie, above, below = pos[:20], pos[20:40], pos[40:]
    flat = x.reshape(-1)
    two = np.float32(2.0)
    flat[tie] = two
    flat[above] = np.nextafter(two, np.float32(3.0))
    flat[below] = np.nextafter(two, np.float32(0.0))
    d['scale'], d['shift'] = np.ones(C, np.float32), np.full(C, -2.0, np.float32)
    d['mean'] = rs.normal(0.3, 0.5, C).astype(np.float32)
    d['invstd'] = rs.uniform(0.5, 1.5, C).astype(np.float32)
    return d, tie, above, below


def check_relu_tie(be):
    """strict `>`: on the tie y = 0 + residuals and the gradient is masked, in the sums and in dx; one ulp above passes,
    one ulp below is masked"""
    d, tie, above, below = tie_data()
    x, dy, sc, sh, mu, inv, gamma = d['x'], d['dy'], d['scale'], d['shift'], d['mean'], d['invstd'], d['gamma']
    N, C, H, W = x.shape
    M = N * H * W
    pre = _f64(x).reshape(-1) - 2.0
    assert (pre[tie] == 0).all() and (pre[above] > 0).all() and (pre[below] < 0).all()
    y = _np(be.apply(x, sc, sh, d['res1'], d['res2'], 1))
    r1, r2 = d['res1'].reshape(-1), d['res2'].reshape(-1)
    for p in (tie, below):
        assert np.array_equal(y.reshape(-1)[p], _f64((np.float32(0.0) + r1[p]) + r2[p])), 'y on / below the tie is not 0 + residuals'
    assert_scaled(y, apply(x, sc, sh, d['res1'], d['res2'], 1), OUT_TOL, 'bn relu tie: y')
    g, gx, g_abs, gx_abs = backward_sums(dy, x, sc, sh, mu, inv, 1)
    gm = masked_gradient(dy, x, sc, sh, 1).reshape(-1)
    assert (gm[tie] == 0).all() and (gm[below] == 0).all() and (np.abs(gm[above]) >= 0.5).all()
    sums, dgamma, dbeta = be.backward_reduce(dy, x, sc, sh, mu, inv, 1)
    assert_sums(sums[0], g, sum_bound(M, g_abs), 'bn relu tie: sum g')
    assert_sums(sums[1], gx, sum_bound(M, gx_abs), 'bn relu tie: sum g xhat')
    own = _np(sums)
    ref_dx = backward_apply(dy, x, sc, sh, mu, inv, 1, own[0], own[1], M, gamma)
    dx, _, _ = be.backward(dy, x, sc, sh, mu, inv, gamma, 1)
    assert_scaled(dx, ref_dx, OUT_TOL, 'bn relu tie: dx')
    # on its own, so that the 20 ties are not lost in the maximum over 4662 elements: dx there is the g = 0 value
    for p, what in ((tie, 'on'), (above, 'above'), (below, 'below')):
        assert_scaled(_np(dx).reshape(-1)[p], ref_dx.reshape(-1)[p], OUT_TOL, 'bn relu tie: dx {} the tie'.format(what))
