"""Cases and helpers for the whole-step gradient parity tests with the DISCRETE DECISIONS of the step forced (a test helper: no device
code of its own).  tests/test_gpu_step_decisions.py runs the device's step on them, tests/test_cpu_step_cases.py checks the table and
the helpers themselves.

Why.  A training step takes discrete decisions -- the ReLU signs of h1, h2, every conv1 of the residual blocks (not the final
blocks'), from_bn and h12, the quantiser's symbols, the importance map's clip to [0, 1] and x_out's clip to [0, 255].  The fp32 device
step and the float64 oracle each take their own; where ONE ReLU sign differs, training-mode BatchNorm over 70 layers with synthetic
weights moves the step's gradients by 5e-3 .. 1.3e-1 of their scale, while the arithmetic agrees to a few 1e-6 (parity
section).  So the gradients are compared with the float64 oracle evaluated AT THE DEVICE'S DECISIONS
(oracle.train_oracle.train_loss(decisions=...)), and every decision that differs from the oracle's own must sit inside the rounding
band of its threshold (in_band).

The cases are small enough for the float64 oracle (about a second) and, with TrainGraph.WINO4_MIN_WORKGROUPS lowered on the
instance, run the SHIPPED path of the 3x3 layers -- F(4x4) forward with the BatchNorm sums in its epilogue, F(4x4) data gradient --
which the default threshold of 160 work-groups keeps from every other small step test (the cases take 8, 8 and 12).
All: cvpr/med + res_shallow, H_target = 0.5 (the rate term active), synthetic weights; the 3x3 layers see maps of H/4 x W/4.

  id      batch        distortion   3x3 maps   F(4x4) segments
  wide    2x3x32x160   mse          8 x 40     1 x 16, 10 of 16 tiles per segment row: the default 160 x 160 crops' geometry
  ragged  2x3x48x128   mse          12 x 32    2 x 8, 3 tile rows in 2-row segments
  msssim  3x3x64x64    ms_ssim      16 x 16    2 x 8, half full (the HIP MS-SSIM distortion; W <= H as its plan asks at this size)
One image seed per case: seed 1 for all three (admitted by test_cpu_step_cases.test_fp32_oracle_meets_float64_at_forced_decisions).

A case may carry overrides of the autoencoder config (tests/config_cases.py: other B, C, L, no importance map, normalization = OFF);
the helpers below take the case for everything that depends on them -- the variables, the centres, and the counts of gradients, ReLU
layers and residual layers (219 / 34 / 64 for the table above).
"""
import functools
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from tests.util import _boundary_margin, rel_err, true_rel_err

GTOL = 2e-4                       # every gradient of a small step, relative to the tensor scale (tests/test_gpu_training.py)
MAX_DIFFERING = 1e-5              # share of all decisions that may differ from the float64 oracle's own (CPU runs: <= 2 of 3.6 M)
WINO4_MODES = (False, 'fwd', 'bwd', True)

# overrides: ((key, value), ...) set on the autoencoder config after cvpr/med is parsed (tests/config_cases.py); empty for the table below
Case = namedtuple('Case', 'id shape distortion seed maps segments modes overrides', defaults=((),))

CASES = (
    Case('wide', (2, 3, 32, 160), 'mse', 1, (8, 40), '1x16', WINO4_MODES),
    Case('ragged', (2, 3, 48, 128), 'mse', 1, (12, 32), '2x8', (False, True)),
    Case('msssim', (3, 3, 64, 64), 'ms_ssim', 1, (16, 16), '2x8', (False, True)),
)
BY_ID = {c.id: c for c in CASES}
CASE_MODES = [(c, m) for c in CASES for m in c.modes]


def case_mode_id(cm):
    return '{}-wino4_{}'.format(cm[0].id, cm[1])


# ---- the table's geometry, restated (csrc/conv3x3_wino4.hip: w4_segments / w4_seg2, TrainGraph._pack_all_3x3) ----------------------

def segments(H, W):
    """-> (segment shape, segments per map): 16 tiles as 1 x 16 or 2 x 8, whichever covers the map with fewer (a tie keeps 1 x 16)"""
    th, tw = -(-H // 4), -(-W // 4)
    s1, s2 = th * (-(-tw // 16)), (-(-th // 2)) * (-(-tw // 8))
    return ('2x8', s2) if s2 < s1 else ('1x16', s1)


def workgroups(N, H, W):
    return 2 * N * segments(H, W)[1]


def half_full(N, H, W):
    """the rule of TrainGraph._pack_all_3x3 that stays: at least half of the segments' tiles exist"""
    tiles = N * (-(-H // 4)) * (-(-W // 4))
    return 2 * tiles >= 8 * workgroups(N, H, W)


# ---- configuration, variables, image ---------------------------------------------------------------------------------------------

def configs(case):
    """fresh config objects (a graph keeps the ones it is given)"""
    from imgcomp_cvpr_amd import config_parser as cp
    ae, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'med'))
    pc, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    ae.distortion_to_minimize = case.distortion
    ae.H_target = 0.5
    for key, value in case.overrides:
        setattr(ae, key, value)
    return ae, pc


def fold_fixed_normalization(w):
    """normalization = OFF: the plain synthetic variables are degenerate on 0 .. 255 input (nearly all symbols in one bin, x_out
    far below the image), so the FIXED normalisation is folded into the edge layers IN PLACE -- with m, s the means of the three
    channel means and standard deviations of oracle.norm_consts:  h1: weights /= s, moving_mean += (m / s) sum_{ky,kx,ci} w;
    h13: gamma *= s, beta = beta s + m.  (Exact for an interior pixel of a grey image; it only shapes the synthetic statistics.)"""
    from oracle import oracle as O
    mean, std = O.norm_consts(torch.float64)
    m, s = float(mean.mean()), float(std.mean())
    h1, h13 = 'autoencoder/encoder/h1', 'autoencoder/decoder/h13'
    k = np.asarray(w[h1 + '/weights'], np.float64)
    w[h1 + '/weights'] = (k / s).astype(np.float32)
    w[h1 + '/BatchNorm/moving_mean'] = (np.asarray(w[h1 + '/BatchNorm/moving_mean'], np.float64) + (m / s) * k.sum(axis=(0, 1, 2))).astype(np.float32)
    w[h13 + '/BatchNorm/gamma'] = (np.asarray(w[h13 + '/BatchNorm/gamma'], np.float64) * s).astype(np.float32)
    w[h13 + '/BatchNorm/beta'] = (np.asarray(w[h13 + '/BatchNorm/beta'], np.float64) * s + m).astype(np.float32)
    return w


@functools.lru_cache(maxsize=None)
def _weights_for(overrides):
    from imgcomp_cvpr_amd import weights as W
    ae, pc = configs(CASES[0]._replace(overrides=overrides))
    w = W.synthetic_weights(ae, pc)
    return fold_fixed_normalization(w) if ae.normalization == 'OFF' else w


def weights(case=None):
    """the synthetic variables of the case's configuration, the fixed normalisation folded in where the case switches it OFF (they
    do not depend on the distortion or H_target: one set per set of overrides; shared, read-only).  None: the table's own."""
    return _weights_for(case.overrides if case is not None else ())


def centers(case=None):
    return np.asarray(weights(case)['autoencoder/encoder/centers'], np.float64)


# ---- what a step of a configuration holds, from B, the importance map and the parameter list ----------------------------------------

def relu_layers(case):
    """layers whose ReLU sign is a decision: h1, h2, from_bn, h12 and conv1 of the 3 B residual blocks per side (not the final blocks')"""
    return 4 + 6 * int(configs(case)[0].arch_param_B)


def residual_layers(case):
    """3x3 128 -> 128 layers: (6 B + 2) per side"""
    return 2 * (6 * int(configs(case)[0].arch_param_B) + 2)


def gradients(case):
    """trainable variables = the parameter list without BatchNorm's moving statistics; restated from the layer count: {filter,
    gamma, beta} of the residual layers and the six edge layers, the centres, {filter, bias} of the context model's four layers"""
    n = sum(1 for name in weights(case) if 'moving_' not in name)
    assert n == 3 * (residual_layers(case) + 6) + 1 + 2 * 4, n
    return n


def decision_kinds(case):
    hm = {'heatmap_low', 'heatmap_high'} if bool(configs(case)[0].heatmap) else set()
    return {'symbols', 'relu', 'x_out_low', 'x_out_high'} | hm


def image(case, seed=None):
    from imgcomp_cvpr_amd import weights as W
    return W.synthetic_image(case.shape, 'natural', case.seed if seed is None else seed)


# ---- the oracle -----------------------------------------------------------------------------------------------------------------

def oracle(case, dtype=torch.float64, decisions=None, seed=None):
    """one evaluation of oracle.train_oracle.train_loss with its backward -> (total, comps, {name: gradient}), all detached"""
    from oracle import train_oracle as T
    torch.set_num_threads(16)
    ae, pc = configs(case)
    total, comps, p = T.train_loss(image(case, seed), weights(case), ae.as_dict(), pc.as_dict(), dtype, decisions=decisions)
    total.backward()
    comps = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in comps.items()}
    return total.detach(), comps, OrderedDict((n, t.grad) for n, t in p.items() if t.grad is not None)


@functools.lru_cache(maxsize=None)
def unforced(case):
    """the float64 oracle at its own decisions: once per case per process, shared and left unchanged"""
    return oracle(case)


def worst_gradient_error(got, ref):
    """-> (name, error relative to the reference gradient's own scale max|ref|, no clamp at 1) of the worst of ALL gradients"""
    assert set(got) == set(ref), set(got) ^ set(ref)
    return max(((n, true_rel_err(got[n], ref[n])) for n in ref), key=lambda t: t[1])


# ---- one evaluation's decisions and the values they were taken on ("a side") ----------------------------------------------------
# {'decisions': the structure train_loss takes, CPU tensors; 'relu_out': {scope: the layer's activated output}; 'z', 'heatmap', 'x_out'}

def oracle_side(comps):
    """an oracle evaluation (e.g. the float32 one) seen as the side under test"""
    return {'decisions': comps['decisions'], 'relu_out': {s: torch.relu(v) for s, v in comps['relu_pre'].items()},
            'z': comps['z'], 'heatmap': comps['heatmap'], 'x_out': comps['x_out']}


def device_decisions(g, x):
    """runs g.forward_backward(x) (a TrainGraph, x on its device) -> (its scalars, the side, how many 3x3 layers
    _conv3x3_with_stats served).  Instance-level wrappers record every relu=True call of g._cba_fwd and count the non-None returns of
    g._conv3x3_with_stats; the clips and the symbols are read off g.last.  Nothing of TrainGraph changes."""
    relu_out, served = OrderedDict(), [0]
    cba, with_stats = g._cba_fwd, g._conv3x3_with_stats

    def cba_recording(scope, x_, relu, *args, **kwargs):
        y = cba(scope, x_, relu, *args, **kwargs)
        if relu:
            assert scope not in relu_out
            relu_out[scope] = y
        return y

    def with_stats_counting(l, x_):
        r = with_stats(l, x_)
        served[0] += r is not None
        return r
    g._cba_fwd, g._conv3x3_with_stats = cba_recording, with_stats_counting
    try:
        out = g.forward_backward(x)
        torch.cuda.synchronize()
    finally:
        del g._cba_fwd, g._conv3x3_with_stats
    last = {k: (v.detach().cpu() if v is not None else None) for k, v in g.last.items()}
    relu_out = OrderedDict((s, y.detach().cpu()) for s, y in relu_out.items())
    dec = {'symbols': last['symbols'], 'relu': OrderedDict((s, y > 0) for s, y in relu_out.items()),
           'x_out_low': last['x_out'] == 0, 'x_out_high': last['x_out'] == 255}
    if last['heatmap'] is not None:
        dec['heatmap_low'], dec['heatmap_high'] = last['heatmap'] == 0, last['heatmap'] == 1
    side = {'decisions': dec, 'relu_out': relu_out, 'z': last['z'], 'heatmap': last['heatmap'], 'x_out': last['x_out'], 'bc': last['bc']}
    return out, side, served[0]


def _max_abs(a, b):
    return float((a.double() - b.double()).abs().max())


def in_band(side, ref, case=None):
    """side: the decisions under test; ref: the comps of the UNFORCED float64 oracle; case: whose centres (None: the table's).
    Every decision of `side` that differs from the oracle's own must sit inside the rounding band of its threshold:
      ReLU sign     |pre64| <= 2 max|y_side - relu(pre64)| over its layer
      symbol        the rule of tests/test_gpu_network.py: no flip where _boundary_margin(z64) > 2 max|z_side - z64| + 1e-12
      heatmap clip  |u64 - 0| resp. |u64 - 1| <= 2 max|heatmap_side - heatmap64|        (u64 = sigmoid(.) C - c before the clip)
      x_out clip    |pre64 - 0| resp. |pre64 - 255| <= 2 max|x_out_side - x_out64|
    -> counts: the differing decisions per kind, 'differing' (their sum), 'total' (all decisions: ReLU elements, symbols, heatmap
    and x_out elements) and 'out_of_band' (differing decisions outside their band: a test asserts 0)."""
    d, r = side['decisions'], ref['decisions']
    counts = OrderedDict((k, 0) for k in ('relu', 'symbols', 'heatmap', 'x_out', 'differing', 'total', 'out_of_band'))
    assert list(d['relu']) == list(r['relu']), 'the two sides took their ReLU decisions in other layers'
    for scope, own in r['relu'].items():
        pre = ref['relu_pre'][scope].double()
        diff = d['relu'][scope] != own
        band = 2 * _max_abs(side['relu_out'][scope], torch.relu(pre))
        counts['relu'] += int(diff.sum())
        counts['total'] += diff.numel()
        counts['out_of_band'] += int((diff & (pre.abs() > band)).sum())
    flips = (d['symbols'] != r['symbols']).numpy()
    margin = _boundary_margin(ref['z'].double().numpy(), centers(case))
    counts['symbols'] = int(flips.sum())
    counts['total'] += flips.size
    counts['out_of_band'] += int(np.sum(flips & (margin > 2 * _max_abs(side['z'], ref['z']) + 1e-12)))
    clips = [('x_out', ref['x_out_pre'], 0.0, 255.0)]
    if ref['heatmap'] is not None:
        clips.append(('heatmap', ref['heatmap_pre'], 0.0, 1.0))
    for kind, pre, lo, hi in clips:
        pre = pre.double()
        band = 2 * _max_abs(side[kind], ref[kind])
        for which, edge in (('low', lo), ('high', hi)):
            diff = d['{}_{}'.format(kind, which)] != r['{}_{}'.format(kind, which)]
            counts[kind] += int(diff.sum())
            counts['out_of_band'] += int((diff & ((pre - edge).abs() > band)).sum())
        counts['total'] += pre.numel()
    counts['differing'] = counts['relu'] + counts['symbols'] + counts['heatmap'] + counts['x_out']
    return counts
