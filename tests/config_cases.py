"""Configurations off the few that every other GPU test builds (a test helper: no device code of its own).
tests/test_gpu_config_space.py runs the device on them, tests/test_cpu_config_cases.py checks, with the oracle alone, the conditions
that keep those comparisons from passing vacuously.

The library takes arch_param_B, num_chan_bn, num_centers, heatmap and normalization as free parameters, and the config grammar
allows them (ae_configs/base: `constrain normalization :: OFF, FIXED`, B = 3, C = 3 * 8 * 8); the other GPU tests build cvpr/low,
med and hi only: C in {32, 64}, B = 5, FIXED, L = 6 on the whole-network path.  Each case here is cvpr/med + res_shallow with
overrides, H_target = 0.5 and distortion_to_minimize = mse as in tests/step_cases.py:

  id             normalization  C    B  L   heatmap  to_bn out  reaches
  norm_off       OFF            32   5  6   yes      33         builtin_norm 0 / 4 of the edge kernels, nothing else changed
  c16_b1_l8      FIXED          16   1  8   yes      17         ragged single MFMA channel tile, direct from_bn, one block
  c8_b0_l2_nohm  OFF            8    0  2   no       8          final block only, ic_quantize_f32, OFF combined
  c96_b3_l16     FIXED          96   3  16  yes      97         conv_mfma_x1_kernel with three tiles, ae_configs/base's B, largest L
  c48_b3_nohm    FIXED          48   3  6   no       48         plain MFMA kernel, ragged second channel tile
  base_c192_b3   FIXED          192  3  6   yes      193        ae_configs/base's sizes: to_bn beyond the matrix-core form

Variables: weights.synthetic_weights of the case's configuration; under OFF with the fixed normalisation folded into h1 and h13
(step_cases.fold_fixed_normalization: the plain ones are degenerate on 0 .. 255 input).  Images: weights.synthetic_image 'natural';
for inference (2, 3, 32, 32) -- bottleneck 4 x 4, 3x3 maps 8 x 8, which the F(4x4)-over-phases form of h2 / h12 accepts -- and
(1, 3, 16, 24) -- 3x3 maps 4 x 6, narrower than an F(4x4) tile row and refused by the phase form; base_c192_b3 runs inference on
(1, 3, 16, 16).  The training step runs on (2, 3, 32, 64): see STEP_SHAPE.  One seed per case, admitted by tests/test_cpu_config_cases.py.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from tests import step_cases as S
from tests.util import HEATMAP_RTOL

Config = namedtuple('Config', 'id normalization C B L heatmap to_bn seed step shapes')

SQUARE, NARROW, TINY = (2, 3, 32, 32), (1, 3, 16, 24), (1, 3, 16, 16)
# a training step: 3x3 maps of 8 x 16 = one 2 x 8-tile segment per map, all 16 tiles of it present -- the smallest batch that passes
# TrainGraph's half-full rule, so that wino4=True runs the F(4x4) forward with the BatchNorm sums and the F(4x4) data gradient
# (the square image's 8 x 8 maps fill a quarter of their segment and would stay on F(2x2) in either mode)
STEP_SHAPE = (2, 3, 32, 64)

TABLE = (
    Config('norm_off', 'OFF', 32, 5, 6, True, 33, 1, True, (SQUARE, NARROW)),
    Config('c16_b1_l8', 'FIXED', 16, 1, 8, True, 17, 1, True, (SQUARE, NARROW)),
    Config('c8_b0_l2_nohm', 'OFF', 8, 0, 2, False, 8, 1, True, (SQUARE, NARROW)),
    Config('c96_b3_l16', 'FIXED', 96, 3, 16, True, 97, 1, True, (SQUARE, NARROW)),
    Config('c48_b3_nohm', 'FIXED', 48, 3, 6, False, 48, 1, False, (SQUARE, NARROW)),
    Config('base_c192_b3', 'FIXED', 192, 3, 6, True, 193, 1, False, (TINY,)),
)
BY_ID = {c.id: c for c in TABLE}
INFERENCE = [(c, shape) for c in TABLE for shape in c.shapes]
STEP_MODES = (False, True)


def shape_id(shape):
    return 'x'.join(str(v) for v in shape)


def inference_id(cs):
    return '{}-{}'.format(cs[0].id, shape_id(cs[1]))


def overrides(c):
    return (('normalization', c.normalization), ('num_chan_bn', c.C), ('arch_param_B', c.B), ('num_centers', c.L), ('heatmap', c.heatmap))


def case(c, shape=STEP_SHAPE):
    """the configuration as a case of tests/step_cases.py (its configs / weights / image / oracle helpers take it)"""
    maps = (shape[2] // 4, shape[3] // 4)
    return S.Case(c.id, tuple(shape), 'mse', c.seed, maps, S.segments(*maps)[0], STEP_MODES, overrides(c))


STEP_CASES = tuple(case(c) for c in TABLE if c.step)
STEP_CASE_MODES = [(sc, m) for sc in STEP_CASES for m in sc.modes]


def heatmap_rtol(c):
    """tests/util.py derives HEATMAP_RTOL = 1e-4 from the C / 4 amplification of z0's error by sigmoid(z0) * C at C <= 64: the
    bound grows with C beyond that, and with nothing else"""
    return HEATMAP_RTOL * max(1.0, c.C / 64.0)


# ---- the inference oracle, once per (case, shape, dtype) per process: shared, read-only ---------------------------------------------

Reference = namedtuple('Reference', 'x enc x_out bits')


@functools.lru_cache(maxsize=None)
def reference(c, shape, dtype=torch.float64):
    """oracle.encode of the case's image, oracle.decode of ITS qhard, oracle.bitcost of its (qhard, symbols) with pad = centers[0]"""
    from oracle import oracle as O
    torch.set_num_threads(16)
    sc = case(c, shape)
    w, cfg = S.weights(sc), S.configs(sc)[0].as_dict()
    x = S.image(sc)
    with torch.no_grad():
        enc = O.encode(torch.as_tensor(x).to(dtype), w, cfg)
        x_out = O.decode(enc.qhard, w, cfg)
        bits, _ = O.bitcost(enc.qhard, enc.symbols, w, float(S.centers(sc)[0]))
    return Reference(x, enc, x_out, bits)


# normalization = OFF decodes through the clip-only epilogue of h13 (builtin_norm = 4); the cases' own x_out never reaches the clip's
# edges (test_cpu_config_cases asserts as much), so that branch gets a decoder input of its own: N(0, sigma) noise, RandomState(7),
# with sigma per case such that the float64 oracle's x_out sits on BOTH edges and mostly between them (asserted on the CPU).
CLIP_PROBE_SIGMA = {'norm_off': 16.0, 'c8_b0_l2_nohm': 256.0}


@functools.lru_cache(maxsize=None)
def clip_probe(c, shape):
    """-> (q float32 numpy (N, C, H/8, W/8), the float64 oracle's decode of it)"""
    from oracle import oracle as O
    sc = case(c, shape)
    N, _, H, W = shape
    q = np.random.RandomState(7).normal(0, CLIP_PROBE_SIGMA[c.id], (N, c.C, H // 8, W // 8)).astype(np.float32)
    with torch.no_grad():
        x_out = O.decode(torch.as_tensor(q).double(), S.weights(sc), S.configs(sc)[0].as_dict())
    return q, x_out


def edge_share(x_out):
    """share of x_out sitting on the clip's edges"""
    return float(((x_out <= 0) | (x_out >= 255)).double().mean())


def symbol_shares(symbols, L):
    return np.bincount(np.asarray(symbols).reshape(-1), minlength=L) / float(np.asarray(symbols).size)
