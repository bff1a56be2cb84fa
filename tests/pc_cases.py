"""Cases for the parity tests of the context model's forward pass (csrc/probclass.hip): weights and symbol volumes per (k, L)
whose channels are all live, and the float64 oracle's answer for them (a test helper: no device code).

weights.synthetic_weights draws biases of N(0, 0.01) under Xavier filters; behind a ReLU some channels then are (almost) never
positive -- with k = 64, L = 16 one logit channel is zero at every position -- and a wrong filter column, bias or fragment row of
such a channel changes nothing a test can see.  weights() therefore re-centres the biases of the three ReLU layers (conv0,
res1/conv1 and the final layer; res1/conv2 is linear): layer by layer, in float64, on ONE seeded calibration volume, each
channel's median pre-activation is subtracted from its bias, so every channel is positive at about half of the calibration
volume's positions.  tests/test_cpu_pc_cases.py asserts what that gives on the volumes the tests use (liveness()).

tests/test_gpu_pc_forward.py has the table of what each volume reaches."""
import functools
import zlib
from collections import OrderedDict

import numpy as np
import torch

PC = 'probclass3d/logits'
CENTERS = 'autoencoder/encoder/centers'
RELU_LAYERS = ('conv0', 'conv1', 'final')
SCOPES = OrderedDict([('conv0', PC + '/conv3d_conv0_mask'), ('conv1', PC + '/res1/conv3d_conv1_mask'),
                      ('conv2', PC + '/res1/conv3d_conv2_mask'), ('final', PC + '/conv3d_conv2_mask')])
CALIBRATION_SHAPE = (2, 6, 9, 20)

# (N, C, h, w).  k = 24: the middle layers pick one of three tiles per plane (ic_pc_mid_tile: 0 = 8 x 16, 1 = 5 x 25, 2 = 6 x 21);
# res1/conv1 works on the plane (h + 4, w + 4), res1/conv2 on (h + 2, w + 2), the final layer on (h, w) in 8 x 16 tiles.
# volume -> (tile of res1/conv1, tile of res1/conv2): what the tests expect the query to say
K24_VOLUMES = OrderedDict([
    ((1, 1, 1, 1), (0, 0)),       # all halo
    ((2, 5, 7, 11), (0, 0)),      # two images
    ((1, 2, 1, 21), (1, 1)),
    ((1, 3, 2, 17), (2, 1)),
    ((1, 2, 4, 19), (0, 2)),
    ((1, 3, 9, 17), (1, 2)),      # several tiles a plane in every layer; the final grid has a one-row and a one-column remainder
    ((1, 1, 8, 16), (2, 1)),      # exactly one final tile, one channel
    ((1, 1, 2, 38), (2, 1)),      # two tiles side by side: 6 x 21 on a 6 x 42 plane, 5 x 25 on 4 x 40 (the second one ragged)
])
# k = 64: one middle tile (3 = 4 x 16), ragged in both directions on the last two
K64_VOLUMES = OrderedDict([((1, 6, 5, 9), (3, 3)), ((2, 2, 3, 13), (3, 3)), ((1, 3, 9, 17), (3, 3))])
# other k: the VALU kernels, no tile (-1)
VALU_VOLUMES = OrderedDict([((2, 3, 5, 7), (-1, -1)), ((1, 1, 1, 1), (-1, -1))])

MFMA_GROUPS = [(24, L) for L in (2, 3, 6, 8, 11, 16)] + [(64, L) for L in (6, 11, 16)]
# k = 20 is no multiple of the 8-channel block of pc_conv3d_kernel; L = 6 ends in the COB = 8 final kernel, L = 11 in COB = 16
VALU_GROUPS = [(8, 6), (8, 11), (20, 6), (20, 11)]
GROUPS = MFMA_GROUPS + VALU_GROUPS
EDGE_GROUPS = [(24, 6), (24, 16)]
EDGE_VOLUME = (1, 3, 4, 19)


def volumes(k):
    return K24_VOLUMES if k == 24 else K64_VOLUMES if k == 64 else VALU_VOLUMES


def configs(k, L):
    from imgcomp_cvpr_amd import config_parser as cp
    ae_cfg, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc_cfg, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    ae_cfg.num_centers = L
    pc_cfg.arch_param__k = k
    return ae_cfg, pc_cfg


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def pre_activations(q64, wts, pad_value):
    """the float64 oracle layer by layer: q64 (N,C,h,w) -> {'conv0', 'conv1', 'conv2', 'final': conv + bias of that layer, before
    its ReLU (conv2: before the residual), (N, Cout, D, H, W)}"""
    from oracle import oracle as O
    first, other = O.pc_masks(3)
    x = O.pad_for_probclass3d(q64, 9, pad_value).unsqueeze(1)
    pre = OrderedDict()
    pre['conv0'] = O._conv3d(x, wts, SCOPES['conv0'], first, False)
    res_in = torch.relu(pre['conv0'])
    pre['conv1'] = O._conv3d(res_in, wts, SCOPES['conv1'], other, False)
    pre['conv2'] = O._conv3d(torch.relu(pre['conv1']), wts, SCOPES['conv2'], other, False)
    net = pre['conv2'] + res_in[:, :, 2:, 2:-2, 2:-2]
    pre['final'] = O._conv3d(net, wts, SCOPES['final'], other, False)
    return pre


@functools.lru_cache(maxsize=None)
def weights(k, L):
    """synthetic_weights for (k, L) with the biases of the three ReLU layers re-centred on the calibration volume; only the
    centres and the context model's variables are kept.  Treat the arrays as read-only: they are shared."""
    from imgcomp_cvpr_amd import weights as W
    full = W.synthetic_weights(*configs(k, L))
    wts = OrderedDict((n, a.copy()) for n, a in full.items() if n == CENTERS or n.startswith(PC + '/'))
    centers = wts[CENTERS]
    sym = np.random.RandomState(_seed('calibration', k, L)).randint(0, L, CALIBRATION_SHAPE)
    q64 = torch.as_tensor(centers[sym]).double()
    for layer in RELU_LAYERS:                       # in network order: a layer is centred on the centred layers before it
        pre = pre_activations(q64, wts, float(centers[0]))[layer]
        med = pre.permute(1, 0, 2, 3, 4).reshape(pre.shape[1], -1).median(dim=1).values.numpy()
        wts[SCOPES[layer] + '/biases'] = (wts[SCOPES[layer] + '/biases'].astype(np.float64) - med).astype(np.float32)
    return wts


@functools.lru_cache(maxsize=None)
def symbols(k, L, shape):
    """seeded targets (N,C,h,w) int64 in [0, L); shared like the weights: read-only"""
    return np.random.RandomState(_seed('symbols', k, L, shape)).randint(0, L, shape).astype(np.int64)


def inputs(k, L, shape, wts=None):
    """-> (q float32 (N,C,h,w) = centres[symbols], symbols int64, pad value = centres[0])"""
    wts = weights(k, L) if wts is None else wts
    sym = symbols(k, L, tuple(shape))
    return wts[CENTERS][sym], sym, float(wts[CENTERS][0])


@functools.lru_cache(maxsize=None)
def reference(k, L, shape):
    """the float64 oracle on a case: (bits (N,C,h,w), logits (N,C,h,w,L)), computed once per session"""
    from oracle import oracle as O
    q, sym, pad = inputs(k, L, shape)
    return O.bitcost(torch.as_tensor(q).double(), torch.as_tensor(sym), weights(k, L), pad)


def reference_with(wts, k, L, shape, dtype=torch.float64):
    """the oracle with other weights (the epilogue edge cases) or in float32 (the rule for a bound above RTOL)"""
    from oracle import oracle as O
    q, sym, pad = inputs(k, L, shape, wts)
    return O.bitcost(torch.as_tensor(q).to(dtype), torch.as_tensor(sym), wts, pad)


def liveness(k, L):
    """over all positions of all volumes of the group pooled: {layer: (share of positions where the channel is positive, per
    channel; share where it is clamped, per channel)} for the three ReLU layers, and the set of target symbols"""
    pos = {l: 0 for l in RELU_LAYERS}
    neg = {l: 0 for l in RELU_LAYERS}
    count = {l: 0 for l in RELU_LAYERS}
    seen = set()
    for shape in volumes(k):
        q, sym, pad = inputs(k, L, shape)
        seen.update(np.unique(sym).tolist())
        pre = pre_activations(torch.as_tensor(q).double(), weights(k, L), pad)
        for l in RELU_LAYERS:
            p = pre[l].permute(1, 0, 2, 3, 4).reshape(pre[l].shape[1], -1)
            pos[l] = pos[l] + (p > 0).sum(1).numpy()
            neg[l] = neg[l] + (p <= 0).sum(1).numpy()
            count[l] += p.shape[1]
    return {l: (pos[l] / count[l], neg[l] / count[l]) for l in RELU_LAYERS}, seen


# ---- the numeric edges of the cross-entropy epilogue ------------------------------------------------------------------------

def _with_final(wts, weight, bias):
    out = OrderedDict(wts)
    out[SCOPES['final'] + '/weights'] = weight.astype(np.float32)
    out[SCOPES['final'] + '/biases'] = bias.astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def far_apart_weights(k, L):
    """the final layer scaled by a power of two so that the float64 logits of EDGE_VOLUME spread over more than 90 somewhere:
    expf of the other logits underflows there and a target the model rules out costs over 100 bits.  (The final ReLU is
    positively homogeneous: the logits scale with the factor.)"""
    wts = weights(k, L)
    logits = reference(k, L, EDGE_VOLUME)[1]
    spread = float((logits.max(-1).values - logits.min(-1).values).max())
    factor = 2.0 ** int(np.ceil(np.log2(96.0 / spread)))
    return _with_final(wts, wts[SCOPES['final'] + '/weights'] * np.float32(factor), wts[SCOPES['final'] + '/biases'] * np.float32(factor))


@functools.lru_cache(maxsize=None)
def all_clamped_weights(k, L):
    """final bias -1e3: every logit clamps to 0, every symbol costs log2(L) bits"""
    wts = weights(k, L)
    return _with_final(wts, wts[SCOPES['final'] + '/weights'], np.full(L, -1e3))
