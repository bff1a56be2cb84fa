"""Small maps for every instantiation family of wino4_3x3_kernel (csrc/conv3x3_wino4.hip): seeded inputs, the launch, and the float64
reference.  Shared by tools/make_wino4_small_golden.py (which records the outputs of a known-good library into
tests/golden/wino4_small.npz) and tests/test_gpu_wino4_small.py (which compares against that record bit for bit and against the
float64 convolution).  Every map is a few tile rows: a launch takes microseconds.

  map            what it exercises
  1 x 8 x 64     one segment per tile row, two tile rows: every patch has a row outside the image, both end lanes load a column outside
  1 x 10 x 72    H % 4 != 0 (the last tile row has 2 valid rows); the second segment has 2 of 16 tiles valid, so a valid lane's right
                 neighbour lies beyond the map
  2 x 12 x 64    batch offset, an interior tile row with no padding
  2 x 32 x 32    2 x 8-tile segments (SEG2): per-lane row validity, the middle lanes 7 / 8
  1 x 8 x 32     SEG2 with one segment
  1 x 12 x 128   the 8-wave form (IC_CONV3_WINO4_WG8)
"""
import hashlib
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wino4_small.npz')

# (name, N, H, W, form flag name or None)
C128_MAPS = [
    ('8x64', 1, 8, 64, None),
    ('10x72', 1, 10, 72, None),
    ('b2_12x64', 2, 12, 64, None),
    ('b2_32x32_seg2', 2, 32, 32, None),
    ('8x32_seg2', 1, 8, 32, None),
    ('12x128_wg8', 1, 12, 128, 'CONV3_WINO4_WG8'),
]
C128_CASES = [(m, n_res, relu) for m in C128_MAPS for n_res in (0, 1, 2) for relu in (0, 1)]
STATS_MAP = ('b2_32x32_seg2', 2, 32, 32, None)
PHASE_MAP = (1, 8, 64)                       # the quarter-resolution map of h2's output / h12's input
PHASE_CASES = [(tr, relu) for tr in (0, 1) for relu in (0, 1)]
RAW_KEPT = ['c128/8x32_seg2/res2/relu1', 'c128/8x64/res2/relu1']      # the two smallest cases: raw float32 output in the record


def c128_id(m, n_res, relu):
    return 'c128/{}/res{}/relu{}'.format(m[0], n_res, relu)


def phase_id(tr, relu):
    return '{}/8x64/relu{}'.format('h12' if tr else 'h2', relu)


def _seed(name):
    return int(hashlib.sha256(name.encode()).hexdigest()[:8], 16) % (2 ** 31)


def c128_inputs(m):
    """activations with about half their values zero (as behind a ReLU), random filter, BatchNorm scale / shift, two residuals"""
    name, N, H, W, _ = m
    rs = np.random.RandomState(_seed('c128/' + name))
    x = np.maximum(rs.normal(0, 1, (N, 128, H, W)), 0).astype(np.float32) * np.float32(1.5)
    w = rs.normal(0, 0.04, (3, 3, 128, 128)).astype(np.float32)
    scale = rs.uniform(0.5, 1.5, 128).astype(np.float32)
    shift = rs.normal(0, 0.3, 128).astype(np.float32)
    r1 = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    r2 = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    return dict(x=x, w=w, scale=scale, shift=shift, r1=r1, r2=r2)


def phase_inputs(tr):
    N, H, W = PHASE_MAP
    rs = np.random.RandomState(_seed('phase/{}'.format(tr)))
    cout = 64 if tr else 128
    shape = (N, 128, H, W) if tr else (N, 64, 2 * H, 2 * W)
    x = np.maximum(rs.normal(0, 1, shape), 0).astype(np.float32) * np.float32(1.2)
    w = rs.normal(0, 0.03, (5, 5, 64, 128)).astype(np.float32)
    scale = rs.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = rs.normal(0, 0.3, cout).astype(np.float32)
    return dict(x=x, w=w, scale=scale, shift=shift)


def space_to_depth2(x):
    """[N][C][2H][2W] -> [N][4 C][H][W], channel (2 py + px) * C + c (what ic_wino4_conv5s2_c64_c128_bn_act_f32 reads)"""
    N, C, H2, W2 = x.shape
    return np.ascontiguousarray(x.reshape(N, C, H2 // 2, 2, W2 // 2, 2).transpose(0, 3, 5, 1, 2, 4)).reshape(N, 4 * C, H2 // 2, W2 // 2)


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


class Device(object):
    """the launches, with the device copies of a map's inputs and its packed filter made once"""

    def __init__(self, L, cuda):
        self.L, self.cuda, self._c128, self._phase = L, cuda, {}, {}

    def _dev(self, a):
        return torch.as_tensor(np.ascontiguousarray(a)).to(self.cuda)

    def c128_state(self, m):
        if m[0] not in self._c128:
            L = self.L
            d = {k: self._dev(v) for k, v in c128_inputs(m).items()}
            d['wp'] = torch.empty(L.lib.ic_wino4_3x3_c128_packed_floats(), device=self.cuda)
            L.check(L.lib.ic_pack_wino4_3x3_c128_f32(L.ptr(d['w']), L.ptr(d['wp']), 0, L.current_stream()))
            self._c128[m[0]] = d
        return self._c128[m[0]]

    def c128(self, m, n_res, relu):
        L = self.L
        name, N, H, W, form = m
        flags = getattr(L, form) if form else L.CONV3_WINO4_WG4
        waves = int(L.lib.ic_wino4_3x3_c128_waves(N, H, W, flags))
        assert waves == (8 if form else 4), (name, waves)
        d = self.c128_state(m)
        y = torch.full((N, 128, H, W), float('nan'), device=self.cuda)
        L.check(L.lib.ic_wino4_3x3_c128_bn_act_f32(L.ptr(d['x']), L.ptr(d['wp']), L.ptr(d['scale']), L.ptr(d['shift']),
                                                   L.ptr(d['r1']) if n_res >= 1 else None, L.ptr(d['r2']) if n_res >= 2 else None,
                                                   L.ptr(y), N, H, W, relu, flags, L.current_stream()))
        torch.cuda.synchronize()
        return y

    def stats(self):
        L = self.L
        _, N, H, W, _ = STATS_MAP
        d = self.c128_state(STATS_MAP)
        parts = int(L.lib.ic_wino4_3x3_c128_stats_parts(N, H, W))
        raw = torch.full((N, 128, H, W), float('nan'), device=self.cuda)
        cst = torch.full((128, parts, 2), float('nan'), device=self.cuda)
        L.check(L.lib.ic_wino4_3x3_c128_raw_stats_f32(L.ptr(d['x']), L.ptr(d['wp']), L.ptr(raw), L.ptr(cst), N, H, W, 0, L.current_stream()))
        torch.cuda.synchronize()
        return raw, cst

    def phase(self, tr, relu):
        L = self.L
        N, H, W = PHASE_MAP
        st = L.current_stream()
        if tr not in self._phase:
            inp = phase_inputs(tr)
            d = {k: self._dev(v) for k, v in inp.items()}
            if not tr:
                d['x'] = self._dev(space_to_depth2(inp['x']))
            d['wp'] = torch.empty(L.lib.ic_wino4_conv5s2_packed_floats(), device=self.cuda)
            L.check(L.lib.ic_pack_wino4_conv5s2_f32(L.ptr(d['w']), L.ptr(d['wp']), tr, st))
            self._phase[tr] = d
        d = self._phase[tr]
        if tr:
            y = torch.full((N, 64, 2 * H, 2 * W), float('nan'), device=self.cuda)
            L.check(L.lib.ic_wino4_deconv5s2_c128_c64_bn_act_f32(L.ptr(d['x']), L.ptr(d['wp']), L.ptr(d['scale']), L.ptr(d['shift']), L.ptr(y),
                                                                 N, H, W, relu, 0, st))
        else:
            y = torch.full((N, 128, H, W), float('nan'), device=self.cuda)
            L.check(L.lib.ic_wino4_conv5s2_c64_c128_bn_act_f32(L.ptr(d['x']), L.ptr(d['wp']), L.ptr(d['scale']), L.ptr(d['shift']), L.ptr(y),
                                                               N, H, W, relu, 0, st))
        torch.cuda.synchronize()
        return y


# ---- float64 references: the convolution of a map is made once, the epilogue variants are applied to it ----
_RAW64 = {}


def c128_raw64(m):
    if m[0] not in _RAW64:
        from oracle import oracle as O
        inp = c128_inputs(m)
        _RAW64[m[0]] = O.conv2d_same(torch.as_tensor(inp['x']).double(), inp['w'], 1)
    return _RAW64[m[0]]


def _epilogue64(raw, inp, relu, res):
    y = raw * torch.as_tensor(inp['scale']).double().view(1, -1, 1, 1) + torch.as_tensor(inp['shift']).double().view(1, -1, 1, 1)
    if relu:
        y = torch.relu(y)
    for r in res:
        y = y + torch.as_tensor(r).double()
    return y


def c128_ref64(m, n_res, relu):
    inp = c128_inputs(m)
    return _epilogue64(c128_raw64(m), inp, relu, [inp['r1'], inp['r2']][:n_res])


def phase_ref64(tr, relu):
    key = 'phase{}'.format(tr)
    inp = phase_inputs(tr)
    if key not in _RAW64:
        from oracle import oracle as O
        xt = torch.as_tensor(inp['x']).double()
        _RAW64[key] = O.conv2d_transpose_same(xt, inp['w'], 2) if tr else O.conv2d_same(xt, inp['w'], 2)
    return _epilogue64(_RAW64[key], inp, relu, [])
