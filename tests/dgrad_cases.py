"""Cases for the parity tests of the data-gradient (dX) dispatch paths: a training step computes every dX by running a forward
kernel on the layer's filter repacked or re-read as its adjoint (TrainGraph._raw_backward_data -> _conv3x3(backward=True, res1,
res2) / _deconv_s / _conv_s in imgcomp_cvpr_amd/training.py).  This file is the table of cases, their seeded inputs and their
float64 references (a test helper: no device code).  tests/test_gpu_data_grad.py runs the kernels on them,
tests/test_cpu_dgrad_cases.py checks the table itself.

Reference: float64 autograd of the oracle's own forward -- y = oracle.train_oracle._conv / _deconv (x), y.backward(g), x.grad --
plus add1 / add2 in float64 where the case has them.  No product code.

A case's (N, H, W) is the shape of the incoming gradient g (the gradient wrt the layer's raw output).  For the layers that are
transposed convolutions (from_bn, h12, h13) g is the layer's OUTPUT, so its sides are even; there the odd / ragged / single-row
grid the case is about is the grid the adjoint kernel walks, (H / 2, W / 2) = the shape of dX.

Paths (PATHS below says what runs):
  part A, the 3x3 128 -> 128 adjoint    direct, f2_single, f2_batch, f4_batch
  part B, the strided adjoints          edge_deconv, mfma_deconv_pair, direct_deconv, mfma_conv3s2, mfma_conv5s2, edge_conv
"""
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

PATHS = {
    # ---- A: g (N,128,H,W) -> dX (N,128,H,W), the SAME convolution with the flipped, channel-swapped filter
    'direct': 'ic_pack_conv3x3_c128_bwd_f32 + ic_conv3x3_c128_bn_act_f32 (direct MFMA form)',
    'f2_single': 'ic_pack_wino3x3_c128_f32(backward = 1) + ic_wino3x3_c128_bn_act_f32 (Winograd F(2x2))',
    'f2_batch': 'ic_pack_wino3x3_c128_batch_f32(backward = 1) + ic_wino3x3_c128_bn_act_f32',
    'f4_batch': 'ic_pack_wino4_3x3_c128_batch_f32(backward = 1) + ic_wino4_3x3_c128_bn_act_f32 (Winograd F(4x4))',
    # ---- B: the layer's own array read in the other layout
    'edge_deconv': 'h1 adjoint: transposed conv 64 -> 3, 5x5 (the h13 edge kernel, no de-normalisation, no clip)',
    'mfma_deconv_pair': 'h2 adjoint: transposed conv 128 -> 64, 5x5 (paired four-phase MFMA kernel)',
    'direct_deconv': 'to_bn adjoint: transposed conv C or C + 1 -> 128, 5x5 (generic transposed direct kernel, 16 channels a lane)',
    'mfma_conv3s2': 'from_bn adjoint: conv 3x3 / 2, 128 -> C (MFMA, ragged last channel tile)',
    'mfma_conv5s2': 'h12 adjoint: conv 5x5 / 2, 64 -> 128 (the h2 MFMA kernel)',
    'edge_conv': 'h13 adjoint: conv 5x5 / 2, 3 -> 64 (the h1 edge kernel without input normalisation)',
}
A_PATHS = ('direct', 'f2_single', 'f2_batch', 'f4_batch')
B_PATHS = ('edge_deconv', 'mfma_deconv_pair', 'direct_deconv', 'mfma_conv3s2', 'mfma_conv5s2', 'edge_conv')
F4_PATHS = ('f4_batch',)                           # compared at W4_RTOL of tests/test_gpu_ops.py, every other path at RTOL

# part, role (layer), config, (N, H, W) of g, epilogue adds, expected path, how it is driven, F(4x4) mode of the graph, which filter:
#   drive 'graph'   TrainGraph._conv3x3(g, name or tensor, backward=True, res1, res2) resp. TrainGraph._raw_backward_data(layer, g, ..)
#         'abi'     the packer and the kernel through the C ABI
#         'auto'    ic_pack_conv3x3_c128_both_f32(backward = 1) + ic_conv3x3_c128_auto_f32 with the form asked for by its flags
#         'forced'  TrainGraph._conv3x3 with ic_conv3x3_c128_pick_algo answering 0: its direct branch, which the library's own answer
#                   reaches only on maps of 2 GiB and more (see DIRECT_NOTE)
#   filt  'random'  a seeded filter tensor; an int: the graph's i-th 3x3 parameter by name; None (part B): the layer's parameter
Case = namedtuple('Case', 'part role config N H W adds path drive mode filt')

DIRECT_NOTE = ('ic_conv3x3_c128_pick_algo(N, H, W, 0) is 0 only where 128 * H * W * 4 bytes reach 2^31 (H * W >= 2^22): no float64 reference '
               'of such a map fits a few seconds, and no tiny or odd map has that answer.  The direct form is therefore driven through '
               'the C ABI (the two calls the graph\'s branch makes, and the auto entry with IC_CONV3_DIRECT), and the graph\'s branch itself '
               'with the plan query answered 0 by the test.')

CONFIGS = {
    # name -> (ae config, pc config, heatmap): to_bn's data gradient comes from C + 1 channels with the importance map, else C
    'low': ('low', 'res_shallow', True),             # C = 32 -> 33
    'hi': ('hi', 'res_shallow_64', True),            # C = 64 -> 65
    'low_nohm': ('low', 'res_shallow', False),       # 32
    'hi_nohm': ('hi', 'res_shallow_64', False),      # 64
}
ENC, DEC = 'autoencoder/encoder', 'autoencoder/decoder'
SCOPES = {'h1': ENC + '/h1', 'h2': ENC + '/h2', 'to_bn': ENC + '/to_bn', 'from_bn': DEC + '/from_bn', 'h12': DEC + '/h12', 'h13': DEC + '/h13'}
ROLE_PATH = {'h1': 'edge_deconv', 'h2': 'mfma_deconv_pair', 'to_bn': 'direct_deconv', 'from_bn': 'mfma_conv3s2', 'h12': 'mfma_conv5s2',
             'h13': 'edge_conv'}
DECONV_ROLES = ('from_bn', 'h12', 'h13')            # the layer is a transposed conv: its adjoint is a strided conv


def _a(N, H, W, path, drive, mode=True, filt='random'):
    return [Case('A', 'res3x3', 'low', N, H, W, adds, path, drive, mode, filt) for adds in (0, 1, 2)]


# F(4x4) "fits" (TrainGraph._pack_all_3x3): wgs >= 160 and 2 * tiles >= 8 * wgs.  The smallest batch that fits, per segment shape
# (ic_wino4_3x3_c128_workgroups = 2 N segments; tests/test_cpu_dgrad_cases.py checks N - 1 does not fit):
#   (80, 8, 32)   one 2 x 8-tile segment a map       (80, 7, 32)   the same with a height that is no multiple of 4
#   (80, 4, 64)   one 1 x 16-tile segment a map      (40, 6, 64)   two 1 x 16 segments, the second row of tiles half beyond the map
#   (30, 40, 40)  the training crop geometry (30 crops of 160 x 160)
F4_SMALLEST = [(80, 8, 32), (80, 7, 32), (80, 4, 64), (40, 6, 64)]
F4_SHAPES = F4_SMALLEST + [(30, 40, 40)]

A_CASES = (
    # 1. direct MFMA form: odd width, a tiny map, two images, a full 16 x 32 tile
    _a(1, 7, 5, 'direct', 'abi') + _a(1, 3, 3, 'direct', 'abi') + _a(2, 13, 21, 'direct', 'abi') + _a(1, 16, 32, 'direct', 'abi')
    + _a(2, 13, 20, 'direct', 'auto') + _a(2, 13, 21, 'direct', 'forced') + _a(1, 7, 5, 'direct', 'forced')
    # 2. F(2x2), single packer (a filter tensor): odd H, odd W, W no multiple of 32, N > 1
    + _a(2, 13, 21, 'f2_single', 'graph') + _a(1, 7, 5, 'f2_single', 'graph') + _a(3, 10, 34, 'f2_single', 'graph')
    + _a(1, 9, 40, 'f2_single', 'graph') + _a(2, 13, 21, 'f2_single', 'abi') + _a(2, 13, 20, 'f2_single', 'auto')
    # 3. F(2x2), batched packer (a parameter name; the first, a middle and the last filter of the table)
    + _a(2, 13, 20, 'f2_batch', 'graph', filt=0) + _a(3, 9, 34, 'f2_batch', 'graph', filt=31) + _a(1, 7, 5, 'f2_batch', 'graph', filt=63)
    + _a(2, 13, 21, 'f2_batch', 'abi')
    # 4. F(4x4), batched packer
    + _a(80, 8, 32, 'f4_batch', 'graph', filt=0) + _a(80, 7, 32, 'f4_batch', 'graph', filt=31) + _a(80, 4, 64, 'f4_batch', 'graph', filt=63)
    + _a(40, 6, 64, 'f4_batch', 'graph', filt=17) + _a(30, 40, 40, 'f4_batch', 'graph', filt=40)
    + _a(80, 7, 32, 'f4_batch', 'abi') + _a(2, 13, 20, 'f4_batch', 'auto')
    #    one direction F(4x4), the other F(2x2), in one graph: mode 'bwd' runs the adjoint in F(4x4), mode 'fwd' leaves it in F(2x2)
    + _a(80, 7, 32, 'f4_batch', 'graph', mode='bwd', filt=5) + _a(80, 7, 32, 'f2_batch', 'graph', mode='fwd', filt=5)
)


def _b(role, config):
    """per role: the adjoint kernel's grid (gh, gw) with odd height and odd width, more than one 16-pixel tile and a ragged last
    one (9 x 37: also more than one 256-pixel block of the direct kernel and several tile rows), a single row, two images; one of
    them with one add, one with both"""
    out = []
    for (N, gh, gw), adds in (((1, 9, 37), 0), ((1, 1, 21), 1), ((2, 3, 17), 2)):
        H, W = (2 * gh, 2 * gw) if role in DECONV_ROLES else (gh, gw)
        out.append(Case('B', role, config, N, H, W, adds, ROLE_PATH[role], 'graph', True, None))
    return out


B_CASES = (_b('h1', 'low') + _b('h2', 'low')
           + _b('to_bn', 'low') + _b('to_bn', 'hi') + _b('to_bn', 'low_nohm') + _b('to_bn', 'hi_nohm')
           + _b('from_bn', 'low') + _b('from_bn', 'hi') + _b('h12', 'low') + _b('h13', 'low'))
CASES = A_CASES + B_CASES


def case_id(c):
    mode = '' if c.mode is True else '-mode_{}'.format(c.mode)
    return '{}-{}-{}-{}x{}x{}-adds{}-{}{}'.format(c.path, c.role, c.config, c.N, c.H, c.W, c.adds, c.drive, mode)


def rtol(case):
    """the project's single-op bars: W4_RTOL for the F(4x4) path, RTOL for every other"""
    from tests.test_gpu_ops import W4_RTOL
    from tests.util import RTOL
    return W4_RTOL if case.path in F4_PATHS else RTOL


def f4_fits(lib, N, H, W):
    """what the table expects of TrainGraph._pack_all_3x3's rule (the GPU tests compare the graph's own _w3_f4 with it)"""
    wgs = int(lib.ic_wino4_3x3_c128_workgroups(N, H, W))
    tiles = N * (-(-H // 4)) * (-(-W // 4))
    return wgs >= 160 and 2 * tiles >= 8 * wgs


# ---- configurations, filters, inputs --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def configs(name):
    from imgcomp_cvpr_amd import config_parser as cp
    ae, pc, heatmap = CONFIGS[name]
    ae_cfg, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', ae))
    pc_cfg, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', pc))
    ae_cfg.heatmap = heatmap
    return ae_cfg, pc_cfg


@functools.lru_cache(maxsize=None)
def weights(name):
    """the synthetic variables of a configuration (read-only: shared by the graphs and the references)"""
    from imgcomp_cvpr_amd import weights as W
    return W.synthetic_weights(*configs(name))


@functools.lru_cache(maxsize=None)
def w3_names(name):
    """the 3x3 128 -> 128 filters in the order of TrainGraph._w3_names (the layer table's order)"""
    from imgcomp_cvpr_amd import weights as W
    ae_cfg, _ = configs(name)
    return [s + '/weights' for s, kind, sh in W.ae_conv_specs(int(ae_cfg.num_chan_bn), int(ae_cfg.arch_param_B), bool(ae_cfg.heatmap))
            if kind == 'conv' and sh == (3, 3, 128, 128)]


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


@functools.lru_cache(maxsize=None)
def random_filter(key=0):
    """a 3x3 128 -> 128 filter with no symmetry at all (TF layout [kh, kw, cin, cout])"""
    return np.random.RandomState(_seed('filter', key)).normal(0, 0.05, (3, 3, 128, 128)).astype(np.float32)


def filter_name(case):
    if case.part == 'A':
        return w3_names(case.config)[case.filt] if case.filt != 'random' else None
    return SCOPES[case.role] + '/weights'


def filter_of(case):
    """the layer's filter in its TF layout, float32"""
    name = filter_name(case)
    return random_filter() if name is None else weights(case.config)[name]


def dx_shape(case):
    w = filter_of(case)
    if case.part == 'A':
        return (case.N, 128, case.H, case.W)
    if case.role in DECONV_ROLES:                    # w [kh, kw, cout_l, cin_l]: dX has the layer's cin_l channels at half the size
        return (case.N, w.shape[3], case.H // 2, case.W // 2)
    return (case.N, w.shape[2], 2 * case.H, 2 * case.W)


def g_channels(case):
    w = filter_of(case)
    return 128 if case.part == 'A' else (w.shape[2] if case.role in DECONV_ROLES else w.shape[3])


def _key(case):
    """what the reference without its adds depends on"""
    return (case.part, case.role, case.config, case.N, case.H, case.W, case.filt)


@functools.lru_cache(maxsize=None)
def _inputs(key):
    case = next(c for c in CASES if _key(c) == key)
    rs = np.random.RandomState(_seed('inputs', key))
    g = rs.normal(0, 1, (case.N, g_channels(case), case.H, case.W)).astype(np.float32)
    add1 = rs.normal(0, 1, dx_shape(case)).astype(np.float32)
    add2 = rs.normal(0, 1, dx_shape(case)).astype(np.float32)
    return g, add1, add2


def inputs(case):
    """-> (g, [the case's adds]) float32, seeded by everything but the number of adds (shared, read-only)"""
    g, add1, add2 = _inputs(_key(case))
    return g, [add1, add2][:case.adds]


# ---- references -----------------------------------------------------------------------------------------------------------------

def forward64(case, x64, w64):
    """the oracle's forward of the case's layer"""
    from oracle import train_oracle as T
    if case.part == 'A':
        return T._conv(x64, w64, 1)
    return T._deconv(x64, w64) if case.role in DECONV_ROLES else T._conv(x64, w64, 2)


@functools.lru_cache(maxsize=None)
def _base_reference(key):
    case = next(c for c in CASES if _key(c) == key)
    torch.set_num_threads(16)
    x = torch.zeros(dx_shape(case), dtype=torch.float64, requires_grad=True)        # the layer is linear: dX does not depend on x
    y = forward64(case, x, torch.as_tensor(filter_of(case)).double())
    g = torch.as_tensor(inputs(case)[0]).double()
    assert y.shape == g.shape, (y.shape, g.shape)
    y.backward(g)
    return x.grad.detach()


def reference(case):
    """float64 autograd of the oracle's forward, + the case's adds: computed once per (layer, shape), shared by the adds variants"""
    ref = _base_reference(_key(case))
    for a in inputs(case)[1]:
        ref = ref + torch.as_tensor(a).double()
    return ref


def adjoint_filter(w):
    """part A's adjoint as a filter: flipped in both spatial axes, channel axes swapped"""
    return np.ascontiguousarray(w[::-1, ::-1].transpose(0, 1, 3, 2))


def independent(case, w=None, adds=None, images=None):
    """the adjoint stated without autograd.  A: a SAME convolution of g with adjoint_filter(w).  B: the oracle's transposed (strided)
    convolution of g with the SAME array read in the other layout -- a conv filter [kh, kw, cin, cout] is the transposed conv's
    [kh, kw, out, in] and the other way round.  w / adds: another filter / other adds (the mistakes below); images: the first
    `images` of the batch only."""
    from oracle import oracle as O
    torch.set_num_threads(16)
    g, own = inputs(case)
    adds = own if adds is None else adds
    n = case.N if images is None else images
    g64 = torch.as_tensor(g[:n]).double()
    if case.part == 'A':
        out = O.conv2d_same(g64, adjoint_filter(filter_of(case)) if w is None else w, 1)
    else:
        w = filter_of(case) if w is None else w
        out = O.conv2d_same(g64, w, 2) if case.role in DECONV_ROLES else O.conv2d_transpose_same(g64, w, 2)
    for a in adds:
        out = out + torch.as_tensor(a[:n]).double()
    return out


def mistakes(case, images=None):
    """three plausible mistakes -> {name: result}: the filter not flipped, its channels not swapped (B: the channel axes of the array
    read in the wrong order -- the same memory, [a][b] taken for [b][a]), the adds left out (cases with adds only)"""
    w = filter_of(case)
    if case.part == 'A':
        not_flipped = np.ascontiguousarray(w.transpose(0, 1, 3, 2))
        not_swapped = np.ascontiguousarray(w[::-1, ::-1])
    else:
        not_flipped = np.ascontiguousarray(w[::-1, ::-1])
        not_swapped = np.ascontiguousarray(w.reshape(w.shape[0], w.shape[1], w.shape[3], w.shape[2]).transpose(0, 1, 3, 2))
    out = {'filter not flipped': independent(case, not_flipped, images=images),
           'channels not swapped': independent(case, not_swapped, images=images)}
    if case.adds:
        out['adds left out'] = independent(case, adds=[], images=images)
    return out


# ---- which path a case takes, by the library's host-side plan functions ---------------------------------------------------------

def auto_flags(L, case):
    """drive 'auto': the flags that ask ic_conv3x3_c128_auto_f32 for the case's form"""
    return {'direct': L.CONV3_DIRECT, 'f2_single': L.CONV3_WINO | L.CONV3_NO_WINO4, 'f4_batch': L.CONV3_WINO4}[case.path]


def adjoint_call(case):
    """part B: the arguments (kh, kw, cin, cout, stride, transposed) of the convolution that is the case's data gradient"""
    kh, kw, a, b = filter_of(case).shape
    return (kh, kw, a, b, 2, 0) if case.role in DECONV_ROLES else (kh, kw, b, a, 2, 1)


def expected_plan(L, case):
    """asserts that the library's plan functions send the case down the path the table names (host arithmetic only); the graph's
    own choice between the batched packers (_w3_f4) is asserted where a graph exists, against f4_fits"""
    lib, N, H, W = L.lib, case.N, case.H, case.W
    if case.part == 'B':
        packed = lib.ic_conv2d_mfma_packed_floats(*adjoint_call(case))
        assert (packed > 0) == (case.path in ('mfma_deconv_pair', 'mfma_conv3s2', 'mfma_conv5s2')), (case.path, packed)
        kh, kw, cin, cout, _, tr = adjoint_call(case)
        assert {'edge_deconv': (5, 64, 3, 1), 'edge_conv': (5, 3, 64, 0), 'mfma_deconv_pair': (5, 128, 64, 1), 'mfma_conv5s2': (5, 64, 128, 0)}.get(
            case.path, (kh, cin, cout, tr)) == (kh, cin, cout, tr)
        if case.path == 'direct_deconv':
            assert (kh, cout, tr) == (5, 128, 1) and cin in (32, 33, 64, 65)
        if case.path == 'mfma_conv3s2':
            assert (kh, cin, tr) == (3, 128, 0) and cout in (32, 64)
        return True
    assert lib.ic_conv3x3_c128_pick_algo(N, H, W, 0) == 1            # every small map: a Winograd form unless the caller asks
    if case.drive == 'auto':
        form = lib.ic_conv3x3_c128_pick_form(N, H, W, auto_flags(L, case))
        assert form == {'direct': 0, 'f2_single': 1, 'f4_batch': 2}[case.path], form
    if case.path == 'direct':
        assert lib.ic_conv3x3_c128_pick_algo(N, H, W, L.CONV3_DIRECT) == 0
    elif case.path == 'f4_batch':
        assert lib.ic_wino4_3x3_c128_supported(N, H, W) == 1
        if case.drive == 'graph':
            assert f4_fits(lib, N, H, W) and case.mode in (True, 'bwd')
    elif case.path == 'f2_batch' and case.drive == 'graph':
        assert (not f4_fits(lib, N, H, W)) if case.mode is True else (f4_fits(lib, N, H, W) and case.mode == 'fwd')
    return True
