"""-m gpu: the data gradient (dX) of every convolution on every adjoint dispatch path, against float64 autograd of the oracle's
own forward (tests/dgrad_cases.py has the table, the inputs and the references; tests/test_cpu_dgrad_cases.py checks them).

A training step computes dX by running the forward kernels on the filter repacked or re-read as its adjoint.  Part A is the 3x3
128 -> 128 adjoint -- direct MFMA form, F(2x2) with the single and with the batched packer, F(4x4) with the batched packer -- driven
through TrainGraph._conv3x3(g, name or tensor, backward=True, res1, res2) and through the C ABI, with 0, 1 and 2 epilogue adds
(the skip gradients of the residual stack).  Part B is the strided adjoints through TrainGraph._raw_backward_data.  Every case
first asserts, by the library's host-side plan functions and the graph's _w3_f4, that it takes the path the table names.
Bars: RTOL, and W4_RTOL on the F(4x4) path."""
import functools

import pytest
import torch

from tests import dgrad_cases as D
from tests.util import assert_close, dev

pytestmark = pytest.mark.gpu


def _L():
    from imgcomp_cvpr_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _graph(config, mode=True):
    """one TrainGraph per configuration and F(4x4) mode for the whole module"""
    from imgcomp_cvpr_amd import training
    ae_cfg, pc_cfg = D.configs(config)
    return training.TrainGraph(ae_cfg, pc_cfg, D.weights(config), 'cuda:0', wino4=mode)


def _label(case):
    return 'dX {} {} ({}, {} adds{})'.format(case.path, case.role if case.part == 'B' else '3x3', case.drive, case.adds,
                                              '' if case.mode is True else ', mode ' + case.mode)


def _device_inputs(cuda, case):
    g, adds = D.inputs(case)
    adds = [dev(a, cuda) for a in adds]
    return dev(g, cuda), (adds + [None, None])[:2]


def _conv3x3_abi(L, cuda, case, gd, wd, r1, r2):
    """the adjoint through the C ABI: the packer of the case's path with backward = 1, then the path's kernel"""
    lib, st = L.lib, L.current_stream()
    N, H, W = case.N, case.H, case.W
    ones, zeros = torch.ones(128, device=cuda), torch.zeros(128, device=cuda)
    y = torch.full((N, 128, H, W), float('nan'), device=cuda)
    args = (L.ptr(ones), L.ptr(zeros), L.ptr(r1), L.ptr(r2), L.ptr(y), N, H, W, 0)
    if case.drive == 'auto':
        wp = torch.full((lib.ic_conv3x3_c128_both_packed_floats(),), float('nan'), device=cuda)
        L.check(lib.ic_pack_conv3x3_c128_both_f32(L.ptr(wd), L.ptr(wp), 1, st))
        L.check(lib.ic_conv3x3_c128_auto_f32(L.ptr(gd), L.ptr(wp), *args, D.auto_flags(L, case), st))
    elif case.path == 'direct':
        wp = torch.full((lib.ic_conv3x3_c128_packed_floats(),), float('nan'), device=cuda)
        L.check(lib.ic_pack_conv3x3_c128_bwd_f32(L.ptr(wd), L.ptr(wp), st))
        L.check(lib.ic_conv3x3_c128_bn_act_f32(L.ptr(gd), L.ptr(wp), *args, 0, st))
    elif case.path == 'f2_single':
        wp = torch.full((lib.ic_wino3x3_c128_packed_floats(),), float('nan'), device=cuda)
        L.check(lib.ic_pack_wino3x3_c128_f32(L.ptr(wd), L.ptr(wp), 1, st))
        L.check(lib.ic_wino3x3_c128_bn_act_f32(L.ptr(gd), L.ptr(wp), *args, 0, st))
    else:
        # the batched packers: the case's filter between two others, its fragments taken from the middle of the batch
        others = [dev(D.random_filter(k), cuda) for k in (1, 2)]
        table = torch.tensor([others[0].data_ptr(), wd.data_ptr(), others[1].data_ptr()], dtype=torch.int64, device=cuda)
        f4 = case.path == 'f4_batch'
        n = lib.ic_wino4_3x3_c128_packed_floats() if f4 else lib.ic_wino3x3_c128_packed_floats()
        wp = torch.full((3, n), float('nan'), device=cuda)
        L.check((lib.ic_pack_wino4_3x3_c128_batch_f32 if f4 else lib.ic_pack_wino3x3_c128_batch_f32)(L.ptr(table), L.ptr(wp), 3, 1, st))
        L.check((lib.ic_wino4_3x3_c128_bn_act_f32 if f4 else lib.ic_wino3x3_c128_bn_act_f32)(L.ptr(gd), L.ptr(wp[1]), *args, 0, st))
    torch.cuda.synchronize()
    return y


class _PlanSaysDirect(object):
    """the library with ic_conv3x3_c128_pick_algo answering 0 (dgrad_cases.DIRECT_NOTE); every other entry is the library's"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def ic_conv3x3_c128_pick_algo(self, N, H, W, flags):
        return 0


def _conv3x3_graph(L, cuda, case, gd, r1, r2, monkeypatch):
    """the adjoint through TrainGraph._conv3x3"""
    from imgcomp_cvpr_amd import training
    G = _graph(case.config, case.mode)
    N, H, W = case.N, case.H, case.W
    if case.drive == 'forced':
        monkeypatch.setattr(training, 'lib', _PlanSaysDirect(L.lib))
        name = dev(D.filter_of(case), cuda)
    elif case.path == 'f2_single':
        name = dev(D.filter_of(case), cuda)                       # a tensor: the single packer whatever the graph has packed
    else:
        G._pack_all_3x3(N, H, W)
        fits = D.f4_fits(L.lib, N, H, W)
        assert G._wino_pk is not None
        assert G._w3_f4 == (fits and case.mode in (True, 'fwd'), fits and case.mode in (True, 'bwd'))
        assert G._w3_f4[1] == (case.path == 'f4_batch')
        name = D.filter_name(case)
        assert G._w3_names == D.w3_names(case.config) and G._w3_index[name] == case.filt
        assert torch.equal(G.params[name].cpu(), torch.as_tensor(D.filter_of(case)))
    y = G._conv3x3(gd, name, backward=True, res1=r1, res2=r2)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize('case', D.A_CASES, ids=D.case_id)
def test_conv3x3_adjoint(cuda, case, monkeypatch):
    L = _L()
    assert D.expected_plan(L, case)
    gd, (r1, r2) = _device_inputs(cuda, case)
    if case.drive in ('abi', 'auto'):
        y = _conv3x3_abi(L, cuda, case, gd, dev(D.filter_of(case), cuda), r1, r2)
    else:
        y = _conv3x3_graph(L, cuda, case, gd, r1, r2, monkeypatch)
    assert_close(y, D.reference(case), _label(case), D.rtol(case))


@pytest.mark.parametrize('mode', ['fwd', 'bwd'])
def test_one_graph_runs_one_direction_in_each_winograd_form(cuda, mode):
    """TrainGraph(wino4='fwd' / 'bwd') at a shape where F(4x4) fits: the forward convolution and the data gradient of one filter come
    from two batched packers and two kernels in the same graph, and each is the oracle's (the adjoint cases of these graphs are in
    the table: this is the forward direction beside them, and that the two directions' fragments are not mixed up)."""
    from oracle import train_oracle as T
    from tests.test_gpu_ops import W4_RTOL
    from tests.util import RTOL
    L = _L()
    case = next(c for c in D.A_CASES if c.mode == mode and c.adds == 2)
    G = _graph(case.config, mode)
    G._pack_all_3x3(case.N, case.H, case.W)
    assert G._w3_f4 == ((True, False) if mode == 'fwd' else (False, True))
    assert G._wino_pk[0].shape[1] == (L.lib.ic_wino4_3x3_c128_packed_floats() if mode == 'fwd' else L.lib.ic_wino3x3_c128_packed_floats())
    assert G._wino_pk[1].shape[1] == (L.lib.ic_wino3x3_c128_packed_floats() if mode == 'fwd' else L.lib.ic_wino4_3x3_c128_packed_floats())
    gd, (r1, r2) = _device_inputs(cuda, case)
    y = G._conv3x3(gd, D.filter_name(case), backward=False, res1=r1, res2=r2)
    dx = G._conv3x3(gd, D.filter_name(case), backward=True, res1=r1, res2=r2)
    torch.cuda.synchronize()
    torch.set_num_threads(16)
    g, adds = D.inputs(case)
    fwd = T._conv(torch.as_tensor(g).double(), torch.as_tensor(D.filter_of(case)).double(), 1)
    fwd = (fwd + torch.as_tensor(adds[0]).double()) + torch.as_tensor(adds[1]).double()
    assert_close(y, fwd, 'forward beside the adjoint, mode {}'.format(mode), W4_RTOL if mode == 'fwd' else RTOL)
    assert_close(dx, D.reference(case), 'dX beside the forward, mode {}'.format(mode), D.rtol(case))


@pytest.mark.parametrize('case', D.B_CASES, ids=D.case_id)
def test_strided_adjoint(cuda, case):
    L = _L()
    assert D.expected_plan(L, case)
    G = _graph(case.config)
    layer = G.layers[D.SCOPES[case.role]]
    kh, kw, cin, cout, stride, transposed = D.adjoint_call(case)
    assert (layer.kind == 'deconv') == (case.role in D.DECONV_ROLES) and (layer.kh, layer.kw) == (kh, kw)
    assert (layer.cout, layer.cin) == (cin, cout)                 # the adjoint maps the layer's outputs back to its inputs
    assert torch.equal(G.params[D.filter_name(case)].cpu(), torch.as_tensor(D.filter_of(case)))
    gd, (a1, a2) = _device_inputs(cuda, case)
    dx = G._raw_backward_data(layer, gd, a1, a2)
    torch.cuda.synchronize()
    assert_close(dx, D.reference(case), _label(case), D.rtol(case))


def test_packer_identities(cuda):
    """the batched F(2x2) packer writes, layer by layer, what the single one writes (forward and adjoint); the `both` blob packed with
    backward = 1 is the direct form's adjoint pack followed by the F(2x2) adjoint pack (and the F(4x4) one); the adjoint pack of a
    filter with no symmetry is not its forward pack, in any of the three forms."""
    L = _L()
    lib, st = L.lib, L.current_stream()
    ws = [dev(D.random_filter(k), cuda) for k in (0, 1, 2)]
    table = torch.tensor([w.data_ptr() for w in ws], dtype=torch.int64, device=cuda)
    n2, n4, nd = lib.ic_wino3x3_c128_packed_floats(), lib.ic_wino4_3x3_c128_packed_floats(), lib.ic_conv3x3_c128_packed_floats()
    assert lib.ic_conv3x3_c128_both_packed_floats() == nd + n2 + n4

    def single(fn, n, w, *backward):
        out = torch.full((n,), float('nan'), device=cuda)
        L.check(fn(L.ptr(w), L.ptr(out), *backward, st))
        return out
    packs = {}
    for backward in (0, 1):
        batch = torch.full((3, n2), float('nan'), device=cuda)
        L.check(lib.ic_pack_wino3x3_c128_batch_f32(L.ptr(table), L.ptr(batch), 3, backward, st))
        for l, w in enumerate(ws):
            one = single(lib.ic_pack_wino3x3_c128_f32, n2, w, backward)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(one).all())
            assert torch.equal(batch[l], one), 'F(2x2) batched packer, layer {} backward {}'.format(l, backward)
        both = single(lib.ic_pack_conv3x3_c128_both_f32, nd + n2 + n4, ws[0], backward)
        direct = single(lib.ic_pack_conv3x3_c128_bwd_f32 if backward else lib.ic_pack_conv3x3_c128_f32, nd, ws[0])
        f2, f4 = single(lib.ic_pack_wino3x3_c128_f32, n2, ws[0], backward), single(lib.ic_pack_wino4_3x3_c128_f32, n4, ws[0], backward)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(both).all())
        assert torch.equal(both[:nd], direct) and torch.equal(both[nd:nd + n2], f2) and torch.equal(both[nd + n2:], f4), backward
        packs[backward] = (direct, f2, f4)
    for fwd, bwd in zip(packs[0], packs[1]):
        assert not torch.equal(fwd, bwd)
    assert nd == ws[0].numel() and torch.equal(packs[0][0].sort().values, packs[1][0].sort().values)      # the direct packs permute the filter, no more


def test_the_table_reaches_every_adjoint_path():
    """a later change of the table (or of a plan rule, through expected_plan in every case above) must not empty a path's coverage"""
    ran = {c.path for c in D.A_CASES} | {c.path for c in D.B_CASES}
    assert ran == set(D.PATHS)
    for path in D.A_PATHS:
        drives = {c.drive for c in D.A_CASES if c.path == path}
        assert drives & {'graph', 'forced'} and drives & {'abi', 'auto'}, path
        assert {c.adds for c in D.A_CASES if c.path == path} == {0, 1, 2}, path
    assert {D.g_channels(c) for c in D.B_CASES if c.role == 'to_bn'} == {32, 33, 64, 65}
