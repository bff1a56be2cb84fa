"""The cases of tests/dgrad_cases.py are what tests/test_gpu_data_grad.py takes them for (no GPU: float64 on the CPU and the host
side of the library).  The conditions below are conditions on the INPUTS and on the table: a case that misses one gets another
shape or seed, never a weaker condition."""
import collections

import pytest
import torch

from tests import dgrad_cases as D
from tests.util import rel_err

BIG = 8192          # pixels (N H W) above which the mistakes are evaluated on the first image only (the adjoint is per image)


@pytest.mark.parametrize('case', [c for c in D.CASES if c.adds == max(k.adds for k in D.CASES if D._key(k) == D._key(c))], ids=D.case_id)
def test_reference_is_the_adjoint_and_the_inputs_can_fail(case):
    """the autograd reference equals the adjoint stated independently (A: SAME convolution with the flipped, channel-swapped filter;
    B: the transposed / strided convolution with the same array read in the other layout) to 1e-12 of the tensor scale, and a filter
    not flipped, channels not swapped or the adds left out each miss it by 100 x the case's tolerance or more.  One variant per
    (layer, shape): the one with the most adds -- the others share its inputs and differ by a sum."""
    ref = D.reference(case)
    assert tuple(ref.shape) == D.dx_shape(case)
    assert rel_err(D.independent(case), ref) <= 1e-12
    n = 1 if case.N * case.H * case.W > BIG else None
    wrong = D.mistakes(case, images=n)
    assert set(wrong) == {'filter not flipped', 'channels not swapped'} | ({'adds left out'} if case.adds else set())
    for name, got in wrong.items():
        miss = rel_err(got, ref[:got.shape[0]])
        assert miss >= 100 * D.rtol(case), (name, miss)


def test_adds_variants_share_inputs_and_differ_by_the_adds():
    by_key = collections.defaultdict(list)
    for c in D.CASES:
        by_key[D._key(c)].append(c)
    for group in by_key.values():
        g0 = D.inputs(group[0])[0]
        for c in group:
            g, adds = D.inputs(c)
            assert g is g0 and len(adds) == c.adds and all(a.shape == D.dx_shape(c) for a in adds)
    c0, c2 = D.A_CASES[0], D.A_CASES[2]
    assert (c0.adds, c2.adds) == (0, 2) and D._key(c0) == D._key(c2)
    a1, a2 = D.inputs(c2)[1]
    assert torch.equal(D.reference(c2), (D.reference(c0) + torch.as_tensor(a1).double()) + torch.as_tensor(a2).double())


def test_table_has_no_duplicates_and_covers_every_path():
    assert len(set(D.CASES)) == len(D.CASES)
    assert len({D.case_id(c) for c in D.CASES}) == len(D.CASES)
    assert {c.path for c in D.A_CASES} == set(D.A_PATHS) and {c.path for c in D.B_CASES} == set(D.B_PATHS)
    assert set(D.PATHS) == set(D.A_PATHS) | set(D.B_PATHS)
    for path in D.PATHS:                                          # 0, 1 and 2 adds on every path of A; both adds somewhere on every path of B
        adds = {c.adds for c in D.CASES if c.path == path}
        assert adds == {0, 1, 2}, (path, adds)
    for path in D.A_PATHS:                                        # every path of A through the graph and through the C ABI
        drives = {c.drive for c in D.A_CASES if c.path == path}
        assert drives & {'graph', 'forced'} and drives & {'abi', 'auto'}, (path, drives)
    # both packers' both directions in one graph
    assert {(c.mode, c.path) for c in D.A_CASES if c.mode is not True} == {('bwd', 'f4_batch'), ('fwd', 'f2_batch')}
    # to_bn from 32, 33, 64 and 65 channels, from_bn to 32 and 64 (the ragged and the full last channel tile)
    assert {D.g_channels(c) for c in D.B_CASES if c.role == 'to_bn'} == {32, 33, 64, 65}
    assert {D.dx_shape(c)[1] for c in D.B_CASES if c.role == 'from_bn'} == {32, 64}
    for role in D.SCOPES:
        grids = {(c.N,) + D.dx_shape(c)[2:] if role in D.DECONV_ROLES else (c.N, c.H, c.W) for c in D.B_CASES if c.role == role}
        assert any(n == 1 and h % 2 and w % 2 and w % 16 and w > 16 and h * w > 256 for n, h, w in grids), role
        assert any(h == 1 for n, h, w in grids) and any(n == 2 for n, h, w in grids), role
    # the shapes part A asks for
    f2 = [(c.N, c.H, c.W) for c in D.A_CASES if c.path == 'f2_single' and c.drive == 'graph']
    assert any(h % 2 for n, h, w in f2) and any(w % 2 for n, h, w in f2) and any(w % 32 and not w % 2 for n, h, w in f2) and any(n > 1 for n, h, w in f2)
    direct = [(c.N, c.H, c.W) for c in D.A_CASES if c.path == 'direct']
    assert any(w % 2 for n, h, w in direct) and any(h * w < 16 for n, h, w in direct)
    assert all(isinstance(c.filt, int) for c in D.A_CASES if c.drive == 'graph' and c.path in ('f2_batch', 'f4_batch'))
    assert all(c.filt == 'random' for c in D.A_CASES if c.path == 'f2_single')
    assert any(h % 4 for n, h, w in D.F4_SHAPES) and (30, 40, 40) in D.F4_SHAPES
    assert {(c.N, c.H, c.W) for c in D.A_CASES if c.path == 'f4_batch' and c.drive == 'graph' and c.mode is True} == set(D.F4_SHAPES)


def test_filters_are_the_graphs_own_and_have_no_symmetry():
    w = D.random_filter()
    assert not (w == w[::-1, ::-1]).all() and not (w == w.transpose(0, 1, 3, 2)).all()
    for cfg in D.CONFIGS:
        names = D.w3_names(cfg)
        assert len(names) == 64 and len(set(names)) == 64 and all(D.weights(cfg)[n].shape == (3, 3, 128, 128) for n in names)
    shapes = {(c.role, c.config): D.filter_of(c).shape for c in D.B_CASES}
    assert shapes[('h1', 'low')] == (5, 5, 3, 64) and shapes[('h2', 'low')] == (5, 5, 64, 128) and shapes[('h12', 'low')] == (5, 5, 64, 128)
    assert shapes[('h13', 'low')] == (5, 5, 3, 64) and shapes[('from_bn', 'low')] == (3, 3, 128, 32) and shapes[('from_bn', 'hi')] == (3, 3, 128, 64)
    assert [shapes[('to_bn', c)][3] for c in ('low', 'hi', 'low_nohm', 'hi_nohm')] == [33, 65, 32, 64]


def test_cases_take_the_paths_the_table_says_by_the_library_queries():
    """the part of the GPU tests' path assertions that is host arithmetic (ic_conv3x3_c128_pick_algo, ic_wino4_3x3_c128_supported,
    ic_wino4_3x3_c128_workgroups, ic_conv2d_mfma_packed_floats: no device call)"""
    from imgcomp_cvpr_amd import _lib as L
    for c in D.CASES:
        assert D.expected_plan(L, c), D.case_id(c)
    # the F(4x4) cases are the smallest batches that fit: one image less does not
    for N, H, W in D.F4_SMALLEST:
        assert D.f4_fits(L.lib, N, H, W) and not D.f4_fits(L.lib, N - 1, H, W), (N, H, W)
        assert L.lib.ic_wino4_3x3_c128_workgroups(N, H, W) == 160
    assert D.f4_fits(L.lib, 30, 40, 40) and L.lib.ic_conv3x3_c128_pick_form(30, 40, 40, 0) == 2
    # the library's answer is 0 (direct) by itself only from 2 GiB a map on: what DIRECT_NOTE says
    assert L.lib.ic_conv3x3_c128_pick_algo(1, 2048, 2048, 0) == 0 and L.lib.ic_conv3x3_c128_pick_algo(1, 2048, 2047, 0) == 1
    assert all(L.lib.ic_conv3x3_c128_pick_algo(c.N, c.H, c.W, 0) == 1 for c in D.A_CASES)
