"""The cases of tests/pc_bwd_cases.py are what tests/test_gpu_pc_data_grad.py takes them for (no GPU: float64 on the CPU and the
host side of the library).  The conditions below are conditions on the INPUTS and on the table: a case that misses one gets another
shape or seed, never a weaker condition."""
import numpy as np
import pytest
import torch

from tests import pc_bwd_cases as B
from tests.util import rel_err

SMALL = 1 << 22          # N * Cin * Cout * positions of dx up to which the explicit sum over taps is evaluated as well


def _most(c):
    """one variant per (shape, mask kind): the one with the residual and the ReLU mask where the shape has them"""
    same = [k for k in B.CASES if B.shape_of(k) == B.shape_of(c) and k.first_mask == c.first_mask]
    return c == max(same, key=lambda k: (k.res, k.relu_mask))


@pytest.mark.parametrize('case', [c for c in B.CASES if _most(c)], ids=B.case_id)
def test_reference_is_the_adjoint_and_the_inputs_can_fail(case):
    """the autograd reference equals the data gradient stated independently -- the transposed convolution with the masked filter,
    and on the small cases the explicit sum over the live taps in numpy -- to 1e-12 of the tensor scale; each mistake of
    pc_bwd_cases.mistakes() misses it by 100 x the tolerance or more."""
    ref = B.reference(case)
    assert tuple(ref.shape) == B.dx_shape(case) and ref.dtype == torch.float64
    assert rel_err(B.finish(case, B.by_conv_transpose(case)), ref) <= 1e-12
    if case.N * case.Cin * case.Cout * int(np.prod(B.dx_shape(case)[2:])) <= SMALL:
        assert rel_err(B.finish(case, B.by_taps(case)), ref) <= 1e-12
    wrong = B.mistakes(case)
    expect = {'taps not mirrored', 'rows not mirrored', 'mask ignored', 'first and other mask swapped'}
    if case.res:
        expect.add('residual at offset (1, 1, 1)')
    if case.relu_mask:
        expect |= {'mask taken as act >= 0', 'mask taken as act != 0'}
    if case.res and case.relu_mask:
        expect.add('residual added after the mask')
    assert set(wrong) == expect
    for name, got in wrong.items():
        miss = rel_err(got, ref)
        assert miss >= 100 * B.RTOL, (name, miss)


def test_variants_share_inputs_and_differ_by_residual_and_mask():
    for c in B.CASES:
        g, w, act, res = B.inputs(c)
        assert g.shape == (c.N, c.Cout, c.OD, c.OH, c.OW) and w.shape == (2, 3, 3, c.Cin, c.Cout)
        assert act.shape == B.dx_shape(c) and all(a.dtype == np.float32 and not a.flags.writeable for a in (g, w, act, res))
        if c.res:
            assert B.has_room_for_res(c) and res.shape == B.res_shape(c)
        zeros, neg = float((act == 0).mean()), int((act < 0).sum())
        assert 0.35 <= zeros <= 0.6 and 1 <= neg <= act.size // 16 + 1, (B.case_id(c), zeros, neg)
        same = [k for k in B.CASES if B.shape_of(k) == B.shape_of(c)]
        assert all(B.inputs(k)[0] is g for k in same)
    full, bare = [next(c for c in B.CASES if c.path == 'mfma24_c24' and c.OH == 7 and (c.res, c.relu_mask) == v) for v in ((True, True), (False, False))]
    _, _, act, res = B.inputs(full)
    want = B.reference(bare).clone()
    want[:, :, 2:, 2:-2, 2:-2] += torch.tensor(res).double()
    assert torch.equal(B.reference(full), want * (torch.tensor(act) > 0))
    assert not bool(B.reference(full)[torch.tensor(act) <= 0].any())


def test_table_conditions():
    assert len(set(B.CASES)) == len(B.CASES) and len({B.case_id(c) for c in B.CASES}) == len(B.CASES)
    assert {c.path for c in B.CASES} == set(B.PATHS) and set(B.MFMA_PATHS) == set(B.TILE) == set(B.CIN) == set(B.COUTS)
    for path in B.MFMA_PATHS:
        cs = [c for c in B.CASES if c.path == path]
        tr, tc = B.TILE[path]
        assert all(c.Cin == B.CIN[path] and c.first_mask == 0 for c in cs)
        planes = {(c.OH + 2, c.OW + 2) for c in cs}
        assert (tr, tc) in planes and (tr + 1, tc + 1) in planes, (path, planes)           # one tile; a row and a column more
        assert B.tiles(next(c for c in cs if (c.OH + 2, c.OW + 2) == (tr, tc))) == (1, 1)
        assert B.tiles(next(c for c in cs if (c.OH + 2, c.OW + 2) == (tr + 1, tc + 1))) == (2, 2)
        assert any((c.OD, c.OH, c.OW) == (1, 1, 1) and not c.res for c in cs)                # all halo
        assert any(c.N == 3 and min(B.tiles(c)) >= 2 for c in cs)                            # several tiles, three images
        assert any(c.N == 1 for c in cs)
        wgs = {B.workgroups(c) for c in cs}
        assert any(n < 8 for n in wgs) and any(n % 8 == 0 for n in wgs) and any(n >= 8 and n % 8 for n in wgs), (path, wgs)
        assert {c.Cout for c in cs} >= B.COUTS[path], path
        assert all((c.Cout <= 24) == path.startswith('mfma24') and c.Cout <= 64 for c in cs)
        # one shape with room for the residual in all four combinations of residual and mask
        combos = {}
        for c in cs:
            if B.has_room_for_res(c):
                combos.setdefault(B.shape_of(c), set()).add((c.res, c.relu_mask))
        assert any(len(v) == 4 for v in combos.values()), path
        assert any((c.N, c.OD, c.OH, c.OW) == (2, 3, 9, 21) for c in cs)                     # the old test's volume
    assert B.Case('mfma24_c24', 2, 24, 24, 9, 18, 18, 0, True, True) in B.CASES             # training proportions
    assert {c.Cout for c in B.CASES if c.path in ('mfma24_c24', 'mfma24_c64')} >= {24} and 25 in B.COUTS['mfma64_c64']
    valu = [c for c in B.CASES if c.path == 'valu']
    assert {c.Cin for c in valu} >= {1, 5, 12, 20} and any(c.Cin % 8 == 0 for c in valu)
    assert {(c.Cin, c.Cout) for c in valu if c.first_mask} >= {(1, 24), (5, 7)}
    assert any(c.first_mask and c.Cin > 8 and c.Cin % 8 for c in valu)
    ivols = [int(np.prod(B.dx_shape(c)[2:])) for c in valu]
    assert any(v < 256 for v in ivols) and any(v > 256 and v % 256 for v in ivols)
    assert any((c.Cin, c.Cout) == (24, 40) for c in valu) and any((c.Cin, c.Cout) == (24, 65) for c in valu)
    for path in B.PATHS:                                               # every mistake of mistakes() is tried on every path
        assert any(c.path == path and c.res and c.relu_mask and _most(c) for c in B.CASES), path
    for c in B.CASES:                                                  # "a few seconds": the largest dx has about 0.4 M values
        assert int(np.prod(B.dx_shape(c))) <= 400000 and c.res <= B.has_room_for_res(c), B.case_id(c)
        assert c.path == B.expected_path(c), B.case_id(c)


def test_cases_take_the_paths_the_table_says_by_the_library_query():
    """ic_pc_bwd_data_workspace_bytes is host arithmetic: non-zero exactly on the matrix-core cases (the GPU test runs each of
    those once more without a workspace, which is the any-shape kernel on the same shape).  Cin = 24 with 25 .. 64 gradient
    channels answers 0: the KP = 64 kernel reads two 32-row fragment tiles and 24 rows pack into one, so the library sends the
    shape to the any-shape kernel."""
    from imgcomp_cvpr_amd import _lib as L
    for c in B.CASES:
        assert (B.query(L.lib, c) > 0) == c.path.startswith('mfma'), B.case_id(c)
    q = L.lib.ic_pc_bwd_data_workspace_bytes
    for N, OD, OH, OW in ((2, 3, 9, 21), (1, 1, 1, 1), (2, 9, 18, 18)):
        for Cin, Cout in B.QUERY_ZERO:
            assert q(N, Cin, Cout, OD, OH, OW) == 0, (Cin, Cout, (N, OD, OH, OW))
        for Cin, Cout in ((24, 1), (24, 24), (64, 1), (64, 24), (64, 25), (64, 64)):
            assert q(N, Cin, Cout, OD, OH, OW) > 0, (Cin, Cout)
        assert q(N, 64, 65, OD, OH, OW) == 0 and q(N, 32, 24, OD, OH, OW) == 0
    # the answer is the padded gradient + the packed fragments + 64 zero floats: KP channels, 14 taps, 32-row tiles
    c = next(c for c in B.CASES if c.path == 'mfma64_c64')
    pad = c.N * 64 * (c.OD + 2) * (c.OH + 4) * (c.OW + 4)
    assert B.query(L.lib, c) == 4 * (pad + (64 // 8) * 14 * 2 * 256 + 64)
    c = next(c for c in B.CASES if c.path == 'mfma24_c64')
    pad = c.N * 24 * (c.OD + 2) * (c.OH + 4) * (c.OW + 4)
    assert B.query(L.lib, c) == 4 * (pad + (24 // 8) * 14 * 2 * 256 + 64)


@pytest.mark.parametrize('Cout', [25, 40, 64])
def test_cin_24_with_more_than_24_gradient_channels_is_not_offered_the_matrix_cores(Cout):
    """pc_pack_adjoint_kernel packs ceil(24 / 32) = 1 row tile, pc_mfma_kernel<64,16,2,2,..> indexes gridDim.y * WM = 2: the
    query must answer 0, so that ic_pc_bwd_data_f32 runs the any-shape kernel whatever buffer it is handed"""
    from imgcomp_cvpr_amd import _lib as L
    assert L.lib.ic_pc_bwd_data_workspace_bytes(2, 24, Cout, 3, 9, 21) == 0
    assert L.lib.ic_pc_bwd_data_workspace_bytes(2, 24, 24, 3, 9, 21) > 0 and L.lib.ic_pc_bwd_data_workspace_bytes(2, 64, Cout, 3, 9, 21) > 0


@pytest.mark.parametrize('k', [24, 64])
def test_training_calls_get_the_matrix_cores(k):
    """the three calls of TrainGraph._pc_backward (final layer k -> L, res1/conv2 and res1/conv1 k -> k) at L = 6,
    (N, C, h, w) = (2, 32, 16, 16)"""
    from imgcomp_cvpr_amd import _lib as L
    N, C, h, w, nl = 2, 32, 16, 16, 6
    for Cout, OD, OH, OW in ((nl, C, h, w), (k, C + 1, h + 2, w + 2), (k, C + 2, h + 4, w + 4)):
        assert L.lib.ic_pc_bwd_data_workspace_bytes(N, k, Cout, OD, OH, OW) > 0, (k, Cout)
