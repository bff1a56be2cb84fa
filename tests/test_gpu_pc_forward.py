"""-m gpu: the context model's forward pass (csrc/probclass.hip, pc_forward) on every kernel it chooses among, against the
float64 oracle (oracle.bitcost) on the cases of tests/pc_cases.py -- weights whose channels are all live behind their ReLUs
(tests/test_cpu_pc_cases.py asserts it), so a wrong filter column, bias or fragment row of ANY channel moves a logit.

Every (k, L) group runs all volumes of its k; per volume: logits and bits of bitcost(return_logits=True) against the oracle at
RTOL, and bit for bit the same numbers from bitcost without logits (the kernels' `out == NULL` branch), from logits_unpadded,
from logits() on the oracle-padded volume (another first-layer kernel) and from the C ABI with a table WITHOUT packed filters
(per-call packing into the workspace), the last one into NaN-filled outputs over a NaN-filled workspace.

k = 24 (conv0: pc_conv0_k24_kernel, pre-padded: pc_conv3d_kernel<24, first, contiguous>; middle layers: pc_mfma_kernel<24, 24> in
the tile ic_pc_mid_tile names: 0 = 8 x 16, 1 = 5 x 25, 2 = 6 x 21; final: pc_final16_kernel<24, 24, 6> for L = 6, <24, 24> with
run-time L otherwise), L in 2, 3, 6, 8, 11, 16:

| N, C, h, w  | res1/conv1 plane, tile | res1/conv2 plane, tile | reaches                                                        |
| 1, 1, 1, 1  | 5 x 5, 0               | 3 x 3, 0               | all halo: one voxel behind four layers of padding              |
| 2, 5, 7, 11 | 11 x 15, 0             | 9 x 13, 0              | two images                                                     |
| 1, 2, 1, 21 | 5 x 25, 1              | 3 x 23, 1              | exactly one 5 x 25 tile; a final tile row of one voxel row     |
| 1, 3, 2, 17 | 6 x 21, 2              | 4 x 19, 1              | exactly one 6 x 21 tile (its last wave has 30 of 32 voxels)    |
| 1, 2, 4, 19 | 8 x 23, 0              | 6 x 21, 2              | two 8 x 16 tiles side by side, the second 7 wide               |
| 1, 3, 9, 17 | 13 x 21, 1             | 11 x 19, 2             | three / two tile rows with a remainder; the final 8 x 16 grid  |
|             |                        |                        | has a one-row and a one-column remainder                       |
| 1, 1, 8, 16 | 12 x 20, 2             | 10 x 18, 1             | exactly one final tile, one channel                            |
| 1, 1, 2, 38 | 6 x 42, 2              | 4 x 40, 1              | two tiles side by side in 6 x 21 and in 5 x 25 (40 = 25 + 15)  |

k = 64 (conv0 and pre-padded: pc_conv3d_kernel<8, first>; middle: pc_mfma_kernel<64, 16, 2, 2, 4, 16>, tile 3; final:
pc_final16_kernel<64, 16, 6> / <64, 16>), L in 6, 11, 16: (1,6,5,9), (2,2,3,13), (1,3,9,17) -- the 4 x 16 tile is ragged in both
directions on the last two.

k = 8 and k = 20 (no matrix-core path: pc_conv3d_kernel<8> in all layers; 20 is no multiple of its 8-channel block, so the last
block's filter offsets clamp), L = 6 (final kernel with 8 channels a lane) and L = 11 (16): (2,3,5,7), (1,1,1,1).

Bounds: RTOL of tests/util.py for every group, the bar test_pc_bitcost_and_logits holds.  For scale: the oracle evaluated in float32
on the CPU differs from float64 by 3e-7 .. 7e-7 (logits) and 2e-7 .. 3e-7 (bits) on these cases, every group alike."""
import math

import pytest
import torch

from tests import pc_cases as P
from tests.util import RTOL, assert_close, dev

pytestmark = pytest.mark.gpu

# the k = 24 list reaches all three tiles in both middle layers (the picks themselves are asserted against the library's query
# in every test that runs a volume)
for _layer in (0, 1):
    assert {t[_layer] for t in P.K24_VOLUMES.values()} == {0, 1, 2}


def _L():
    from imgcomp_cvpr_amd import _lib
    return _lib


def _net(cuda, k, L, wts=None):
    from imgcomp_cvpr_amd import probclass
    _, pc_cfg = P.configs(k, L)
    return probclass.get_network_cls(pc_cfg)(pc_cfg, num_centers=L).load_weights(P.weights(k, L) if wts is None else wts, cuda)


def _assert_tiles(k, shape, tiles):
    mid = _L().lib.ic_pc_mid_tile
    N, C, h, w = shape
    assert (mid(k, h + 4, w + 4), mid(k, h + 2, w + 2)) == tiles, 'volume {} does not reach the tiles it is listed for'.format(shape)


def _abi_bitcost(pc, tab, qd, symd, pad, k, L, short=0, claim_L=None):
    """ic_pc_bitcost_f32 through the C ABI with a table of the caller's: NaN-filled logits and bits over a workspace of NaN bit
    patterns (short: that many bytes less than asked for).  -> (return code, bits, logits)"""
    lib = _L()
    N, C, h, w = qd.shape
    cl = L if claim_L is None else claim_L
    bits = torch.full((N, C, h, w), float('nan'), device=qd.device)
    logits = torch.full((N, C, h, w, cl), float('nan'), device=qd.device)
    need = lib.lib.ic_pc_workspace_bytes(N, C, h, w, k)
    ws = torch.full((need,), 0xff, dtype=torch.uint8, device=qd.device)
    rc = lib.lib.ic_pc_bitcost_f32(lib.ptr(qd), lib.ptr(symd), tab, k, cl, pad, lib.ptr(logits), lib.ptr(bits), N, C, h, w,
                                   lib.ptr(ws), need - short, lib.current_stream(qd.device))
    torch.cuda.synchronize()
    return rc, bits, logits


def _check_group(cuda, k, L):
    from oracle import oracle as O
    lib = _L()
    pc = _net(cuda, k, L)
    assert (lib.lib.ic_pc_packed_floats(k, L) > 0) == (k in (24, 64)) and (pc._tab_tensors[8] is not None) == (k in (24, 64))
    unpacked = lib.ptr_table(pc._tab_tensors[:8] + [None])
    for shape, tiles in P.volumes(k).items():
        _assert_tiles(k, shape, tiles)
        q, sym, pad = P.inputs(k, L, shape)
        qd, symd = dev(q, cuda), dev(sym, cuda, torch.int64)
        what = 'k = {} L = {} shape {}'.format(k, L, shape)
        bits, logits = pc.bitcost(qd, symd, False, pad_value=pad, return_logits=True)
        rb, rl = P.reference(k, L, shape)
        assert_close(logits, rl, 'pc forward logits ' + what, rtol=RTOL)
        assert_close(bits, rb, 'pc forward bits ' + what, rtol=RTOL)
        assert torch.equal(pc.bitcost(qd, symd, False, pad_value=pad), bits), 'bits without logits differ: ' + what
        assert torch.equal(pc.logits_unpadded(qd, pad), logits), 'logits_unpadded differs: ' + what
        qp = O.pad_for_probclass3d(torch.as_tensor(q), 9, pad)
        assert torch.equal(pc.logits(dev(qp.numpy(), cuda), False), logits), 'logits() on the padded volume differs: ' + what
        # the table without packed filters: every call packs into its workspace (k = 24, 64), or there is nothing to pack
        rc, b2, l2 = _abi_bitcost(pc, unpacked, qd, symd, pad, k, L)
        assert rc == 0
        assert torch.equal(b2, bits) and torch.equal(l2, logits), 'per-call packing / NaN-filled outputs differ: ' + what


@pytest.mark.parametrize('k,L', P.MFMA_GROUPS)
def test_matrix_core_paths(cuda, k, L):
    """logits and bits of the matrix-core kernels for k = 24 and k = 64 at every supported kind of L, on every middle-layer tile
    (module docstring); the per-call packing branch gives the bits of the load-time packing."""
    _check_group(cuda, k, L)


@pytest.mark.parametrize('k,L', P.VALU_GROUPS)
def test_valu_paths(cuda, k, L):
    """the any-shape kernels for a k without a matrix-core path, k = 20 with a partly filled last channel block"""
    assert _L().lib.ic_pc_packed_floats(k, L) == 0 and _L().lib.ic_pc_mid_tile(k, 9, 11) == -1
    _check_group(cuda, k, L)


@pytest.mark.parametrize('k,L', P.EDGE_GROUPS)
def test_cross_entropy_epilogue_at_its_numeric_edges(cuda, k, L):
    """logits far apart (spread > 90: expf of the others underflows, a ruled-out target costs > 100 bits) and all logits
    clamped to zero (every symbol costs log2(L) bits, the logits are exactly 0)."""
    shape = P.EDGE_VOLUME
    what = 'k = {} L = {} shape {}'.format(k, L, shape)
    far = P.far_apart_weights(k, L)
    q, sym, pad = P.inputs(k, L, shape, far)
    qd, symd = dev(q, cuda), dev(sym, cuda, torch.int64)
    rb, rl = P.reference_with(far, k, L, shape)
    assert float((rl.max(-1).values - rl.min(-1).values).max()) > 90 and float(rb.max()) > 100
    bits, logits = _net(cuda, k, L, far).bitcost(qd, symd, False, pad_value=pad, return_logits=True)
    assert bool(torch.isfinite(bits).all()) and bool(torch.isfinite(logits).all())
    assert_close(logits, rl, 'pc forward logits far apart ' + what, rtol=RTOL)
    assert_close(bits, rb, 'pc forward bits far apart ' + what, rtol=RTOL)

    clamped = P.all_clamped_weights(k, L)
    rb, rl = P.reference_with(clamped, k, L, shape)
    bits, logits = _net(cuda, k, L, clamped).bitcost(qd, symd, False, pad_value=pad, return_logits=True)
    assert not bool(logits.any()), 'a logit survived a bias of -1e3'
    assert not bool(rl.any()) and abs(float(rb.max()) - math.log2(L)) < 1e-12 and abs(float(rb.min()) - math.log2(L)) < 1e-12
    assert_close(bits, rb, 'pc forward bits all clamped ' + what, rtol=RTOL)


def test_refusals_leave_the_outputs_untouched(cuda):
    """L = 17: unsupported; a workspace one byte short: the workspace code; both before anything is written"""
    k, L, shape = 24, 16, (1, 2, 4, 19)
    pc = _net(cuda, k, L)
    q, sym, pad = P.inputs(k, L, shape)
    qd, symd = dev(q, cuda), dev(sym, cuda, torch.int64)
    for tab in (pc._tab, _L().ptr_table(pc._tab_tensors[:8] + [None])):
        rc, bits, logits = _abi_bitcost(pc, tab, qd, symd, pad, k, L, claim_L=17)
        assert rc == -2 and bool(torch.isnan(bits).all()) and bool(torch.isnan(logits).all())
        rc, bits, logits = _abi_bitcost(pc, tab, qd, symd, pad, k, L, short=1)
        assert rc == -3 and bool(torch.isnan(bits).all()) and bool(torch.isnan(logits).all())
    rc, bits, logits = _abi_bitcost(pc, pc._tab, qd, symd, pad, k, L)
    assert rc == 0 and not bool(torch.isnan(bits).any()) and not bool(torch.isnan(logits).any())
