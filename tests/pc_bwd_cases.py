"""Cases for the parity tests of ic_pc_bwd_data_f32, the data gradient of the context model's masked VALID conv3d
(csrc/train_pc.hip, csrc/probclass.hip; TrainGraph._pc_backward calls it three times a step).  This file is the table of cases,
their seeded inputs and their float64 references (a test helper: no device code).  tests/test_gpu_pc_data_grad.py runs the
kernels on them, tests/test_cpu_pc_bwd_cases.py checks the table itself.

  dx[n][ci][u] = ( sum_{live taps t, co} g[n][co][u - off(t)] * w[t][ci][co]  (+ res[n][ci][u - (2,2,2)] when inside) ) * [act > 0]
  g (N, Cout, OD, OH, OW)    w (2, 3, 3, Cin, Cout)    dx, act (N, Cin, OD+1, OH+2, OW+2)    res (N, Cin, OD-1, OH-2, OW-2)

Reference: float64 autograd of F.conv3d(x, (w * mask).permute(4, 3, 0, 1, 2)) with respect to x, mask from oracle.pc_masks(3);
res added at offset (2, 2, 2), then the product with [act > 0].  No product code.

Paths (PATHS below says what runs).  The matrix-core kernels walk the plane (OH + 2, OW + 2) of dx in tiles (TILE) with one
work-group per (depth slice, tile): (OD + 1) * tiles_y * tiles_x work-groups an image, renumbered by ic_xcd_run, which permutes the
first 8 * (count // 8) of them and leaves the tail in place.  The gradient's channels are zero-padded to KP = 24 (Cout <= 24) or
64; the rows of the GEMM are the layer's Cin input channels in tiles of 32.

A case's path is what the library's workspace query makes of its shape (non-zero: a matrix-core path), so the table lists no
matrix-core shape a second time under 'valu': the GPU test runs every matrix-core case once more without a workspace."""
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

PATHS = {
    'mfma24_c24': 'pc_pad_grad + pc_pack_adjoint + pc_mfma_kernel<24,24,1,4,8,16,false,true>, one row tile + pc_bwd_fix_kernel',
    'mfma24_c64': 'the same kernel with Cin = 64: two row tiles through gridDim.y (the second one full: 64 = 2 * 32)',
    'mfma64_c64': 'pc_pad_grad + pc_pack_adjoint + pc_mfma_kernel<64,16,2,2,4,16,false,true> + pc_bwd_fix_kernel',
    'valu': 'pc_bwd_data_kernel<8>: no workspace, or a shape whose workspace query answers 0',
}
MFMA_PATHS = ('mfma24_c24', 'mfma24_c64', 'mfma64_c64')
TILE = {'mfma24_c24': (8, 16), 'mfma24_c64': (8, 16), 'mfma64_c64': (4, 16)}
CIN = {'mfma24_c24': 24, 'mfma24_c64': 64, 'mfma64_c64': 64}
COUTS = {'mfma24_c24': {3, 6, 16, 24}, 'mfma24_c64': {6, 16}, 'mfma64_c64': {25, 40, 64}}       # what each path must have run
RTOL = 1e-5          # of the tensor scale: the bar of test_pc_data_gradient_matrix_core_path and of the 3-D filter gradient

# res: the residual is passed (a volume with OD = 1, OH <= 2 or OW <= 2 has none: RD, RH or RW is 0); relu_mask: act is passed
Case = namedtuple('Case', 'path N Cin Cout OD OH OW first_mask res relu_mask')


def _all4(path, N, Cin, Cout, OD, OH, OW):
    return [Case(path, N, Cin, Cout, OD, OH, OW, 0, res, mask) for res in (True, False) for mask in (True, False)]


def _mfma(path, couts, old_cout):
    """one path's list.  couts = the Cout of (one tile, second tile, all halo, N = 3), old_cout that of the earlier test's volume.
    The all-halo case gets a Cout above 8: with one live tap an output and at most 8 gradient channels the matrix-core sum IS the
    VALU kernel's fmaf chain (one 8-channel group, in channel order), and the GPU test asserts that the two kernels differ."""
    th, Cin = TILE[path][0], CIN[path]
    c_one, c_second, c_halo, c_n3 = couts
    return ([Case(path, 1, Cin, c_one, 1, th - 2, 14, 0, False, True)]              # exactly one tile; 2 work-groups
            + _all4(path, 2, Cin, c_second, 3, th - 1, 15)                           # a row and a column into a second tile; 16
            + [Case(path, 1, Cin, c_halo, 1, 1, 1, 0, False, True)]                  # all halo: every output sees one tap at most
            + [Case(path, 3, Cin, c_n3, 2, 9, 21, 0, True, True)]                    # 11 x 23: 2 x 2 (12) resp. 3 x 2 tiles (18)
            + [Case(path, 2, Cin, old_cout, 3, 9, 21, 0, True, True)])               # test_pc_data_gradient_matrix_core_path's


CASES = (
    _mfma('mfma24_c24', (3, 6, 24, 16), 24)
    + [Case('mfma24_c24', 2, 24, 24, 9, 18, 18, 0, True, True)]                      # training proportions: 10 x 3 x 2 = 60
    + _mfma('mfma24_c64', (6, 16, 16, 16), 6)
    + [Case('mfma24_c64', 1, 64, 24, 2, 3, 3, 0, False, False)]                      # KP = 24 filled, no epilogue kernel at all
    + _mfma('mfma64_c64', (64, 25, 40, 40), 64)
    + [
        # ---- the any-shape kernel: 256 positions x 8 input channels a work-group
        Case('valu', 1, 1, 24, 1, 2, 3, 1, False, True),          # first mask; 40 positions: under one block; one channel of 8
        Case('valu', 2, 5, 7, 2, 5, 9, 1, True, True),            # first mask; 231 positions
        Case('valu', 2, 5, 7, 3, 6, 10, 0, True, False),          # the same widths under the other mask; 384 positions
        Case('valu', 2, 12, 6, 3, 7, 11, 0, True, True),          # 8 + 4 channels; 468 positions: two blocks, the second ragged
        Case('valu', 1, 20, 24, 2, 6, 10, 0, False, True),        # 8 + 8 + 4 channels; 288 positions
        Case('valu', 3, 20, 16, 2, 4, 5, 1, True, True),          # first mask with a ragged last channel block, three images
        Case('valu', 1, 8, 24, 2, 5, 7, 0, True, True),           # exactly one channel block (no matrix-core path: Cin = 8)
        Case('valu', 2, 24, 40, 2, 7, 15, 0, True, True),         # Cin = 24 with Cout above 24: the query answers 0
        Case('valu', 1, 24, 65, 1, 3, 5, 0, False, True),         # Cout above 64
    ]
)
QUERY_ZERO = [(24, 40), (8, 24), (24, 65), (24, 25), (24, 64)]    # (Cin, Cout) whose workspace query is 0 at any volume


def case_id(c):
    return '{}-{}x{}to{}-{}x{}x{}-first{}-res{}-mask{}'.format(c.path, c.N, c.Cin, c.Cout, c.OD, c.OH, c.OW, c.first_mask, int(c.res),
                                                               int(c.relu_mask))


def shape_of(c):
    return (c.N, c.Cin, c.Cout, c.OD, c.OH, c.OW)


def dx_shape(c):
    return (c.N, c.Cin, c.OD + 1, c.OH + 2, c.OW + 2)


def res_shape(c):
    return (c.N, c.Cin, c.OD - 1, c.OH - 2, c.OW - 2)


def has_room_for_res(c):
    return c.OD >= 2 and c.OH >= 3 and c.OW >= 3


def tiles(c):
    """(tiles_y, tiles_x) of a matrix-core case"""
    tr, tc = TILE[c.path]
    return -(-(c.OH + 2) // tr), -(-(c.OW + 2) // tc)


def workgroups(c):
    """gridDim.x of the matrix-core kernel: what ic_xcd_run renumbers"""
    ty, tx = tiles(c)
    return (c.OD + 1) * ty * tx


# ---- inputs ---------------------------------------------------------------------------------------------------------------------

def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    N, Cin, Cout, OD, OH, OW = shape
    rs = np.random.RandomState(_seed('pc bwd data', shape))
    g = rs.normal(0, 1, (N, Cout, OD, OH, OW)).astype(np.float32)
    w = rs.normal(0, 0.1, (2, 3, 3, Cin, Cout)).astype(np.float32)
    act = np.maximum(rs.normal(0, 1, (N, Cin, OD + 1, OH + 2, OW + 2)), 0).astype(np.float32)     # post-ReLU: half exact zeros
    act.reshape(-1)[3::17] = -0.75                 # and a few negative entries, which no ReLU output has: the mask is act > 0
    res = rs.normal(0, 1, (N, Cin, max(OD - 1, 0), max(OH - 2, 0), max(OW - 2, 0))).astype(np.float32)
    for a in (g, w, act, res):
        a.setflags(write=False)
    return g, w, act, res


def inputs(c):
    """-> (g, w, act, res) float32, seeded by the shape alone: shared by the mask / residual / first-mask variants, read-only"""
    return _inputs(shape_of(c))


def masks():
    """{first_mask: (2, 3, 3) float64}"""
    from oracle import oracle as O
    first, other = O.pc_masks(3)
    return {1: first.astype(np.float64), 0: other.astype(np.float64)}


# ---- references -----------------------------------------------------------------------------------------------------------------

def masked_filter(c, first_mask=None):
    """(w * mask) as the conv3d filter (Cout, Cin, 2, 3, 3), float64"""
    w = torch.tensor(inputs(c)[1]).double()
    m = torch.tensor(masks()[c.first_mask if first_mask is None else first_mask])
    return (w * m[..., None, None]).permute(4, 3, 0, 1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def _raw_reference(shape, first_mask):
    import torch.nn.functional as F
    c = Case('valu', *shape, first_mask, False, False)
    torch.set_num_threads(16)
    x = torch.zeros(dx_shape(c), dtype=torch.float64, requires_grad=True)           # the layer is linear: dX does not depend on x
    y = F.conv3d(x, masked_filter(c))
    g = torch.tensor(inputs(c)[0]).double()
    assert y.shape == g.shape, (y.shape, g.shape)
    y.backward(g)
    return x.grad.detach()


def finish(c, raw, res_offset=2, mask='gt', res_after_mask=False):
    """raw (+ res embedded at res_offset) * [act > 0], float64.  The keywords state the mistakes of mistakes()."""
    _, _, act, res = inputs(c)
    out = raw.clone()
    act = torch.tensor(act)
    keep = {'gt': act > 0, 'ge': act >= 0, 'ne': act != 0}[mask].double()

    def add_res(t):
        if c.res:
            o = res_offset
            t[:, :, o:o + c.OD - 1, o:o + c.OH - 2, o:o + c.OW - 2] += torch.tensor(res).double()
        return t
    if res_after_mask:
        return add_res(out * keep if c.relu_mask else out)
    out = add_res(out)
    return out * keep if c.relu_mask else out


def reference(c):
    """float64 autograd of the masked conv3d (once per (shape, mask kind), shared) + the case's residual and ReLU mask"""
    assert not c.res or has_room_for_res(c)
    return finish(c, _raw_reference(shape_of(c), c.first_mask))


def by_taps(c, mirrored=True, mask=None):
    """the raw data gradient as the explicit sum over the live taps, in numpy float64:
       dx[n, ci, od + kd, oy + kh, ox + kw] += sum_co g[n, co, od, oy, ox] * w[kd, kh, kw, ci, co]      for mask[kd, kh, kw] != 0
    mirrored = False: the tap's filter slice read at (1 - kd, 2 - kh, 2 - kw) -- the gradient scattered as the forward layer gathers;
    a triple of booleans: per axis (depth, rows, columns); mask: another (2, 3, 3) mask."""
    g, w, _, _ = inputs(c)
    g, w = g.astype(np.float64), w.astype(np.float64)
    mask = masks()[c.first_mask] if mask is None else mask
    md, mh, mw = (mirrored,) * 3 if isinstance(mirrored, bool) else mirrored
    dx = np.zeros(dx_shape(c), np.float64)
    for kd in range(2):
        for kh in range(3):
            for kw in range(3):
                sd, sh, sw = (kd if md else 1 - kd), (kh if mh else 2 - kh), (kw if mw else 2 - kw)
                if mask[sd, sh, sw] == 0:
                    continue
                dx[:, :, kd:kd + c.OD, kh:kh + c.OH, kw:kw + c.OW] += np.einsum('nodhw,io->nidhw', g, w[sd, sh, sw])
    return torch.as_tensor(dx)


def by_conv_transpose(c):
    """the raw data gradient as the transposed convolution of g with the masked filter (no autograd)"""
    import torch.nn.functional as F
    torch.set_num_threads(16)
    return F.conv_transpose3d(torch.tensor(inputs(c)[0]).double(), masked_filter(c))


def mistakes(c):
    """plausible mistakes -> {name: result}; the ones about the residual / the ReLU mask only where the case has them"""
    raw = _raw_reference(shape_of(c), c.first_mask)
    out = {'taps not mirrored': finish(c, by_taps(c, mirrored=False)),
           'rows not mirrored': finish(c, by_taps(c, mirrored=(True, False, True))),
           'mask ignored': finish(c, by_taps(c, mask=np.ones((2, 3, 3)))),
           'first and other mask swapped': finish(c, by_taps(c, mask=masks()[1 - c.first_mask]))}
    if c.res:
        out['residual at offset (1, 1, 1)'] = finish(c, raw, res_offset=1)
    if c.relu_mask:
        out['mask taken as act >= 0'] = finish(c, raw, mask='ge')
        out['mask taken as act != 0'] = finish(c, raw, mask='ne')
    if c.res and c.relu_mask:
        out['residual added after the mask'] = finish(c, raw, res_after_mask=True)
    return out


# ---- which path a case takes, by the library's host-side query -------------------------------------------------------------------

def query(lib, c):
    return int(lib.ic_pc_bwd_data_workspace_bytes(c.N, c.Cin, c.Cout, c.OD, c.OH, c.OW))


def expected_path(c):
    """the dispatch of ic_pc_bwd_data_f32 restated: the matrix cores take the other mask with Cin = 24 and Cout <= 24, or Cin = 64
    and Cout <= 64 (KP = 24 up to 24 gradient channels, else 64)"""
    if c.first_mask or c.Cout > 64:
        return 'valu'
    if c.Cin == 24 and c.Cout <= 24:
        return 'mfma24_c24'
    if c.Cin == 64:
        return 'mfma24_c64' if c.Cout <= 24 else 'mfma64_c64'
    return 'valu'
