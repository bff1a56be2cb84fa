"""-m gpu: ic_pc_bwd_data_f32, the data gradient of the context model's masked conv3d, on every kernel it chooses among, against
float64 autograd on the cases of tests/pc_bwd_cases.py (the table, the inputs and the references; tests/test_cpu_pc_bwd_cases.py
checks them).  Through the C ABI, all device buffers from tests/fenced.py.

Every case: dx into a NaN-filled tensor; two launches with identical bits (the matrix-core cases over a workspace of exactly the
queried size, filled with 0xFF and then with 0x00); no NaN left; exactly 0 wherever act <= 0 (cases with the ReLU mask); the
reference within 1e-5 of the tensor scale.  Every matrix-core case runs once more without a workspace -- the any-shape kernel on
the same shape -- which must hold the same bound with OTHER bits: the two kernels sum in different orders (the VALU kernel tap by
tap over all gradient channels, the matrix cores 8-channel group by group in four partial sums), so equal bits would mean that
the workspace did not select the matrix cores.

| path       | kernel                                                   | what its cases reach                                        |
| mfma24_c24 | pc_mfma_kernel<24,24,1,4,8,16,false,true>, gridDim.y = 1 | 8 x 16 tiles: one, 2 x 2 by a row and a column, all halo,   |
| mfma24_c64 | the same, gridDim.y = 2 (64 rows = two 32-row tiles)     | N = 3; 2 / 12 / 16 / 60 work-groups (ic_xcd_run's tail);    |
|            |                                                          | Cout 3, 6, 16 (zero-padded gradient channels, the packer's  |
|            |                                                          | kq < Cout guard) and 24                                     |
| mfma64_c64 | pc_mfma_kernel<64,16,2,2,4,16,false,true>                | 4 x 16 tiles in the same four forms; 2 / 16 / 18 / 24       |
|            |                                                          | work-groups; Cout 25, 40, 64                                |
| valu       | pc_bwd_data_kernel<8>                                    | Cin 1, 5, 12, 20 (clamped filter offsets, the ci >= Cin     |
|            |                                                          | break) and 8; the first mask; under one block of 256        |
|            |                                                          | positions and a ragged second one; Cin = 24 with Cout 40    |
All matrix-core paths: pc_bwd_fix_kernel with residual and mask, either alone and neither (then it is not launched).

What no value here can show: the packer's `kq < CoutF` guard and the `min(ci0 + j, Cin - 1)` clamp of the any-shape kernel only keep
LOADS inside the filter array.  What the packer would load without its guard meets a zero-padded gradient channel, and what the
any-shape kernel would load without its clamp feeds an accumulator that the `ci >= Cin` break never stores.  (A clamp that is too
LOW, or a missing break, does show: the last channel gets another channel's filter row, resp. dx is written past its Cin
channels, into the next image or the fence.)"""
import pytest
import torch

from tests import pc_bwd_cases as B
from tests.fenced import OUT_FENCE, poison, same_bits
from tests.test_gpu_fenced_buffers import Bufs, _Poisoned, _refill, _written
from tests.util import assert_close

pytestmark = pytest.mark.gpu


def _L():
    from imgcomp_cvpr_amd import _lib
    return _lib


class _Run(object):
    """the fenced device buffers of one case and its launches"""

    def __init__(self, cuda, case):
        self.L, self.bufs, self.case = _L(), Bufs(cuda), case
        g, w, act, res = B.inputs(case)
        fin = self.bufs.fin
        self.g, self.w = fin(g.copy(), 'g'), fin(w.copy(), 'filter')              # (the shared arrays are read-only)
        self.act = fin(act.copy(), 'act') if case.relu_mask else None
        self.res = fin(res.copy(), 'res') if case.res else None
        self.dx = self.bufs.out(B.dx_shape(case), 'dx')
        self.dead = torch.tensor(act <= 0, device=cuda) if case.relu_mask else None
        self.ref = B.reference(case)

    def launch(self, ws=None, nbytes=0):
        L, c = self.L, self.case
        return L.lib.ic_pc_bwd_data_f32(L.ptr(self.g), L.ptr(self.w), L.ptr(self.res), L.ptr(self.act), L.ptr(self.dx), c.N, c.Cin, c.Cout,
                                        c.OD, c.OH, c.OW, c.first_mask, int(c.relu_mask), L.ptr(ws), nbytes, L.current_stream())

    def check(self, kernel):
        """the values of dx -> a clone of it"""
        what = 'pc data gradient {} {}'.format(self.case.path, kernel)
        _written(self.dx, what + ' ' + B.case_id(self.case))
        if self.dead is not None:
            assert not bool(self.dx[self.dead].any()), what + ': a gradient behind a clamped activation'
        assert_close(self.dx, self.ref, what + ' shape ' + B.case_id(self.case), B.RTOL)
        return self.dx.clone()

    def valu_twice(self, ws=None, nbytes=0):
        """two launches of the any-shape kernel into a NaN-filled dx: identical bits -> the values"""
        got = []
        for _ in range(2):
            _refill(self.dx)
            self.bufs.done(self.launch(ws, nbytes), B.case_id(self.case))
            got.append(self.dx.clone())
        assert same_bits(got[0], got[1]), 'a second launch gives other bits'
        return self.check('VALU')


@pytest.mark.parametrize('case', [c for c in B.CASES if c.path in B.MFMA_PATHS], ids=B.case_id)
def test_matrix_core_paths(cuda, case):
    r = _Run(cuda, case)
    need = B.query(r.L.lib, case)
    assert need > 0 and B.expected_path(case) == case.path
    ws = r.bufs.ws(need)
    run = _Poisoned(r.bufs, ws, [r.dx], lambda: r.launch(ws, need), B.case_id(case))
    mfma = r.check('matrix cores')
    run.again()
    valu = r.valu_twice()
    assert not torch.equal(mfma, valu), 'the workspace did not select another kernel'


@pytest.mark.parametrize('case', [c for c in B.CASES if c.path == 'valu'], ids=B.case_id)
def test_any_shape_kernel(cuda, case):
    """no matrix-core path: the query answers 0 (asserted BEFORE anything is launched), and a buffer passed all the same is not
    touched and changes nothing -- (Cin, Cout) = (24, 40) among these, a shape the KP = 64 kernel must not get"""
    r = _Run(cuda, case)
    assert B.query(r.L.lib, case) == 0 and B.expected_path(case) == 'valu'
    plain = r.valu_twice()
    ws = poison(r.bufs.ws(4096), OUT_FENCE)
    with_buffer = r.valu_twice(ws, 4096)
    assert same_bits(plain, with_buffer)
    assert bool((ws == OUT_FENCE).all()), 'the any-shape kernel has no workspace, yet the buffer passed was written'


def test_first_mask_never_takes_the_matrix_cores(cuda):
    """a k -> k shape whose query is non-zero, with first_mask = 1 and the workspace passed: the any-shape kernel under the first
    mask (the matrix-core kernels have the other mask's 14 taps), the workspace untouched"""
    shape = next(c for c in B.CASES if c.path == 'mfma24_c24' and c.res and c.relu_mask and c.OH == 7)
    case = shape._replace(path='valu', first_mask=1)
    r = _Run(cuda, case)
    need = B.query(r.L.lib, case)
    assert need > 0
    plain = r.valu_twice()
    ws = poison(r.bufs.ws(need), OUT_FENCE)
    assert same_bits(plain, r.valu_twice(ws, need))
    assert bool((ws == OUT_FENCE).all())
    other = B.reference(shape)
    assert float((other - r.ref).abs().max()) >= 100 * B.RTOL * max(1.0, float(r.ref.abs().max()))       # the masks differ here
