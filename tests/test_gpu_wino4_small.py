"""-m gpu: the F(4x4) 3x3 kernel (csrc/conv3x3_wino4.hip) on maps of a few tile rows, every instantiation family -- 1 x 16 and 2 x 8
segments, the 8-wave form, 0 / 1 / 2 residuals, ReLU on / off, the STATS epilogue, the h2 / h12 phase forms.  Each case asserts
  (a) the output is byte-identical to the output recorded from the library before the kernel's vector-instruction diet
      (tests/golden/wino4_small.npz, written by tools/make_wino4_small_golden.py): the diet removes instructions, not operations, and
  (b) the output agrees with the float64 convolution within the single-layer bound tests/test_gpu_ops.py uses for the form
      (W4_RTOL for 128 -> 128, W5_RTOL for the phase forms).
The maps and what each exercises: tests/wino4_small_cases.py."""
import numpy as np
import pytest
import torch

from tests import wino4_small_cases as C
from tests.test_gpu_ops import W4_RTOL, W5_RTOL
from tests.util import assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    z = np.load(C.GOLDEN)
    rec = dict(zip([str(i) for i in z['ids']], [str(s) for s in z['sha256']]))
    raws = {k[4:]: z[k] for k in z.files if k.startswith('raw:')}
    assert sorted(raws) == sorted(C.RAW_KEPT)
    return rec, raws


@pytest.fixture(scope='module')
def device(cuda):
    from imgcomp_cvpr_amd import _lib
    return C.Device(_lib, cuda)


def _same_bits(y, cid, golden):
    rec, raws = golden
    if cid in raws:
        ref = torch.as_tensor(raws[cid])
        got = y.cpu()
        assert got.shape == ref.shape
        diff = got.view(torch.int32) != ref.view(torch.int32)
        assert not bool(diff.any()), '{}: {} of {} values differ from the record, first at {}'.format(
            cid, int(diff.sum()), diff.numel(), diff.nonzero()[0].tolist())
    assert C.sha(y) == rec[cid], '{}: output is not byte-identical to the recorded one'.format(cid)


@pytest.mark.parametrize('m,n_res,relu', C.C128_CASES, ids=[C.c128_id(*c) for c in C.C128_CASES])
def test_wino4_small_c128(device, golden, m, n_res, relu):
    y = device.c128(m, n_res, relu)
    cid = C.c128_id(m, n_res, relu)
    _same_bits(y, cid, golden)
    assert_close(y, C.c128_ref64(m, n_res, relu), 'winograd F(4x4) small ' + cid, W4_RTOL)


def test_wino4_small_stats_epilogue(device, golden):
    """the training forward: raw output + per-segment channel sums (2 x 32 x 32, 2 x 8-tile segments)"""
    raw, cst = device.stats()
    _same_bits(raw, 'stats/raw', golden)
    _same_bits(cst, 'stats/sums', golden)
    ref = C.c128_raw64(C.STATS_MAP)
    assert_close(raw, ref, 'winograd F(4x4) small stats/raw', W4_RTOL)
    # the sums are those of the values stored: float32 partial sums against their float64 sum, the bound of tests/test_gpu_training.py
    tot = cst.double().sum(dim=1).cpu()
    assert_close(tot[:, 0], raw.double().sum(dim=(0, 2, 3)).cpu(), 'winograd F(4x4) small stats: channel sums', 1e-6)
    assert_close(tot[:, 1], (raw.double() ** 2).sum(dim=(0, 2, 3)).cpu(), 'winograd F(4x4) small stats: channel sums of squares', 1e-6)


@pytest.mark.parametrize('tr,relu', C.PHASE_CASES, ids=[C.phase_id(*c) for c in C.PHASE_CASES])
def test_wino4_small_phase_forms(device, golden, tr, relu):
    """h2 (CIN 256) and h12 (COUT 256, SHUF) at an 8 x 64 quarter-resolution map"""
    y = device.phase(tr, relu)
    _same_bits(y, C.phase_id(tr, relu), golden)
    assert_close(y, C.phase_ref64(tr, relu), 'winograd F(4x4) small ' + C.phase_id(tr, relu), W5_RTOL)
