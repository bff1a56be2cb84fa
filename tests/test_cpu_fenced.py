"""Self-test of tests/fenced.py on CPU tensors: plain torch writes stand in for a kernel and plant each class of error the GPU
tests (tests/test_gpu_fenced_buffers.py) are to catch; then the coverage manifest against _lib.PROTOTYPES."""
import os
import re

import numpy as np
import pytest
import torch

from tests import fenced as F
from tests.fenced import FENCE, IN_FENCE, OUT_FENCE, check_fences, fenced, poison


def _raw_as(view, dtype):
    return F.allocation(view).view(dtype)


def test_view_is_dense_aligned_and_of_the_asked_shape_and_dtype():
    assert FENCE == 65536 and FENCE % 256 == 0
    for shape, dtype in (((2, 3, 5, 7), torch.float32), ((11,), torch.float64), ((3, 1), torch.int64), ((13,), torch.uint8)):
        v = fenced(shape, dtype, 'cpu', OUT_FENCE)
        raw = F.allocation(v)
        assert tuple(v.shape) == shape and v.dtype == dtype and v.is_contiguous()
        assert (v.data_ptr() - raw.data_ptr()) == FENCE and (v.data_ptr() - raw.data_ptr()) % 256 == 0
        assert raw.numel() == 2 * FENCE + v.numel() * v.element_size()
        assert bool((raw[:FENCE] == OUT_FENCE).all()) and bool((raw[FENCE + v.numel() * v.element_size():] == OUT_FENCE).all())
        if dtype.is_floating_point:
            assert bool(torch.isnan(v).all())                     # an output: every element must be written
    a = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    v = fenced(a, torch.float32, 'cpu', IN_FENCE)
    assert v.dtype == torch.float32 and tuple(v.shape) == (2, 3, 4) and torch.equal(v, torch.as_tensor(a).float())
    # the fences of a float input read as NaN in float32 and in float64
    assert bool(torch.isnan(_raw_as(v, torch.float32)[:FENCE // 4]).all())
    assert bool(torch.isnan(_raw_as(fenced((2,), torch.float64, 'cpu', IN_FENCE), torch.float64)[:FENCE // 8]).all())


def test_untouched_call_passes():
    x, y = fenced(np.ones((3, 5), np.float32), torch.float32, 'cpu', IN_FENCE, 'x'), fenced((3, 5), torch.float32, 'cpu', OUT_FENCE, 'y')
    y.copy_(x * 2)                                                # a correct kernel: writes every element, nothing else
    check_fences(x, y, None)
    assert not bool(torch.isnan(y).any())


def test_store_one_element_before_the_view_is_reported():
    y = fenced((4, 4), torch.float32, 'cpu', OUT_FENCE, 'the output')
    _raw_as(y, torch.float32)[FENCE // 4 - 1] = 1.0
    with pytest.raises(AssertionError) as e:
        check_fences(y)
    msg = str(e.value)
    assert 'the output' in msg and 'front fence' in msg and 'first at byte -4' in msg and 'last at byte -1' in msg and re.search(r'\b[34] bytes changed', msg)


def test_store_one_element_behind_the_view_is_reported():
    y = fenced((4, 4), torch.float32, 'cpu', OUT_FENCE, 'the output')
    _raw_as(y, torch.float32)[FENCE // 4 + 16] = 1.0
    with pytest.raises(AssertionError) as e:
        check_fences(y)
    msg = str(e.value)
    assert 'the output' in msg and 'back fence' in msg and 'first at byte +64' in msg and 'last at byte +67' in msg


def test_store_at_the_last_fence_byte_is_reported():
    y = fenced((5,), torch.uint8, 'cpu', OUT_FENCE, 'ws')
    F.allocation(y)[-1] = 0
    with pytest.raises(AssertionError) as e:
        check_fences(y)
    assert 'back fence: 1 bytes changed, first at byte +{0}, last at byte +{0}'.format(5 + FENCE - 1) in str(e.value)
    y = fenced((5,), torch.uint8, 'cpu', OUT_FENCE, 'ws')
    F.allocation(y)[0] = 0                                        # and the first byte of the front fence
    with pytest.raises(AssertionError) as e:
        check_fences(y)
    assert 'front fence: 1 bytes changed, first at byte -{0}, last at byte -{0}'.format(FENCE) in str(e.value)


def test_a_read_of_one_fence_element_poisons_the_result():
    x = fenced(np.ones((8,), np.float32), torch.float32, 'cpu', IN_FENCE, 'x')
    raw = _raw_as(x, torch.float32)
    good = raw[FENCE // 4:FENCE // 4 + 8].sum()
    assert bool(torch.isfinite(good))
    for lo in (FENCE // 4 - 1, FENCE // 4 + 1):                   # a window one element early, one element late
        assert not bool(torch.isfinite(raw[lo:lo + 8].sum()))
    # "multiplied by a zero mask" does not hide it either: NaN * 0 is NaN
    assert not bool(torch.isfinite(raw[FENCE // 4 - 1] * 0.0))


def test_poison_and_bit_comparison():
    ws = fenced((64,), torch.uint8, 'cpu', OUT_FENCE, 'ws')
    poison(ws, 0xFF)
    assert bool((ws == 0xFF).all()) and bool(torch.isnan(ws.view(torch.float32)).all())
    poison(ws[:16], 0x00)
    assert bool((ws[:16] == 0).all()) and bool((ws[16:] == 0xFF).all())
    check_fences(ws)
    a = torch.tensor([1.0, float('nan')])
    assert not torch.equal(a, a.clone()) and F.same_bits(a, a.clone())
    assert not F.same_bits(a, torch.tensor([1.0, 2.0]))
    d = torch.tensor([float('nan')], dtype=torch.float64)
    assert F.same_bits(d, d.clone())
    # a refused call must leave views and fences as they were
    y = fenced((4,), torch.float32, 'cpu', OUT_FENCE, 'y')
    snap = F.snapshot(y, None)
    F.unchanged(snap, y, None)
    y[2] = 1.0
    with pytest.raises(AssertionError):
        F.unchanged(snap, y)
    # the second fill of an integer input
    s = fenced(np.arange(5), torch.int64, 'cpu', F.ZERO_FENCE, 'symbols')
    check_fences(s)
    F.refence(s, IN_FENCE)
    check_fences(s)
    assert bool((F.allocation(s)[:FENCE] == 0xFF).all()) and torch.equal(s, torch.arange(5))


# ---- the coverage manifest -------------------------------------------------------------------------------------------------------

def test_manifest_covers_the_prototypes_exactly():
    from imgcomp_cvpr_amd import _lib
    names = set(_lib.PROTOTYPES)
    assert set(F.COVERAGE) == names, 'undecided: {}; gone: {}'.format(sorted(names - set(F.COVERAGE)), sorted(set(F.COVERAGE) - names))


def test_every_fenced_name_is_called_by_the_gpu_test():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_gpu_fenced_buffers.py')).read()
    missing = [n for n, v in F.COVERAGE.items() if v == F.FENCED and 'lib.{}('.format(n) not in src]
    assert not missing, missing


def test_only_the_four_reasons_are_used():
    for name, v in F.COVERAGE.items():
        if v == F.FENCED:
            continue
        assert v.startswith(F.ALLOWED_REASON_PREFIXES), (name, v)
        if v.startswith('codec entry'):
            assert name.startswith(('ic_pc_encode', 'ic_pc_decode', 'ic_pc_conceal')), name
            f = v.split('tests/')[1]
            path = os.path.join(os.path.dirname(os.path.abspath(__file__)), f)
            assert re.match(r'test_gpu_codec\w*\.py$', f) and os.path.isfile(path) and re.search(name + r'\b', open(path).read()), (name, f)
        if v == F.PEER:
            assert name.startswith('ic_peer_'), name
