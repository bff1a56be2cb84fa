#!/usr/bin/env python
"""Record the outputs of the F(4x4) 3x3 kernel on the small maps of tests/wino4_small_cases.py into tests/golden/wino4_small.npz:
the SHA-256 of every case's float32 output and the raw output of the two smallest cases.  Run it on an MI355X with a library that is
known to be good (the record in the tree was made from the library BEFORE the kernel's vector-instruction diet);
tests/test_gpu_wino4_small.py then holds every later build to these bits.

  python tools/make_wino4_small_golden.py [--out tests/golden/wino4_small.npz]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from imgcomp_cvpr_amd import _lib as L  # noqa: E402
from tests import wino4_small_cases as C  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=C.GOLDEN)
    a = p.parse_args()
    cuda = torch.device('cuda:0')
    dev = C.Device(L, cuda)
    ids, shas, raws = [], [], {}
    for m, n_res, relu in C.C128_CASES:
        cid = C.c128_id(m, n_res, relu)
        y = dev.c128(m, n_res, relu)
        assert bool(torch.isfinite(y).all()), cid
        ids.append(cid)
        shas.append(C.sha(y))
        if cid in C.RAW_KEPT:
            raws['raw:' + cid] = y.cpu().numpy()
    raw, cst = dev.stats()
    assert bool(torch.isfinite(raw).all()) and bool(torch.isfinite(cst).all())
    ids += ['stats/raw', 'stats/sums']
    shas += [C.sha(raw), C.sha(cst)]
    for tr, relu in C.PHASE_CASES:
        y = dev.phase(tr, relu)
        assert bool(torch.isfinite(y).all()), (tr, relu)
        ids.append(C.phase_id(tr, relu))
        shas.append(C.sha(y))
    assert sorted(k[4:] for k in raws) == sorted(C.RAW_KEPT)
    np.savez_compressed(a.out, ids=np.array(ids), sha256=np.array(shas), **raws)
    for i, s in zip(ids, shas):
        print(s, i)
    print('wrote', a.out, os.path.getsize(a.out), 'bytes')


if __name__ == '__main__':
    main()
