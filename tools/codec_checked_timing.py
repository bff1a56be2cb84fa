"""What the checked container (format 4) and salvage cost against format 2, on one Kodak-shaped (512 x 768) synthetic natural image at
tiles of 128 pixels (24 tiles), all in ONE process and run:
  decompress of the format-2 file (the reference side: that path does not know about format 4),
  decompress of the format-4 file (strict reader: the header CRC and 24 stream CRCs more on the host),
  salvage of the intact format-4 file, and of the file with 1 and with 6 of its 24 tiles damaged (one flipped byte each).
The sides are alternated inside every repeat, each call ended by a device synchronise, host clock, medians; every figure is to be
read against the format-2 figure OF THE SAME RUN.  --conceal-only runs nothing but a few salvage calls of the damaged files: the
program for a kernel trace of its own (pc_conceal_tiles_kernel).  Prints one JSON line; --out writes it.

    python tools/codec_checked_timing.py [--repeats 5] [--tile 128] [--out profiles/codec_checked_timing.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def flipped(codec, data, tiles):
    """one byte in the middle of each named tile's stream flipped"""
    c = codec.parse_container(data)
    start = len(data) - 4 - len(c.payload)
    offs = np.concatenate([[0], np.cumsum([len(b) for b in c.streams])]).astype(np.int64)
    bad = bytearray(data)
    for t in tiles:
        bad[start + int(offs[t]) + len(c.streams[t]) // 2] ^= 0x20
    return bytes(bad)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--tile', type=int, default=128)
    p.add_argument('--conceal-only', action='store_true')
    p.add_argument('--out')
    flags = p.parse_args()
    from imgcomp_cvpr_amd import codec, config_parser as cp, weights as W
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda:0')
    ae_cfg, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc_cfg, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    wts = W.synthetic_weights(ae_cfg, pc_cfg)
    c = codec.Codec(ae_cfg, pc_cfg, wts, dev)
    e = flags.tile // c.factor
    c.tile = (e, e)
    img = np.ascontiguousarray(W.synthetic_image((1, 3, 512, 768), 'natural', seed=4)[0].transpose(1, 2, 0))
    v2 = c.compress(img)
    c.checked = True
    v4 = c.compress(img)
    ntiles = len(codec.parse_container(v4).streams)
    assert len(v4) == len(v2) + 4 * ntiles + 4
    one, six = flipped(codec, v4, [9]), flipped(codec, v4, [0, 3, 9, 10, 16, 23])
    if flags.conceal_only:
        for _ in range(3):
            assert len(c.salvage(one)[1].damaged) == 1 and len(c.salvage(six)[1].damaged) == 6
        torch.cuda.synchronize()
        return

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    sides = {'decompress_v2': lambda: c.decompress(v2), 'decompress_v4': lambda: c.decompress(v4), 'salvage_intact': lambda: c.salvage(v4)[0],
             'salvage_1_damaged': lambda: c.salvage(one)[0], 'salvage_6_damaged': lambda: c.salvage(six)[0]}
    want = c.decompress(v2)
    for _ in range(2):                                       # warm-up of every side, and what each must give
        assert np.array_equal(c.decompress(v4), want) and np.array_equal(c.salvage(v4)[0], want)
        assert c.salvage(one)[0].shape == want.shape and c.salvage(six)[0].shape == want.shape
    t = {k: [] for k in sides}
    for _ in range(flags.repeats):
        for k, fn in sides.items():
            t[k].append(timed(fn)[0])
    med = lambda v: round(1e3 * float(np.median(v)), 3)
    res = {'image': '512x768 synthetic natural, seed 4', 'tile_pixels': flags.tile, 'tiles': ntiles, 'repeats': flags.repeats,
           'device': torch.cuda.get_device_name(0), 'weights': 'synthetic', 'bytes_v2': len(v2), 'bytes_v4': len(v4)}
    for k in sides:
        res[k + '_ms'] = [round(1e3 * x, 3) for x in t[k]]
        res[k + '_median_ms'] = med(t[k])
        res[k + '_over_decompress_v2_same_run'] = round(med(t[k]) / med(t['decompress_v2']), 5)
    line = json.dumps(res)
    print(line)
    if flags.out:
        with open(flags.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
