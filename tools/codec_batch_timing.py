"""The batch codec against the loop over the single-image codec, for 1, 2, 4 and 8 Kodak-shaped (512 x 768) synthetic natural images
at tiles of 128 pixels (24 tiles per image), all in ONE process and run:
  (a) the loop of Codec.compress / Codec.decompress, image after image -- what a caller had to write before the batch calls,
  (b) Codec.compress_many / Codec.decompress_many,
and the decoders alone: the loop of decode_tiles (one launch of 24 work-groups per image, the symbols to the host) against one
decode_tiles_batch (one launch of 24 N work-groups, q staying on the device).  The two sides are alternated inside every repeat, each
call ended by a device synchronise, host clock; every batch figure is to be read against the loop figure OF THE SAME RUN.
Prints one JSON line; --out writes it.

    python tools/codec_batch_timing.py [--repeats 5] [--counts 1,2,4,8] [--tile 128] [--out profiles/codec_batch_timing.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--counts', default='1,2,4,8')
    p.add_argument('--tile', type=int, default=128)
    p.add_argument('--out')
    flags = p.parse_args()
    counts = [int(v) for v in flags.counts.split(',')]
    from imgcomp_cvpr_amd import codec, config_parser as cp, weights as W
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda:0')
    ae_cfg, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc_cfg, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    wts = W.synthetic_weights(ae_cfg, pc_cfg)
    c = codec.Codec(ae_cfg, pc_cfg, wts, dev)
    e = flags.tile // c.factor
    c.tile = (e, e)
    imgs = [np.ascontiguousarray(W.synthetic_image((1, 3, 512, 768), 'natural', seed=4 + i)[0].transpose(1, 2, 0)) for i in range(max(counts))]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    files = [c.compress(img) for img in imgs]                # warm-up of the single-image path, and the references
    want = [c.decompress(f) for f in files]
    heads = [codec.parse_container(f) for f in files]
    vols = [(h.streams, h.first_syms, (h.C, h.h, h.w)) for h in heads]
    sides = {'compress_loop': lambda n: [c.compress(img) for img in imgs[:n]],
             'compress_many': lambda n: c.compress_many(imgs[:n]),
             'decompress_loop': lambda n: [c.decompress(f) for f in files[:n]],
             'decompress_many': lambda n: c.decompress_many(files[:n]),
             'decode_tiles_loop': lambda n: [c.pred.decode_tiles(s, f, shape, e, e) for s, f, shape in vols[:n]],
             'decode_tiles_batch': lambda n: c.pred.decode_tiles_batch(vols[:n], e, e, want='q')}
    for n in counts:                                         # warm-up of the batch path at every size (allocator, lanes), and its results
        assert c.compress_many(imgs[:n]) == files[:n], n
        assert all(np.array_equal(a, b) for a, b in zip(c.decompress_many(files[:n]), want[:n])), n
        sides['decode_tiles_batch'](n)
    t = {n: {k: [] for k in sides} for n in counts}
    for _ in range(flags.repeats):
        for n in counts:
            for k, fn in sides.items():
                t[n][k].append(timed(lambda: fn(n))[0])
    ms = lambda v: [round(1e3 * x, 3) for x in v]
    med = lambda v: round(1e3 * float(np.median(v)), 3)
    res = {'image': '512x768 synthetic natural, seeds 4..', 'tile_pixels': flags.tile, 'tiles_per_image': len(heads[0].streams),
           'repeats': flags.repeats, 'in_flight': c.IN_FLIGHT, 'device': torch.cuda.get_device_name(0),
           'weights': 'synthetic', 'counts': []}
    for n in counts:
        row = {'images': n, 'tiles': n * len(heads[0].streams)}
        for k in sides:
            row[k + '_ms'] = ms(t[n][k])
            row[k + '_median_ms'] = med(t[n][k])
        for what, a, b in (('compress', 'compress_many', 'compress_loop'), ('decompress', 'decompress_many', 'decompress_loop'),
                           ('decode_tiles', 'decode_tiles_batch', 'decode_tiles_loop')):
            row[what + '_batch_over_loop_same_run'] = round(med(t[n][a]) / med(t[n][b]), 5)
        row['decode_tiles_batch_over_one_image_same_run'] = round(med(t[n]['decode_tiles_batch']) / med(t[counts[0]]['decode_tiles_batch']), 5)
        res['counts'].append(row)
    line = json.dumps(res)
    print(line)
    if flags.out:
        with open(flags.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
