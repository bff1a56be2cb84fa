"""Wavefront tiles (format 5) against checked tiles (format 4) on the 512 x 768 synthetic natural image of codec_tiled_timing.py, at
--tile 128 and --tile 64, in ONE run: compress and decompress of one file (image <-> container bytes, end to end), the decoder
launches alone (decode_tiles_batch of that file's streams, raster order against wavefront order, q staying on the device), 8 files
through decompress_many, and the payload bytes of both.  The two formats are alternated inside every repeat, each call ended by a
device synchronise, host clock; medians and the spread (min .. max) of the repeats.  A format-5 figure is to be read against the
format-4 figure OF THE SAME RUN.  Prints one JSON line; --out writes it.

    python tools/codec_wavefront_timing.py [--repeats 5] [--out profiles/codec_wavefront_timing.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

TILES = (128, 64)
FORMATS = (('format4', 'raster', True), ('format5', 'wavefront', False))
MANY = 8


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--out')
    flags = p.parse_args()
    from imgcomp_cvpr_amd import codec, config_parser as cp, weights as W
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda:0')
    ae_cfg, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc_cfg, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    c = codec.Codec(ae_cfg, pc_cfg, W.synthetic_weights(ae_cfg, pc_cfg), dev)
    imgs = [np.ascontiguousarray(W.synthetic_image((1, 3, 512, 768), 'natural', seed=4 + i)[0].transpose(1, 2, 0)) for i in range(MANY)]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def setup(tile, order, checked):
        c.tile, c.order, c.checked = (tile // c.factor, tile // c.factor), order, checked

    def launch(head, order):
        return c.pred.decode_tiles_batch([(head.streams, head.first_syms, (head.C, head.h, head.w))], head.th, head.tw, want='q', order=order)

    files, heads, t = {}, {}, {}
    for tile in TILES:                                     # warm-up of every path, the files, and that both formats hold one image
        for name, order, checked in FORMATS:
            setup(tile, order, checked)
            files[tile, name] = c.compress_many(imgs)
            assert files[tile, name][0] == c.compress(imgs[0])
            heads[tile, name] = codec.parse_container(files[tile, name][0])
            launch(heads[tile, name], order)
            c.decompress_many(files[tile, name])
            t[tile, name] = {'compress': [], 'decompress': [], 'decode_launch': [], 'decompress_many': []}
        assert np.array_equal(c.decompress(files[tile, 'format4'][0]), c.decompress(files[tile, 'format5'][0]))
        assert torch.equal(launch(heads[tile, 'format4'], 'raster')[0], launch(heads[tile, 'format5'], 'wavefront')[0])
    for _ in range(flags.repeats):
        for tile in TILES:
            for name, order, checked in FORMATS:
                setup(tile, order, checked)
                t[tile, name]['compress'].append(timed(lambda: c.compress(imgs[0]))[0])
                t[tile, name]['decompress'].append(timed(lambda: c.decompress(files[tile, name][0]))[0])
                t[tile, name]['decode_launch'].append(timed(lambda: launch(heads[tile, name], order))[0])
                t[tile, name]['decompress_many'].append(timed(lambda: c.decompress_many(files[tile, name]))[0])
    ms = lambda v: [round(1e3 * x, 3) for x in v]
    med = lambda v: round(1e3 * float(np.median(v)), 3)
    res = {'image': '512x768 synthetic natural, seeds 4..{} ({} files through decompress_many)'.format(3 + MANY, MANY), 'repeats': flags.repeats,
           'weights': 'synthetic', 'device': torch.cuda.get_device_name(0), 'configs': []}
    for tile in TILES:
        row = {'tile_pixels': tile, 'tiles': len(heads[tile, 'format4'].streams)}
        for name, _, _ in FORMATS:
            r = {'payload_bytes': len(heads[tile, name].payload), 'file_bytes': len(files[tile, name][0])}
            for what, v in t[tile, name].items():
                r[what + '_ms'] = ms(v)
                r[what + '_median_ms'] = med(v)
                r[what + '_spread_ms'] = round(1e3 * (max(v) - min(v)), 3)
            row[name] = r
        a, b = row['format4'], row['format5']
        for what in ('decode_launch', 'decompress', 'decompress_many', 'compress'):
            row[what + '_format4_over_format5'] = round(a[what + '_median_ms'] / b[what + '_median_ms'], 3)
        row['payload_format5_minus_format4_bytes'] = b['payload_bytes'] - a['payload_bytes']
        # the claim: the format-5 decoder launch is faster than the raster launch of this run by more than the recorded spread
        row['decode_launch_faster_by_more_than_spread'] = bool(
            a['decode_launch_median_ms'] - b['decode_launch_median_ms'] > max(a['decode_launch_spread_ms'], b['decode_launch_spread_ms']))
        res['configs'].append(row)
    line = json.dumps(res)
    print(line)
    if flags.out:
        with open(flags.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
