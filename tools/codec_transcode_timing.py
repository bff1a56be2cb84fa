"""Transcoding, on the 512 x 768 synthetic natural image of the other codec timings with --tile 128, synthetic weights, in ONE run:
  1. transcode A -> B                     Codec.transcode for 2 -> 8, 4 -> 6 and 1 -> 2, and beside it its two halves timed on their
                                          own: the decoder call that leaves the symbols on the device, and the coding call
                                          (Codec._container) on symbols that are already there.
  2. decompress + compress                decompress(data) then compress(pixels) into the target's format, the same file in the same
                                          repeat: the only way to change a file's format without transcode.  It runs the autoencoder
                                          twice, so its bytes are NOT the transcoded file's (`same_bytes` says whether they happen to be).
  3. transcode_many                       8 files (formats 2 and 4 alternating) to format 8 in one call against the loop over transcode.
The calls of a group are alternated inside every repeat after a warm-up round, each ended by a device synchronise, host clock; medians
and the spread (max - min) of the repeats.  Every figure is to be read against its partner OF THE SAME RUN; nothing is asserted about
times, the bytes are: every transcoded file equals compress(img) of the target.  Prints one JSON line; --out writes it.

    python tools/codec_transcode_timing.py [--repeats 7] [--out profiles/codec_transcode_timing.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

TILE = 128
FILES = 8


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--repeats', type=int, default=7)
    p.add_argument('--out')
    flags = p.parse_args()
    from imgcomp_cvpr_amd import codec, config_parser as cp, weights as W
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda:0')
    ae_cfg, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc_cfg, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    c = codec.Codec(ae_cfg, pc_cfg, W.synthetic_weights(ae_cfg, pc_cfg), dev)
    tile = (TILE // 8, TILE // 8)
    formats = {1: {}, 2: dict(tile=tile), 4: dict(tile=tile, checked=True), 6: dict(tile=tile, layers='default'),
               8: dict(tile=tile, front_layers='default')}

    def to(fmt):
        kw = formats[fmt]
        c.tile, c.checked, c.order, c.layers, c.front_layers = kw.get('tile'), kw.get('checked', False), 'raster', kw.get('layers'), kw.get('front_layers')
        return c

    images = [np.ascontiguousarray(W.synthetic_image((1, 3, 512, 768), 'natural', seed=4 + i)[0].transpose(1, 2, 0)) for i in range(FILES)]
    img = images[0]
    files = {fmt: to(fmt).compress(img) for fmt in formats}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def stats(v):
        return {'ms': [round(1e3 * x, 3) for x in v], 'median_ms': round(1e3 * float(np.median(v)), 3),
                'spread_ms': round(1e3 * (max(v) - min(v)), 3)}

    def alternate(calls, check=None):
        """calls: [(name, fn)] -> {name: stats}; one warm-up round (checked), then flags.repeats rounds, the calls in turn"""
        got = {name: fn() for name, fn in calls}
        if check:
            check(got)
        t = {name: [] for name, _ in calls}
        for _ in range(flags.repeats):
            for name, fn in calls:
                t[name].append(timed(fn)[0])
        return {name: stats(v) for name, v in t.items()}

    res = {'image': '512x768 synthetic natural, seed 4', 'tile': TILE, 'repeats': flags.repeats, 'weights': 'synthetic',
           'device': torch.cuda.get_device_name(0), 'file_bytes': {str(k): len(v) for k, v in files.items()}}

    # 1. and 2.: one file to another format
    for A, B in ((2, 8), (4, 6), (1, 2)):
        data, head = files[A], codec.parse_container(files[A])
        sym = c._decode_device(head)
        note = {}

        def check(got, B=B, note=note):
            assert got['transcode'] == files[B] and got['code'] == files[B] and torch.equal(got['decode'], sym)
            note['same_bytes'] = got['decompress_compress'] == files[B]
        pair = alternate([('transcode', lambda: to(B).transcode(data)),
                          ('decode', lambda: c._decode_device(head)),
                          ('code', lambda: to(B)._container(sym, head.H, head.W)),
                          ('decompress_compress', lambda: to(B).compress(c.decompress(data)))], check)
        pair['decompress_compress']['same_bytes_as_transcode'] = note['same_bytes']
        pair['transcode_over_decompress_compress'] = round(pair['transcode']['median_ms'] / pair['decompress_compress']['median_ms'], 4)
        res['{}_to_{}'.format(A, B)] = pair

    # 3. a list of files
    datas = [to(2 if i % 2 == 0 else 4).compress(im) for i, im in enumerate(images)]
    want = [to(8).compress(im) for im in images]

    def same(got):
        assert got['transcode_many'] == want and got['transcode_loop'] == want
    many = alternate([('transcode_many', lambda: to(8).transcode_many(datas)),
                      ('transcode_loop', lambda: [to(8).transcode(d) for d in datas])], same)
    many['files'] = FILES
    many['many_over_loop'] = round(many['transcode_many']['median_ms'] / many['transcode_loop']['median_ms'], 4)
    res['many_2_4_to_8'] = many
    line = json.dumps(res)
    print(line)
    if flags.out:
        with open(flags.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
