"""Layered tiles (format 6, --tile 128 --progressive: layer ends C/8, C/4, C/2, C) against checked tiles (format 4, --tile 128) on the
512 x 768 synthetic natural image of codec_tiled_timing.py, in ONE run:
  compress and decompress of both formats;
  decompress_partial of the format-6 file cut at every layer prefix (layer_prefix_bytes(g), g = 1 .. G);
  the payload of format 6 minus that of format 4, in total and per segment (the price of G coder terminations per tile).
All configurations are alternated inside every repeat, each call ended by a device synchronise, host clock; medians and the spread
(min .. max) of the repeats.  Every figure is to be read against the format-4 figure OF THE SAME RUN.  Nothing is asserted about
times or sizes; the pixels are (format 6 == format 4, every prefix == the --channels preview of the whole file).
Prints one JSON line; --out writes it.

    python tools/codec_layered_timing.py [--repeats 5] [--out profiles/codec_layered_timing.json]
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
    img = np.ascontiguousarray(W.synthetic_image((1, 3, 512, 768), 'natural', seed=4)[0].transpose(1, 2, 0))
    tile = (TILE // c.factor, TILE // c.factor)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def compress(version):
        c.tile, c.checked, c.order, c.layers = tile, version == 4, 'raster', 'default' if version == 6 else None
        try:
            return c.compress(img)
        finally:
            c.tile, c.checked, c.layers = None, False, None

    files = {v: compress(v) for v in (4, 6)}               # also the warm-up of both encoders
    heads = {v: codec.parse_container(files[v]) for v in (4, 6)}
    ends = heads[6].layer_ends
    cuts = [files[6][:codec.layer_prefix_bytes(files[6], g)] for g in range(1, len(ends) + 1)]
    whole = c.decompress(files[4])
    assert np.array_equal(c.decompress(files[6]), whole)
    for g, cut in enumerate(cuts):
        out, report = c.decompress_partial(cut)
        assert report.layers_decoded == g + 1 and np.array_equal(out, c.decompress(files[6], channels=ends[g]))
    t = {('compress', v): [] for v in (4, 6)}
    t.update({('decompress', v): [] for v in (4, 6)})
    t.update({('partial', g): [] for g in range(len(cuts))})
    for _ in range(flags.repeats):
        for v in (4, 6):
            t['compress', v].append(timed(lambda: compress(v))[0])
            t['decompress', v].append(timed(lambda: c.decompress(files[v]))[0])
        for g, cut in enumerate(cuts):
            t['partial', g].append(timed(lambda: c.decompress_partial(cut))[0])

    def stats(v):
        return {'ms': [round(1e3 * x, 3) for x in v], 'median_ms': round(1e3 * float(np.median(v)), 3),
                'spread_ms': round(1e3 * (max(v) - min(v)), 3)}

    nt, G = len(heads[6].first_syms), len(ends)
    pay4, pay6 = len(heads[4].payload), len(heads[6].payload)
    res = {'image': '512x768 synthetic natural, seed 4', 'tile': TILE, 'layer_ends': ends, 'tiles': nt, 'repeats': flags.repeats,
           'weights': 'synthetic', 'device': torch.cuda.get_device_name(0),
           'file_bytes': {'format4': len(files[4]), 'format6': len(files[6])},
           'payload_bytes': {'format4': pay4, 'format6': pay6, 'format6_minus_format4': pay6 - pay4,
                             'per_segment': round((pay6 - pay4) / float(nt * G), 3), 'relative': round((pay6 - pay4) / float(pay4), 5)},
           'prefix_bytes': [len(cut) for cut in cuts]}
    for what in ('compress', 'decompress'):
        res[what] = {'format4': stats(t[what, 4]), 'format6': stats(t[what, 6])}
        res[what]['format6_over_format4'] = round(res[what]['format6']['median_ms'] / res[what]['format4']['median_ms'], 4)
    res['decompress_partial'] = []
    for g, cut in enumerate(cuts):
        r = {'layers': g + 1, 'channels': ends[g], 'bytes': len(cut), 'share_of_file': round(len(cut) / float(len(files[6])), 4)}
        r.update(stats(t['partial', g]))
        r['over_format6_decompress'] = round(r['median_ms'] / res['decompress']['format6']['median_ms'], 4)
        res['decompress_partial'].append(r)
    line = json.dumps(res)
    print(line)
    if flags.out:
        with open(flags.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
