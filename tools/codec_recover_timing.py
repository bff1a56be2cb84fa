"""Recovery of layered files (format 6, --tile 128 --progressive) against the two readers it stands beside, on the 512 x 768 synthetic
natural image of codec_layered_timing.py, in ONE run:
  recover of the intact file                       against decompress of it (the same pixels);
  recover of the file cut in the middle of layer 2 against decompress_partial of the same bytes (which shows layers 0 and 1 of every
                                                   tile; recover adds layer 2 of the tiles in front of the cut and conceals it in the rest).
The four calls are alternated inside every repeat after one warm-up round, each call ended by a device synchronise, host clock;
medians and the spread (min .. max) of the repeats.  Every figure is to be read against its partner OF THE SAME RUN.  Nothing is
asserted about times; the pixels of the intact file are.
Prints one JSON line; --out writes it.

    python tools/codec_recover_timing.py [--repeats 7] [--out profiles/codec_recover_timing.json]
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
    p.add_argument('--repeats', type=int, default=7)
    p.add_argument('--out')
    flags = p.parse_args()
    from imgcomp_cvpr_amd import codec, config_parser as cp, weights as W
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda:0')
    ae_cfg, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc_cfg, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    c = codec.Codec(ae_cfg, pc_cfg, W.synthetic_weights(ae_cfg, pc_cfg), dev)
    img = np.ascontiguousarray(W.synthetic_image((1, 3, 512, 768), 'natural', seed=4)[0].transpose(1, 2, 0))
    c.tile, c.layers = (TILE // c.factor, TILE // c.factor), 'default'
    try:
        data = c.compress(img)
    finally:
        c.tile, c.layers = None, None
    head = codec.parse_container(data)
    a, b = codec.layer_prefix_bytes(data, 2), codec.layer_prefix_bytes(data, 3)
    cut = data[:(a + b) // 2]                              # the middle of layer 2

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    calls = [('decompress', lambda: c.decompress(data)), ('recover_intact', lambda: c.recover(data)[0]),
             ('decompress_partial_cut', lambda: c.decompress_partial(cut)[0]), ('recover_cut', lambda: c.recover(cut)[0])]
    warm = {name: fn() for name, fn in calls}              # warm-up: workspaces, kernels, the autoencoder's plan
    assert np.array_equal(warm['recover_intact'], warm['decompress'])
    _, report = c.recover(cut)
    held = sorted(set(d.layers for d in report.tiles))
    assert held == [2, 3] and c.decompress_partial(cut)[1].layers_decoded == 2
    t = {name: [] for name, _ in calls}
    for _ in range(flags.repeats):
        for name, fn in calls:
            t[name].append(timed(fn)[0])

    def stats(v):
        return {'ms': [round(1e3 * x, 3) for x in v], 'median_ms': round(1e3 * float(np.median(v)), 3),
                'spread_ms': round(1e3 * (max(v) - min(v)), 3)}

    res = {'image': '512x768 synthetic natural, seed 4', 'tile': TILE, 'layer_ends': head.layer_ends, 'tiles': len(head.first_syms),
           'repeats': flags.repeats, 'weights': 'synthetic', 'device': torch.cuda.get_device_name(0),
           'file_bytes': len(data), 'cut_bytes': len(cut), 'cut_tiles_with_layer_2': sum(d.layers == 3 for d in report.tiles)}
    res.update({name: stats(v) for name, v in t.items()})
    res['recover_intact_over_decompress'] = round(res['recover_intact']['median_ms'] / res['decompress']['median_ms'], 4)
    res['recover_cut_over_decompress_partial'] = round(res['recover_cut']['median_ms'] / res['decompress_partial_cut']['median_ms'], 4)
    line = json.dumps(res)
    print(line)
    if flags.out:
        with open(flags.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
