"""Tiled against untiled codec on the 512 x 768 synthetic natural image of test_encode_stream_equals_parent_file[kodak] (symbol volume
32 x 64 x 96): for no tiles and for square tiles of 256, 128 and 64 pixels -- payload bytes, file bytes, compress and decompress
(image <-> container bytes, end to end), and the coders alone (encode_tiles / decode_tiles against encode_stream / decode_stream of
the whole volume).  The configurations are alternated inside every repeat, each call ended by a device synchronise, host clock.
Every tiled figure is to be read against the untiled figure OF THE SAME RUN.  Prints one JSON line; --out writes it.

    python tools/codec_tiled_timing.py [--repeats 5] [--out profiles/codec_tiled_timing.json] [--decode_only PIXELS]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

TILES = (None, 256, 128, 64)


def sweep_steps(C, h, w):
    """steps of the activation-cache decoder's sweep over one padded volume"""
    return (C + 3) * (h + 6) * (w + 6)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--out')
    p.add_argument('--decode_only', type=int, default=None, metavar='PIXELS',
                   help='only decode_tiles with this tile size, 0 = only the untiled decode_stream (for a kernel trace)')
    flags = p.parse_args()
    from imgcomp_cvpr_amd import codec, config_parser as cp, weights as W
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda:0')
    ae_cfg, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc_cfg, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    wts = W.synthetic_weights(ae_cfg, pc_cfg)
    c = codec.Codec(ae_cfg, pc_cfg, wts, dev)
    planar = W.synthetic_image((1, 3, 512, 768), 'natural', seed=4)
    img = np.ascontiguousarray(planar[0].transpose(1, 2, 0))
    sym_dev = c.ae.encode(torch.as_tensor(planar).float().to(dev), is_training=False).symbols[0]
    sym = sym_dev.cpu().numpy()
    C, h, w = sym.shape

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def encode(tile):
        if tile is None:
            return [c.pred.encode_stream(sym_dev)]
        return c.pred.encode_tiles(sym_dev, tile // c.factor, tile // c.factor)

    def decode(tile, coded):
        if tile is None:
            return c.pred.decode_stream(coded[0][0], sym.shape, coded[0][1])
        return c.pred.decode_tiles([b for b, _ in coded], [f for _, f in coded], sym.shape, tile // c.factor, tile // c.factor)

    if flags.decode_only is not None:
        tile = flags.decode_only or None
        coded = encode(tile)
        for _ in range(flags.repeats):
            assert np.array_equal(decode(tile, coded), sym)
        torch.cuda.synchronize()
        print(json.dumps({'decode_only': tile, 'streams': len(coded)}))
        return

    coded, files = {}, {}
    for tile in TILES:                                     # warm-up of every path, and the sizes
        c.tile = None if tile is None else (tile // c.factor, tile // c.factor)
        coded[tile] = encode(tile)
        assert np.array_equal(decode(tile, coded[tile]), sym), tile
        files[tile] = c.compress(img)
        c.decompress(files[tile])
    want = c.decompress(files[None])
    t = {tile: {'encode': [], 'decode': [], 'compress': [], 'decompress': []} for tile in TILES}
    for _ in range(flags.repeats):
        for tile in TILES:
            c.tile = None if tile is None else (tile // c.factor, tile // c.factor)
            t[tile]['encode'].append(timed(lambda: encode(tile))[0])
            t[tile]['decode'].append(timed(lambda: decode(tile, coded[tile]))[0])
            t[tile]['compress'].append(timed(lambda: c.compress(img))[0])
            dt, out = timed(lambda: c.decompress(files[tile]))
            t[tile]['decompress'].append(dt)
            assert np.array_equal(out, want), tile
    ms = lambda v: [round(1e3 * x, 3) for x in v]
    med = lambda v: round(1e3 * float(np.median(v)), 3)
    whole = sweep_steps(C, h, w)
    res = {'image': '512x768 synthetic natural, seed 4', 'symbols': int(sym.size), 'repeats': flags.repeats,
           'weights': 'synthetic (no trained checkpoint: the bpp overhead of a trained context model is not measured here)',
           'device': torch.cuda.get_device_name(0), 'configs': []}
    for tile in TILES:
        head = codec.parse_container(files[tile])
        row = {'tile_pixels': tile, 'streams': len(coded[tile]), 'payload_bytes': len(head.payload), 'file_bytes': len(files[tile]),
               'payload_over_untiled': round(len(head.payload) / float(len(codec.parse_container(files[None]).payload)), 5),
               'encode_ms': ms(t[tile]['encode']), 'decode_ms': ms(t[tile]['decode']),
               'compress_ms': ms(t[tile]['compress']), 'decompress_ms': ms(t[tile]['decompress']),
               'encode_median_ms': med(t[tile]['encode']), 'decode_median_ms': med(t[tile]['decode']),
               'compress_median_ms': med(t[tile]['compress']), 'decompress_median_ms': med(t[tile]['decompress'])}
        if tile is not None:
            # the largest tile's sweep against the whole volume's: what one work-group of the tiled launch has to do
            e = min(tile // c.factor, h), min(tile // c.factor, w)
            ratio = sweep_steps(C, e[0], e[1]) / float(whole)
            row['sweep_step_ratio'] = round(ratio, 5)
            row['decode_over_untiled_same_run'] = round(med(t[tile]['decode']) / med(t[None]['decode']), 5)
            row['decode_expectation_2x_ratio'] = round(2 * ratio, 5)
            row['decode_within_expectation'] = bool(med(t[tile]['decode']) <= 2 * ratio * med(t[None]['decode']))
            row['encode_over_untiled_same_run'] = round(med(t[tile]['encode']) / med(t[None]['encode']), 5)
        res['configs'].append(row)
    line = json.dumps(res)
    print(line)
    if flags.out:
        with open(flags.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
