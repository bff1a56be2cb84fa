"""Region decode, on synthetic natural images of 512 x 768 and 2160 x 3840 written with --tile 128 --checked (format 4), synthetic
weights, in ONE run:
  1. decompress_region of a 512 x 512 interior rectangle against decompress of the same file, and beside them their two halves timed
     on their own: the tile decoder's call (decode_tiles_batch over the window's tiles / over all tiles, q left on the device) and the
     autoencoder's decoder pass (over the window with the picture's plan forced / over the picture).  At 512 x 768 the rectangle's
     reach covers every tile (`tiles` says so): the region call IS decompress plus a crop there.
  2. decompress_regions_many of 8 such rectangles of the file against 8 decompress calls -- what a tile server does for 8 requests
     today.
The workspace of each half is recorded in bytes (the tile decoder's: one slot per tile; the autoencoder's: its activations).
The calls of a group are alternated inside every repeat after a warm-up round, each ended by a device synchronise, host clock; medians
and the spread (max - min) of the repeats.  Every figure is to be read against its partner OF THE SAME RUN; nothing is asserted about
times, the pixels are: every region equals the crop of decompress.  Prints one JSON line; --out writes it.

    python tools/codec_region_timing.py [--repeats 7] [--out profiles/codec_region_timing.json]
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
REQUESTS = 8
SIDE = 512


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--repeats', type=int, default=7)
    p.add_argument('--out')
    flags = p.parse_args()
    from imgcomp_cvpr_amd import codec, config_parser as cp, weights as W
    from imgcomp_cvpr_amd._lib import lib
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda:0')
    ae_cfg, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc_cfg, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    c = codec.Codec(ae_cfg, pc_cfg, W.synthetic_weights(ae_cfg, pc_cfg), dev, tile=(TILE // 8, TILE // 8), checked=True)
    k = int(c.pc._k)

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

    res = {'tile': TILE, 'format': 4, 'rectangle': '{0} x {0}, interior'.format(SIDE), 'requests': REQUESTS, 'repeats': flags.repeats,
           'weights': 'synthetic', 'device': torch.cuda.get_device_name(0)}
    for H, Wd in ((512, 768), (2160, 3840)):
        img = np.ascontiguousarray(W.synthetic_image((1, 3, H, Wd), 'natural', seed=4)[0].transpose(1, 2, 0))
        data = c.compress(img)
        head = codec.parse_container(data)
        rect = ((Wd - SIDE) // 2, (H - SIDE) // 2, SIDE, SIDE)
        _, plan, win, bits = c._region_head(data, rect)
        src = head if win is None else win                                  # (None: the rectangle needs every tile)
        volume = lambda s: [(s.streams, s.first_syms, (s.C, s.h, s.w))]
        q_win = c.pred.decode_tiles_batch(volume(src), src.th, src.tw, want='q')[0]
        q_all = c.pred.decode_tiles_batch(volume(head), head.th, head.tw, want='q')[0]
        if win is not None:                                                  # the forced plan, before the cast: the picture's floats, bit for bit
            (oy, ox), top, left = plan.offset, ((-H) % 8) // 2, ((-Wd) % 8) // 2
            a = c.ae.decode(q_win[None], is_training=False, plan_flags=bits)[0, :, oy:oy + SIDE, ox:ox + SIDE]
            b = c.ae.decode(q_all[None], is_training=False)[0, :, rect[1] + top:rect[1] + top + SIDE, rect[0] + left:rect[0] + left + SIDE]
            assert torch.equal(a, b), '{} values of the window differ from the picture before the cast'.format(int((a != b).sum()))
        whole = c.decompress(data)
        crop = lambda r: whole[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]

        def check(got):
            assert np.array_equal(got['decompress_region'], crop(rect)) and np.array_equal(got['decompress'], whole)
        one = alternate([('decompress_region', lambda: c.decompress_region(data, rect)),
                         ('decompress', lambda: c.decompress(data)),
                         ('region_tile_decoder', lambda: c.pred.decode_tiles_batch(volume(src), src.th, src.tw, want='q')),
                         ('whole_tile_decoder', lambda: c.pred.decode_tiles_batch(volume(head), head.th, head.tw, want='q')),
                         ('region_autoencoder', lambda: c.ae.decode(q_win[None], is_training=False, plan_flags=bits)),
                         ('whole_autoencoder', lambda: c.ae.decode(q_all[None], is_training=False))], check)
        one['region_over_decompress'] = round(one['decompress_region']['median_ms'] / one['decompress']['median_ms'], 4)
        tiles_of = lambda s: len(s.streams)
        ws = lambda s: int(lib.ic_pc_decode_tiles_batch_workspace_bytes(s.C, min(s.th, s.h), min(s.tw, s.w), tiles_of(s), 1, k))
        one['tiles'] = {'region': tiles_of(src), 'whole': tiles_of(head)}
        one['window_cells'] = [src.h, src.w]
        one['decoder_pass_pixels'] = {'region': [8 * src.h, 8 * src.w], 'whole': [8 * head.h, 8 * head.w]}
        one['workspace_bytes'] = {'region_tile_decoder': ws(src), 'whole_tile_decoder': ws(head),
                                  'region_autoencoder': int(lib.ic_ae_workspace_bytes(1, 8 * src.h, 8 * src.w, c.C)),
                                  'whole_autoencoder': int(lib.ic_ae_workspace_bytes(1, 8 * head.h, 8 * head.w, c.C))}
        one['plan_bits'] = '{:#x}'.format(bits)
        one['file_bytes'] = len(data)

        # 2. eight rectangles of the file, spread over the interior
        rs = np.random.RandomState(5)
        rects = [(int(rs.randint(0, Wd - SIDE + 1)), int(rs.randint(0, H - SIDE + 1)), SIDE, SIDE) for _ in range(REQUESTS)]

        def same(got):
            assert all(np.array_equal(x, crop(r)) for x, r in zip(got['regions_many'], rects))
        many = alternate([('regions_many', lambda: c.decompress_regions_many([(data, r) for r in rects])),
                          ('decompress_loop', lambda: [c.decompress(data) for _ in rects])], same)
        many['many_over_loop'] = round(many['regions_many']['median_ms'] / many['decompress_loop']['median_ms'], 4)
        many['tiles'] = [len(c._region_head(data, r)[1].tiles) for r in rects]
        res['{}x{}'.format(H, Wd)] = {'one': one, 'many': many}
    line = json.dumps(res)
    print(line)
    if flags.out:
        with open(flags.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
