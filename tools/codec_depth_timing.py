"""Depth-mapped tiles (format 10) against wavefront tiles (format 5): decoder call, decompress and compress times, payload bytes, live
share and front steps of a 512 x 768 picture at --tile 128, at cap in {none, 16, 8, 4} and depth blocks B in {1, 2, 4, 8}.  The two
formats alternate within the repeats; medians and spread (max - min) are written to profiles/codec_depth_timing.json.

    python tools/codec_depth_timing.py [--out profiles/codec_depth_timing.json] [--repeats 7]

Synthetic weights: the payload bytes and the live share say nothing about a trained model (its importance map decides both);
the times per live symbol and per front step do not depend on the weights."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default='profiles/codec_depth_timing.json')
    p.add_argument('--repeats', type=int, default=7)
    p.add_argument('--device', default='cuda:0')
    flags = p.parse_args()
    import torch
    from imgcomp_cvpr_amd import codec, config_parser as cp, weights as W
    ae_cfg, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc_cfg, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    c = codec.Codec(ae_cfg, pc_cfg, W.synthetic_weights(ae_cfg, pc_cfg), flags.device)
    H, W_, tile = 512, 768, 128
    img = np.ascontiguousarray(W.synthetic_image((1, 3, H, W_), 'natural', seed=4)[0].transpose(1, 2, 0))
    cells = tile // c.factor

    def as_format(B):
        c.tile, c.order, c.depth_block = (cells, cells), ('raster' if B else 'wavefront'), (B or None)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def decoder_call(head):
        kw = {'order': 'wavefront'}
        if isinstance(head, codec.DepthContainer):
            kw['depth_block'] = head.depth_block
        return lambda: c.pred.decode_tiles_batch([(head.streams, head.first_syms, (head.C, head.h, head.w))], head.th, head.tw, want='q', **kw)

    def stats(ms):
        return {'ms': [round(v, 3) for v in ms], 'median_ms': round(float(np.median(ms)), 3), 'spread_ms': round(max(ms) - min(ms), 3)}

    result = {'image': '{}x{} synthetic natural, seed 4'.format(H, W_), 'tile': tile, 'repeats': flags.repeats, 'weights': 'synthetic',
              'device': torch.cuda.get_device_name(0), 'cases': []}
    for cap in (None, 16, 8, 4):
        for B in (1, 2, 4, 8):
            files, heads = {}, {}
            for fmt in (5, 10):
                as_format(B if fmt == 10 else 0)
                files[fmt] = c.compress(img, cap=cap)
                heads[fmt] = codec.parse_container(files[fmt])
            assert np.array_equal(c.decompress(files[5]), c.decompress(files[10]))          # (also the warm-up of both formats)
            times = {(fmt, what): [] for fmt in (5, 10) for what in ('decoder', 'decompress', 'compress')}
            for _ in range(flags.repeats):
                for fmt in (5, 10):                                                          # alternated within a repeat
                    as_format(B if fmt == 10 else 0)
                    times[fmt, 'decoder'].append(timed(decoder_call(heads[fmt]))[1])
                    times[fmt, 'decompress'].append(timed(lambda: c.decompress(files[fmt]))[1])
                    times[fmt, 'compress'].append(timed(lambda: c.compress(img, cap=cap))[1])
            h10 = heads[10]
            grid = codec.tile_grid(h10.h, h10.w, h10.th, h10.tw)
            planes = [codec.split_depth_stream(s, h10.C, a, b, B)[0] for (_, _, a, b), s in zip(grid, h10.streams)]
            live = sum(int(codec.depth_live(h10.C, a, b, d, B).sum()) for (_, _, a, b), d in zip(grid, planes))
            case = {'cap': cap, 'depth_block': B,
                    'payload_bytes': {'format_5': len(heads[5].payload), 'format_10': len(h10.payload), 'depth_plane_bytes': sum(d.size for d in planes)},
                    'file_bytes': {'format_5': len(files[5]), 'format_10': len(files[10])},
                    'live_symbols': live, 'live_share': round(live / float(h10.C * h10.h * h10.w), 4),
                    'front_steps_per_tile': {'format_5': codec.depth_front_steps(grid[0][2], grid[0][3], h10.C),
                                             'format_10': [codec.depth_front_steps(a, b, int(d.max())) for (_, _, a, b), d in zip(grid, planes)]}}
            for (fmt, what), ms in times.items():
                case['{}_format_{}'.format(what, fmt)] = stats(ms)
            result['cases'].append(case)
            print('cap {} B {}: decoder {:.2f} -> {:.2f} ms, decompress {:.2f} -> {:.2f} ms, compress {:.2f} -> {:.2f} ms, payload {} -> {} bytes, '
                  'live share {:.3f}'.format(cap, B, case['decoder_format_5']['median_ms'], case['decoder_format_10']['median_ms'],
                                             case['decompress_format_5']['median_ms'], case['decompress_format_10']['median_ms'],
                                             case['compress_format_5']['median_ms'], case['compress_format_10']['median_ms'],
                                             case['payload_bytes']['format_5'], case['payload_bytes']['format_10'], case['live_share']), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(flags.out)), exist_ok=True)
    with open(flags.out, 'w') as f:
        json.dump(result, f)
        f.write('\n')


if __name__ == '__main__':
    main()
