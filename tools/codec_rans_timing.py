"""Lane-parallel rANS tiles (format 12) against wavefront tiles (format 5): decoder call, decompress and compress times and payload
bytes of a 512 x 768 picture at --tile 128, for W in {8, 16, 32, 64} coders per tile.  The two formats alternate within the repeats;
medians and spread (max - min) are written to profiles/codec_rans_timing.json.

    python tools/codec_rans_timing.py [--out profiles/codec_rans_timing.json] [--repeats 7]

Synthetic weights: the payload bytes say nothing about a trained model; the times per front and per symbol do not depend on the
weights."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default='profiles/codec_rans_timing.json')
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

    def as_format(lanes):
        c.tile, c.order, c.rans = (cells, cells), ('raster' if lanes else 'wavefront'), (lanes or None)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def decoder_call(head):
        kw = {'order': 'rans', 'lanes': head.lanes} if isinstance(head, codec.RansContainer) else {'order': 'wavefront'}
        return lambda: c.pred.decode_tiles_batch([(head.streams, head.first_syms, (head.C, head.h, head.w))], head.th, head.tw, want='q', **kw)

    def stats(ms):
        return {'ms': [round(v, 3) for v in ms], 'median_ms': round(float(np.median(ms)), 3), 'spread_ms': round(max(ms) - min(ms), 3)}

    fronts = (cells + 3) + 2 * (cells + 3) + 4 * (c.C + 3) - 6
    result = {'image': '{}x{} synthetic natural, seed 4'.format(H, W_), 'tile': tile, 'repeats': flags.repeats, 'weights': 'synthetic',
              'device': torch.cuda.get_device_name(0), 'front_steps_per_tile': fronts,
              'predicted_decoder_ms': round(fronts * 35e-3, 3), 'cases': []}
    for lanes in codec.RANS_LANES:
        files, heads = {}, {}
        for fmt in (5, 12):
            as_format(lanes if fmt == 12 else 0)
            files[fmt] = c.compress(img)
            heads[fmt] = codec.parse_container(files[fmt])
        assert np.array_equal(c.decompress(files[5]), c.decompress(files[12]))              # (also the warm-up of both formats)
        times = {(fmt, what): [] for fmt in (5, 12) for what in ('decoder', 'decompress', 'compress')}
        for _ in range(flags.repeats):
            for fmt in (5, 12):                                                              # alternated within a repeat
                as_format(lanes if fmt == 12 else 0)
                times[fmt, 'decoder'].append(timed(decoder_call(heads[fmt]))[1])
                times[fmt, 'decompress'].append(timed(lambda: c.decompress(files[fmt]))[1])
                times[fmt, 'compress'].append(timed(lambda: c.compress(img))[1])
        ntiles = len(heads[12].streams)
        case = {'lanes': lanes,
                'payload_bytes': {'format_5': len(heads[5].payload), 'format_12': len(heads[12].payload), 'state_bytes': 4 * lanes * ntiles},
                'file_bytes': {'format_5': len(files[5]), 'format_12': len(files[12])}}
        for (fmt, what), ms in times.items():
            case['{}_format_{}'.format(what, fmt)] = stats(ms)
        result['cases'].append(case)
        print('W {}: decoder {:.2f} -> {:.2f} ms, decompress {:.2f} -> {:.2f} ms, compress {:.2f} -> {:.2f} ms, payload {} -> {} bytes '
              '({} of them states)'.format(lanes, case['decoder_format_5']['median_ms'], case['decoder_format_12']['median_ms'],
                                           case['decompress_format_5']['median_ms'], case['decompress_format_12']['median_ms'],
                                           case['compress_format_5']['median_ms'], case['compress_format_12']['median_ms'],
                                           case['payload_bytes']['format_5'], case['payload_bytes']['format_12'],
                                           case['payload_bytes']['state_bytes']), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(flags.out)), exist_ok=True)
    with open(flags.out, 'w') as f:
        json.dump(result, f)
        f.write('\n')


if __name__ == '__main__':
    main()
