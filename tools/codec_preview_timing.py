"""Preview decode (--channels K) against the full decode on the 512 x 768 synthetic natural image of codec_tiled_timing.py, in ONE
run: format 1 (one stream), format 2 at --tile 128 and format 5 at --tile 128; K = 4, 8, 16 and C, each beside the full decode
(channels=None, the existing entries).  Timed are the decoder call alone (decode_stream for format 1, decode_tiles_batch with q
staying on the device for the tiled formats) and decompress (container bytes -> image); and, for 8 files through decompress_many,
K = 8 against full.  All configurations are alternated inside every repeat, each call ended by a device synchronise, host clock;
medians and the spread (min .. max) of the repeats.  Every K is to be read against the full decode OF THE SAME RUN; K = C is the
control and must equal it within the spread.

The claim it decides: for formats 1 and 2 the decoder call at K = C / 4 is faster than the full decode by more than the recorded
spread, and its time is within 1.5 x of (K + 3) / (C + 3) of the full decode's (the share of the sweep's planes); format 5 is
held against its own figure, the share of the fronts: ((tw + 3) + 2 (th + 3) + 4 (K + 3) - 6) / ((tw + 3) + 2 (th + 3) + 4 (C + 3) - 6).
Prints one JSON line; --out writes it.

    python tools/codec_preview_timing.py [--repeats 5] [--out profiles/codec_preview_timing.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

FORMATS = (('format1', None, 'raster'), ('format2_tile128', 128, 'raster'), ('format5_tile128', 128, 'wavefront'))
MANY, MANY_K = 8, 8


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
    C = c.C
    ks = [4, 8, 16, C]
    configs = [None] + ks                                  # None: the full decode through the existing entries
    imgs = [np.ascontiguousarray(W.synthetic_image((1, 3, 512, 768), 'natural', seed=4 + i)[0].transpose(1, 2, 0)) for i in range(MANY)]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def decoder(head, order, k):
        if isinstance(head, codec.Container):
            return c.pred.decode_stream(head.payload, (head.C, head.h, head.w), head.first_sym, channels=k)
        return c.pred.decode_tiles_batch([(head.streams, head.first_syms, (head.C, head.h, head.w))], head.th, head.tw, want='q',
                                         order=order, channels=k)

    files, heads, t, tm = {}, {}, {}, {}
    fill = codec.fill_symbol(c.ae.get_centers_variable().detach().cpu().numpy())
    for name, tile, order in FORMATS:                      # the files, a warm-up of every path, and that every K obeys the rule
        c.tile, c.order, c.checked = (None if tile is None else (tile // c.factor, tile // c.factor)), order, False
        files[name] = c.compress_many(imgs)
        heads[name] = codec.parse_container(files[name][0])
        full = c.decode_symbols(files[name][0])[0]
        for k in configs:
            decoder(heads[name], order, k)
            c.decompress(files[name][0], channels=k)
            if k is not None:
                assert np.array_equal(c.decode_symbols(files[name][0], channels=k)[0], codec.preview_symbols(full, k, fill)), (name, k)
            t[name, k] = {'decoder': [], 'decompress': []}
        for k in (None, MANY_K):
            c.decompress_many(files[name], channels=k)
            tm[name, k] = []
    c.tile, c.order = None, 'raster'
    for _ in range(flags.repeats):
        for name, tile, order in FORMATS:
            for k in configs:
                t[name, k]['decoder'].append(timed(lambda: decoder(heads[name], order, k))[0])
                t[name, k]['decompress'].append(timed(lambda: c.decompress(files[name][0], channels=k))[0])
            for k in (None, MANY_K):
                tm[name, k].append(timed(lambda: c.decompress_many(files[name], channels=k))[0])

    def stats(v):
        return {'ms': [round(1e3 * x, 3) for x in v], 'median_ms': round(1e3 * float(np.median(v)), 3),
                'spread_ms': round(1e3 * (max(v) - min(v)), 3)}

    res = {'image': '512x768 synthetic natural, seeds 4..{} (seed 4 alone; all {} through decompress_many)'.format(3 + MANY, MANY),
           'repeats': flags.repeats, 'weights': 'synthetic', 'device': torch.cuda.get_device_name(0), 'C': C, 'formats': []}
    for name, tile, order in FORMATS:
        head = heads[name]
        row = {'format': name, 'file_bytes': len(files[name][0]), 'tiles': len(head.streams) if hasattr(head, 'streams') else 1, 'full': {}}
        for what in ('decoder', 'decompress'):
            row['full'][what] = stats(t[name, None][what])
        row['channels'] = []
        for k in ks:
            if order == 'wavefront':
                th, tw = min(head.th, head.h), min(head.tw, head.w)
                expected = ((tw + 3) + 2 * (th + 3) + 4 * (k + 3) - 6) / float((tw + 3) + 2 * (th + 3) + 4 * (C + 3) - 6)
            else:
                expected = (k + 3) / float(C + 3)
            r = {'K': k, 'expected_share_of_steps': round(expected, 4)}
            for what in ('decoder', 'decompress'):
                r[what] = stats(t[name, k][what])
                r[what + '_over_full'] = round(r[what]['median_ms'] / row['full'][what]['median_ms'], 4)
            a, b = row['full']['decoder'], r['decoder']
            spread = max(a['spread_ms'], b['spread_ms'])
            r['decoder_faster_by_more_than_spread'] = bool(a['median_ms'] - b['median_ms'] > spread)
            r['decoder_equals_full_within_spread'] = bool(abs(a['median_ms'] - b['median_ms']) <= spread)
            r['decoder_share_over_expected'] = round(r['decoder_over_full'] / expected, 3)
            row['channels'].append(r)
        quarter = [r for r in row['channels'] if r['K'] == C // 4][0]
        row['claim_K_quarter'] = {'K': C // 4, 'faster_by_more_than_spread': quarter['decoder_faster_by_more_than_spread'],
                                  'within_1.5x_of_expected_share': bool(1 / 1.5 <= quarter['decoder_share_over_expected'] <= 1.5),
                                  'control_K_equals_C_within_spread': row['channels'][-1]['decoder_equals_full_within_spread']}
        row['decompress_many'] = {'files': MANY, 'full': stats(tm[name, None]), 'K': MANY_K, 'preview': stats(tm[name, MANY_K])}
        row['decompress_many']['preview_over_full'] = round(row['decompress_many']['preview']['median_ms'] /
                                                            row['decompress_many']['full']['median_ms'], 4)
        res['formats'].append(row)
    line = json.dumps(res)
    print(line)
    if flags.out:
        with open(flags.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
