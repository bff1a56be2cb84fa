"""Front-layered tiles (format 8, --tile 128 --front-progressive) against wavefront tiles (format 5, --tile 128 --wavefront) and layered
tiles (format 6, --tile 128 --progressive: the same layer ends C/8, C/4, C/2, C) on the 512 x 768 synthetic natural image of
codec_tiled_timing.py, in ONE run:
  compress and decompress of the three formats;
  the decoder call alone (PredictionNetwork.decode_tiles_batch of the parsed file, want='q': the tables' upload, the slot fill, the one
  decoder launch and the read-back of the status words; no parsing, no autoencoder);
  decompress_partial of the format-6 and the format-8 file cut at every layer prefix (layer_prefix_bytes(g), g = 1 .. G);
  the payloads and every prefix length of formats 6 and 8.
All configurations are alternated inside every repeat, each call ended by a device synchronise, host clock; medians and the spread
(max - min) of the repeats.  The claims it decides, each against figures of the same run:
  full_decode_within_spread   |format-8 decoder call - format-5 decoder call| <= the larger of the two spreads
  partial_faster_than_format6 per layer end: format-6 partial - format-8 partial > the larger of the two spreads
  prefix_bytes                how much longer the format-8 prefixes are (bytes behind the header, format 8 over format 6)
Nothing is asserted about times or sizes; the pixels are (the three formats agree, every prefix == the --channels preview).
Prints one JSON line; --out writes it.

    python tools/codec_fronts_timing.py [--repeats 5] [--out profiles/codec_fronts_timing.json]
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
FORMATS = (5, 6, 8)


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
        c.tile, c.order = tile, 'wavefront' if version == 5 else 'raster'
        c.layers, c.front_layers = 'default' if version == 6 else None, 'default' if version == 8 else None
        try:
            return c.compress(img)
        finally:
            c.tile, c.order, c.layers, c.front_layers = None, 'raster', None, None

    def decoder_call(head):
        kw = {'order': 'wavefront'} if head.version == 5 else codec._ends_kw(head)
        return c.pred.decode_tiles_batch([(head.streams, head.first_syms, (head.C, head.h, head.w))], head.th, head.tw, want='q', **kw)

    files = {v: compress(v) for v in FORMATS}              # also the warm-up of the encoders
    heads = {v: codec.parse_container(files[v]) for v in FORMATS}
    ends = heads[8].layer_ends
    assert heads[6].layer_ends == ends
    G = len(ends)
    cuts = {v: [files[v][:codec.layer_prefix_bytes(files[v], g)] for g in range(1, G + 1)] for v in (6, 8)}
    whole = c.decompress(files[5])
    for v in (6, 8):                                       # the pixels, and the warm-up of every decoder form that is timed
        assert np.array_equal(c.decompress(files[v]), whole)
        for g, cut in enumerate(cuts[v]):
            out, report = c.decompress_partial(cut)
            assert report.layers_decoded == g + 1 and np.array_equal(out, c.decompress(files[5], channels=ends[g]))
    qs = [decoder_call(heads[v])[0] for v in FORMATS]
    assert torch.equal(qs[0], qs[1]) and torch.equal(qs[0], qs[2])
    t = {(what, v): [] for what in ('compress', 'decompress', 'decoder_call') for v in FORMATS}
    t.update({('partial', v, g): [] for v in (6, 8) for g in range(G)})
    for _ in range(flags.repeats):
        for v in FORMATS:
            t['compress', v].append(timed(lambda: compress(v))[0])
            t['decompress', v].append(timed(lambda: c.decompress(files[v]))[0])
            t['decoder_call', v].append(timed(lambda: decoder_call(heads[v]))[0])
        for g in range(G):
            for v in (6, 8):
                t['partial', v, g].append(timed(lambda: c.decompress_partial(cuts[v][g]))[0])

    def stats(v):
        return {'ms': [round(1e3 * x, 3) for x in v], 'median_ms': round(1e3 * float(np.median(v)), 3),
                'spread_ms': round(1e3 * (max(v) - min(v)), 3)}

    name = lambda v: 'format{}'.format(v)
    nt = len(heads[8].first_syms)
    header = codec.layer_prefix_bytes(files[8], 0)
    assert header == codec.layer_prefix_bytes(files[6], 0)
    res = {'image': '512x768 synthetic natural, seed 4', 'tile': TILE, 'layer_ends': ends, 'tiles': nt, 'repeats': flags.repeats,
           'weights': 'synthetic', 'device': torch.cuda.get_device_name(0),
           'file_bytes': {name(v): len(files[v]) for v in FORMATS},
           'payload_bytes': {name(v): len(heads[v].payload) for v in FORMATS},
           'header_bytes': header,
           'prefix_bytes': {name(v): [len(cut) for cut in cuts[v]] for v in (6, 8)}}
    res['payload_bytes']['format8_minus_format5'] = len(heads[8].payload) - len(heads[5].payload)
    res['payload_bytes']['format8_minus_format6'] = len(heads[8].payload) - len(heads[6].payload)
    for what in ('compress', 'decompress', 'decoder_call'):
        res[what] = {name(v): stats(t[what, v]) for v in FORMATS}
    res['decompress_partial'] = []
    for g in range(G):
        r = {'layers': g + 1, 'channels': ends[g]}
        for v in (6, 8):
            r[name(v)] = dict(stats(t['partial', v, g]), bytes=len(cuts[v][g]))
        r['format8_over_format6_time'] = round(r['format8']['median_ms'] / r['format6']['median_ms'], 4)
        r['format8_over_format6_bytes_behind_header'] = round((len(cuts[8][g]) - header) / float(max(len(cuts[6][g]) - header, 1)), 4)
        res['decompress_partial'].append(r)
    d5, d8 = res['decoder_call']['format5'], res['decoder_call']['format8']
    res['claims'] = {
        'full_decode_within_spread': {
            'format8_minus_format5_ms': round(d8['median_ms'] - d5['median_ms'], 3), 'spread_ms': max(d5['spread_ms'], d8['spread_ms']),
            'holds': abs(d8['median_ms'] - d5['median_ms']) <= max(d5['spread_ms'], d8['spread_ms'])},
        'partial_faster_than_format6': [
            {'channels': r['channels'], 'format6_minus_format8_ms': round(r['format6']['median_ms'] - r['format8']['median_ms'], 3),
             'spread_ms': max(r['format6']['spread_ms'], r['format8']['spread_ms']),
             'holds': r['format6']['median_ms'] - r['format8']['median_ms'] > max(r['format6']['spread_ms'], r['format8']['spread_ms'])}
            for r in res['decompress_partial']],
        'prefix_bytes_format8_over_format6': [r['format8_over_format6_bytes_behind_header'] for r in res['decompress_partial']]}
    line = json.dumps(res)
    print(line)
    if flags.out:
        with open(flags.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
