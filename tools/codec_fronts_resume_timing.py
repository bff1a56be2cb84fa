"""A front-layered file (format 8, --tile 128 --front-progressive) shown while it arrives, on the 512 x 768 synthetic natural image of
codec_resume_timing.py, in ONE run and with that tool's method.  The file is fed at its four layer ends; per layer end
  1. partial8          decompress --partial (Codec.decompress_partial) of the format-8 prefix: what a viewer had before stream --fronts,
                       every tile swept from front 0 again,
  2. stream8_image     image() of a StreamDecoder(fronts=True) that has drawn the layer ends before it (the same pixels as 1), and
     session8_advance  advance() of a front session alone (the decoder launch + the concealment launch),
  3. stream6_image     image() of the format-6 stream of the same image, and session6_advance, its session alone.
The calls of a step are alternated inside every repeat after one warm-up round (a repeat opens new decoders / sessions: opening is not
timed), each call ended by a device synchronise, host clock; medians and the spread (min .. max) of the repeats, per step and for the
sum over the four steps.  Every figure is to be read against its partners OF THE SAME RUN.
What the step arithmetic predicts for a (32, 16, 16) tile: 191 decoder steps for (2) against 79 + 95 + 127 + 191 = 492 for (1); no ratio
of times is fixed in advance (a step's cost grows with the front).  Nothing is asserted about times; the pixels are.
Prints one JSON line; --out writes it.

    python tools/codec_fronts_resume_timing.py [--repeats 5] [--out profiles/codec_fronts_resume_timing.json]
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
    files = {}
    for version, attr in ((8, 'front_layers'), (6, 'layers')):
        c.tile = (TILE // c.factor, TILE // c.factor)
        setattr(c, attr, 'default')
        try:
            files[version] = c.compress(img)
        finally:
            c.tile, c.layers, c.front_layers = None, None, None
    heads = {v: codec.parse_container(d) for v, d in files.items()}
    head = heads[8]
    assert head.version == 8 and heads[6].version == 6 and heads[6].layer_ends == head.layer_ends
    ends, G, nt = head.layer_ends, len(head.layer_ends), len(head.first_syms)
    cuts = {v: [codec.layer_prefix_bytes(d, g) for g in range(1, G)] + [len(d)] for v, d in files.items()}
    volumes = {v: (h.streams, h.first_syms, (h.C, h.h, h.w)) for v, h in heads.items()}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def one_round(t=None):
        """the four steps, the calls of every step alternated; t: where the times go (None: the warm-up, which checks pixels)"""
        dec8, dec6 = c.open_stream(fronts=True), c.open_stream()
        session8 = c.pred.open_layers([volumes[8][2]], head.th, head.tw, front_ends=ends)
        session6 = c.pred.open_layers([volumes[6][2]], head.th, head.tw, ends)
        pos = {8: 0, 6: 0}
        for g in range(1, G + 1):
            for v, dec in ((8, dec8), (6, dec6)):
                assert dec.feed(files[v][pos[v]:cuts[v][g - 1]])
                pos[v] = cuts[v][g - 1]
            prefix8 = files[8][:pos[8]]
            calls = [('partial8', lambda: c.decompress_partial(prefix8)[0]), ('stream8_image', lambda: dec8.image()[0]),
                     ('session8_advance', lambda: session8.advance([volumes[8][:2]], [[g] * nt], want='q')[0][0]),
                     ('stream6_image', lambda: dec6.image()[0]),
                     ('session6_advance', lambda: session6.advance([volumes[6][:2]], [[g] * nt], want='q')[0][0])]
            got = {}
            for name, fn in calls:
                dt, got[name] = timed(fn)
                if t is not None:
                    t[name][g - 1].append(dt)
            if t is None:
                assert np.array_equal(got['stream8_image'], got['partial8']), g
                assert np.array_equal(got['stream6_image'], got['partial8']), g      # the two formats hold the same symbols
                assert torch.equal(got['session8_advance'], got['session6_advance']), g
        assert dec8._session.fronts and dec8._session.launches == G and session8.launches == G and dec6._session.launches == G

    one_round()                                            # warm-up: workspaces, kernels, the autoencoder's plan
    names = ('partial8', 'stream8_image', 'session8_advance', 'stream6_image', 'session6_advance')
    t = {name: [[] for _ in range(G)] for name in names}
    for _ in range(flags.repeats):
        one_round(t)

    def stats(v):
        return {'ms': [round(1e3 * x, 3) for x in v], 'median_ms': round(1e3 * float(np.median(v)), 3),
                'spread_ms': round(1e3 * (max(v) - min(v)), 3)}

    a, b = head.th, head.tw
    steps = lambda e: (b + 3) + 2 * (a + 3) + 4 * (e + 3) - 6
    res = {'image': '512x768 synthetic natural, seed 4', 'tile': TILE, 'layer_ends': ends, 'tiles': nt, 'repeats': flags.repeats,
           'weights': 'synthetic', 'device': torch.cuda.get_device_name(0), 'file_bytes': {str(v): len(d) for v, d in files.items()},
           'fed_at_bytes': {str(v): cuts[v] for v in files},
           'decoder_steps_per_full_tile': {'resumed': [steps(ends[0])] + [4 * (y - x) for x, y in zip(ends, ends[1:])], 'redecoded': [steps(e) for e in ends]}}
    for name in names:
        res[name] = {'steps': [stats(v) for v in t[name]], 'sum': stats([sum(step[r] for step in t[name]) for r in range(flags.repeats)])}
    ratio = lambda x, y: round(res[x]['sum']['median_ms'] / res[y]['sum']['median_ms'], 4)
    res['stream8_over_partial8_sum'] = ratio('stream8_image', 'partial8')
    res['session8_over_partial8_sum'] = ratio('session8_advance', 'partial8')
    res['stream8_over_stream6_sum'] = ratio('stream8_image', 'stream6_image')
    res['session8_over_session6_sum'] = ratio('session8_advance', 'session6_advance')
    line = json.dumps(res)
    print(line)
    if flags.out:
        with open(flags.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
