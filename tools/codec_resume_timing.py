"""A layered file (format 6, --tile 128 --progressive) shown while it arrives: the stream decoder, which goes on where its last picture
stopped, against decompress_partial, which starts every tile at channel 0 again, on the 512 x 768 synthetic natural image of
codec_layered_timing.py, in ONE run.  The file is fed at its four layer ends; per layer end
  image()      of a StreamDecoder that has drawn the layer ends before it   against decompress_partial of the same prefix (the same pixels),
  advance()    of the decoder session alone (decode + concealment launch)   against decode_tiles_batch(channels = that layer's end) alone.
Both pairs are alternated inside every repeat after one warm-up round (a repeat opens a new StreamDecoder / session: opening is not
timed, it happens once per file), each call ended by a device synchronise, host clock; medians and the spread (min .. max) of the
repeats, per step and for the sum over the four steps.  Every figure is to be read against its partner OF THE SAME RUN.
The claim to decide: the sum of the session's decoder time over the four steps lies below the sum of the re-decodes by more than the
recorded spread and near 35 / 72 of it (planes swept: (4 + 3) + 4 + 8 + 16 against 7 + 11 + 19 + 35); the last step alone near 16 / 35
of a full decode.  Nothing is asserted about times; the pixels are.
Prints one JSON line; --out writes it.

    python tools/codec_resume_timing.py [--repeats 5] [--out profiles/codec_resume_timing.json]
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
    c.tile, c.layers = (TILE // c.factor, TILE // c.factor), 'default'
    try:
        data = c.compress(img)
    finally:
        c.tile, c.layers = None, None
    head = codec.parse_container(data)
    ends, G, nt = head.layer_ends, len(head.layer_ends), len(head.first_syms)
    cuts = [codec.layer_prefix_bytes(data, g) for g in range(1, G)] + [len(data)]
    volume = (head.streams, head.first_syms, (head.C, head.h, head.w))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def one_round(t=None):
        """the four steps, the four calls of every step alternated; t: where the times go (None: the warm-up, which checks pixels)"""
        dec, session, pos = c.open_stream(), c.pred.open_layers([volume[2]], head.th, head.tw, ends), 0
        for g in range(1, G + 1):
            assert dec.feed(data[pos:cuts[g - 1]])
            pos = cuts[g - 1]
            prefix = data[:pos]
            calls = [('stream_image', lambda: dec.image()[0]), ('decompress_partial', lambda: c.decompress_partial(prefix)[0]),
                     ('session_advance', lambda: session.advance([volume[:2]], [[g] * nt], want='q')[0][0]),
                     ('decode_tiles_batch', lambda: c.pred.decode_tiles_batch([volume], head.th, head.tw, want='q', channels=ends[g - 1],
                                                                            layer_ends=ends)[0])]
            got = {}
            for name, fn in calls:
                dt, got[name] = timed(fn)
                if t is not None:
                    t[name][g - 1].append(dt)
            if t is None:
                assert np.array_equal(got['stream_image'], got['decompress_partial']), g
                assert torch.equal(got['session_advance'], got['decode_tiles_batch']), g
        assert dec._session.launches == G and session.launches == G

    one_round()                                            # warm-up: workspaces, kernels, the autoencoder's plan
    names = ('stream_image', 'decompress_partial', 'session_advance', 'decode_tiles_batch')
    t = {name: [[] for _ in range(G)] for name in names}
    for _ in range(flags.repeats):
        one_round(t)

    def stats(v):
        return {'ms': [round(1e3 * x, 3) for x in v], 'median_ms': round(1e3 * float(np.median(v)), 3),
                'spread_ms': round(1e3 * (max(v) - min(v)), 3)}

    res = {'image': '512x768 synthetic natural, seed 4', 'tile': TILE, 'layer_ends': ends, 'tiles': nt, 'repeats': flags.repeats,
           'weights': 'synthetic', 'device': torch.cuda.get_device_name(0), 'file_bytes': len(data), 'fed_at_bytes': cuts,
           'planes_swept': {'resumed': [ends[0] + 3] + [b - a for a, b in zip(ends, ends[1:])], 'redecoded': [e + 3 for e in ends]}}
    for name in names:
        res[name] = {'steps': [stats(v) for v in t[name]], 'sum': stats([sum(step[r] for step in t[name]) for r in range(flags.repeats)])}
    res['stream_over_partial_sum'] = round(res['stream_image']['sum']['median_ms'] / res['decompress_partial']['sum']['median_ms'], 4)
    res['session_over_redecode_sum'] = round(res['session_advance']['sum']['median_ms'] / res['decode_tiles_batch']['sum']['median_ms'], 4)
    res['session_last_step_over_full_decode'] = round(res['session_advance']['steps'][-1]['median_ms'] /
                                                      res['decode_tiles_batch']['steps'][-1]['median_ms'], 4)
    line = json.dumps(res)
    print(line)
    if flags.out:
        with open(flags.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
