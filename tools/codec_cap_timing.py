"""The importance-map cap at encode, on the 512 x 768 synthetic natural image of the other codec timings with --tile 128, in ONE run:
  1. compress_plain / compress_cap_inf   Codec.compress(img) against compress(img, cap=+inf): the same bytes, the second through
                                         ic_ae_encode_cap_f32 and the capped kernel.  Expected level; the spread says what "level" means.
  2. requantize                          ae.requantize of the kept bottleneck at T = 1 and at T = 16 levels a launch, all six outputs
                                         and symbols + qhard alone (what the budget search asks for); LAUNCHES launches per timed window.
  3. budget / bisection                  compress_to_budget at a budget halfway between the files of level 0 and level C, against a
                                         bisection of 9 codings over the same grid that runs compress(img, cap=level) -- the whole
                                         encoder -- every time: the only way to change the level without the kept bottleneck.
The calls of a pair are alternated inside every repeat after a warm-up round, each ended by a device synchronise, host clock; medians
and the spread (max - min) of the repeats.  Every figure is to be read against its partner OF THE SAME RUN; nothing is asserted about
times, the bytes are.  Under the untrained synthetic context model a capped file need not be smaller; if the file of level 0 is not the
smaller one, step 3 takes a context model whose last layer is a constant table with a cheap fill symbol (as the budget tests do) and
says so in `budget_weights`.  Prints one JSON line; --out writes it.

    python tools/codec_cap_timing.py [--repeats 7] [--out profiles/codec_cap_timing.json]
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
LAUNCHES = 50
LAST_LAYER = 'probclass3d/logits/conv3d_conv2_mask'


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
    wts = W.synthetic_weights(ae_cfg, pc_cfg)
    tile = (TILE // 8, TILE // 8)
    c = codec.Codec(ae_cfg, pc_cfg, wts, dev, tile=tile)
    img = np.ascontiguousarray(W.synthetic_image((1, 3, 512, 768), 'natural', seed=4)[0].transpose(1, 2, 0))
    levels = codec.cap_levels(c.C)

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

    res = {'image': '512x768 synthetic natural, seed 4', 'tile': TILE, 'repeats': flags.repeats, 'weights': 'synthetic',
           'device': torch.cuda.get_device_name(0)}

    # 1. the cap that caps nothing
    def same(got):
        assert got['compress_plain'] == got['compress_cap_inf']
    res.update(alternate([('compress_plain', lambda: c.compress(img)), ('compress_cap_inf', lambda: c.compress(img, cap=float('inf')))], same))
    res['file_bytes'] = len(c.compress(img))
    res['cap_inf_over_plain'] = round(res['compress_cap_inf']['median_ms'] / res['compress_plain']['median_ms'], 4)

    # 2. a level from the kept bottleneck
    x, _ = c._image_tensor(img)
    res.update(alternate([('encode_plain', lambda: c.ae.encode(x, is_training=False)),
                          ('encode_keep_bottleneck', lambda: c.ae.encode_capped(x, None, keep_bottleneck=True))]))
    _, bott = c.ae.encode_capped(x, None, keep_bottleneck=True)
    h, w = int(bott.shape[2]), int(bott.shape[3])
    caps = {T: torch.as_tensor(levels[np.linspace(16, 256, T).astype(int)]).to(dev)[None, :, None, None].expand(1, T, h, w).contiguous() for T in (1, 16)}

    def launches(T, hard):
        def fn():
            for _ in range(LAUNCHES):
                out = c.ae.requantize(bott, caps[T], hard_only=hard)
            return out
        return fn
    rq = alternate([('T{}_{}'.format(T, 'hard' if hard else 'all'), launches(T, hard)) for T in (1, 16) for hard in (False, True)])
    res['requantize'] = {'launches_per_window': LAUNCHES, 'bottleneck_shape': list(bott.shape)}
    for name, s in rq.items():
        res['requantize'][name] = dict(s, per_launch_us=round(1e3 * s['median_ms'] / LAUNCHES, 2),
                                       per_level_us=round(1e3 * s['median_ms'] / LAUNCHES / int(name[1:].split('_')[0]), 2))

    # 3. a byte budget
    s0, sC = len(c.compress(img, cap=0)), len(c.compress(img))
    cb, res['budget_weights'] = c, 'synthetic'
    if not s0 < sC:
        wb = dict(wts)
        wb[LAST_LAYER + '/weights'] = np.zeros_like(wts[LAST_LAYER + '/weights'])
        bias = np.ones(ae_cfg.num_centers, np.float32)
        bias[codec.fill_symbol(wts['autoencoder/encoder/centers'])] = 9.0
        wb[LAST_LAYER + '/biases'] = bias
        cb = codec.Codec(ae_cfg, pc_cfg, wb, dev, tile=tile)
        res['budget_weights'] = ('synthetic, the last context-model layer a constant table with a cheap fill symbol (with the synthetic context model '
                                 'the file of level 0 has {} bytes, the uncapped one {})'.format(s0, sC))
        s0, sC = len(cb.compress(img, cap=0)), len(cb.compress(img))
    assert s0 < sC, (s0, sC)
    budget = (s0 + sC) // 2

    def bisection():
        """9 codings: level C, then 8 halvings, every one a whole compress"""
        size = lambda k: len(cb.compress(img, cap=levels[k]))
        if size(256) <= budget:
            return 256
        lo, hi = 0, 256
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if size(mid) <= budget else (lo, mid)
        return lo

    def agree(got):
        data, level, probes = got['compress_to_budget']
        assert len(data) <= budget and data == cb.compress(img, cap=level)
        res['budget'] = {'bytes_level_0': s0, 'bytes_level_C': sC, 'budget_bytes': budget, 'file_bytes': len(data), 'level': level,
                         'real_codings': probes, 'bisection_codings': 9, 'bisection_level': float(levels[got['bisection_9_compress']])}
    res.update(alternate([('compress_to_budget', lambda: cb.compress_to_budget(img, budget)), ('bisection_9_compress', bisection)], agree))
    res['budget_over_bisection'] = round(res['compress_to_budget']['median_ms'] / res['bisection_9_compress']['median_ms'], 4)
    line = json.dumps(res)
    print(line)
    if flags.out:
        with open(flags.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
