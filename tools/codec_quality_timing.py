"""The quality axis of the codec, on the 512 x 768 synthetic natural image of the other codec timings with --tile 128, in ONE run:
  1. measure / decompress_host_metrics     Codec.measure(img, data) against decompress(data) and the host's NumPy PSNR and MS-SSIM,
                                           which is what a caller had before; the figures agree to the device metrics' tolerance.
  2. rd_curve_17 / loop_17                 Codec.rd_curve at the 17 default levels against the loop of compress(img, cap=level),
                                           decompress and val_metrics_device per level -- the whole encoder, a host round trip of the
                                           picture and an upload per level: the only way without rd_curve.  The rows are equal.
  3. compress_to_quality / rd_curve_257    compress_to_quality at a PSNR halfway between level 0's and the uncapped file's, against
                                           rd_curve over all 257 levels of the grid and a scan of the table: the only way to a level
                                           that meets a target without the search.
  4. transcode_to_quality / loop_transcode transcode_to_quality at a PSNR between those of the integer levels, against C + 1 calls of
                                           transcode, decompress and val_metrics_device against decompress(source).
The calls of a pair are alternated inside every repeat after a warm-up round, each ended by a device synchronise, host clock; medians
and the spread (max - min) of the repeats.  Every figure is to be read against its partner OF THE SAME RUN; nothing is asserted about
times, the results are.  With synthetic weights the quality figures themselves mean nothing.  Prints one JSON line; --out writes it.

    python tools/codec_quality_timing.py [--repeats 7] [--out profiles/codec_quality_timing.json]
"""
import argparse
import json
import math
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
    from imgcomp_cvpr_amd import codec, config_parser as cp, metrics, weights as W
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda:0')
    ae_cfg, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc_cfg, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    wts = W.synthetic_weights(ae_cfg, pc_cfg)
    c = codec.Codec(ae_cfg, pc_cfg, wts, dev, tile=(TILE // 8, TILE // 8))
    img = np.ascontiguousarray(W.synthetic_image((1, 3, 512, 768), 'natural', seed=4)[0].transpose(1, 2, 0))
    H, W_ = img.shape[:2]

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

    def ratio(a, b):
        return round(res[a]['median_ms'] / res[b]['median_ms'], 4)

    up = lambda pic: torch.as_tensor(np.ascontiguousarray(np.transpose(pic, (2, 0, 1)))[None]).to(dev)
    nchw = lambda pic: np.transpose(pic, (2, 0, 1))[None]

    def device_measure(orig, data):
        """what a caller had for a table row: the picture to the host, back up, the device metrics"""
        scales, mse = metrics.val_metrics_device(up(orig), up(c.decompress(data)))
        return codec.measure_from_values(scales.tolist() + [float(mse)], len(data), H * W_)

    res = {'image': '512x768 synthetic natural, seed 4', 'tile': TILE, 'repeats': flags.repeats, 'weights': 'synthetic',
           'device': torch.cuda.get_device_name(0)}

    # 1. one file
    data = c.compress(img)

    def host_metrics():
        dec = c.decompress(data)
        return float(metrics.psnr_uint8(img, dec)), float(metrics.msssim_nchw_uint8(nchw(img), nchw(dec)))

    def close(got):
        m, (psnr, msssim) = got['measure'], got['decompress_host_metrics']
        assert abs(m.psnr - psnr) <= 1e-4 and abs(m.ms_ssim - msssim) <= 1e-6, (m, psnr, msssim)
        res['file'] = dict(m._asdict())
    res.update(alternate([('measure', lambda: c.measure(img, data)), ('decompress_host_metrics', host_metrics)], close))
    res['measure_over_host'] = ratio('measure', 'decompress_host_metrics')

    # 2. the table at 17 levels
    levels17 = codec.rd_levels(c.C)

    def same_rows(got):
        assert got['rd_curve_17'] == list(zip(levels17, got['loop_17']))
        res['rd_rows'] = [dict(m._asdict(), level=lv) for lv, m in got['rd_curve_17']]
    res.update(alternate([('rd_curve_17', lambda: c.rd_curve(img)),
                          ('loop_17', lambda: [device_measure(img, c.compress(img, cap=lv)) for lv in levels17])], same_rows))
    res['rd_curve_over_loop'] = ratio('rd_curve_17', 'loop_17')

    # 3. a level for a PSNR
    m0, mC = c.measure(img, c.compress(img, cap=0)), c.measure(img, data)
    target = 0.5 * (m0.psnr + mC.psnr)
    levels257 = codec.rd_levels(c.C, codec.CAP_STEPS)

    def scan():
        """the first adjacent pair (misses, meets) from the top of the whole table, or level 0: a level with the search's contract"""
        rows = c.rd_curve(img, levels=levels257)
        if rows[0][1].psnr >= target:
            return rows[0]
        return next(rows[k] for k in range(len(rows) - 1, 0, -1) if rows[k][1].psnr >= target and not rows[k - 1][1].psnr >= target)

    def contract(got):
        d, level, m, probes = got['compress_to_quality']
        assert d == c.compress(img, cap=level) and m == c.measure(img, d) and m.psnr >= target
        res['quality'] = {'psnr_level_0': m0.psnr, 'psnr_uncapped': mC.psnr, 'target_psnr': target, 'level': level, 'probes': probes,
                          'file': dict(m._asdict()), 'scan_level': got['rd_curve_257'][0]}
    res.update(alternate([('compress_to_quality', lambda: c.compress_to_quality(img, psnr=target)), ('rd_curve_257', scan)], contract))
    res['quality_over_rd_curve_257'] = ratio('compress_to_quality', 'rd_curve_257')

    # 4. a file lowered to a PSNR against its own picture
    ref = c.decompress(data)
    per_level = [device_measure(ref, c.transcode(data, cap=K)).psnr for K in range(c.C + 1)]
    finite = sorted(v for v in per_level if math.isfinite(v))
    t_target = finite[len(finite) // 2]

    def loop_transcode():
        rows = [device_measure(ref, c.transcode(data, cap=K)) for K in range(c.C + 1)]
        return next(K for K in range(c.C, -1, -1) if rows[K].psnr >= t_target and (K == 0 or not rows[K - 1].psnr >= t_target))

    def t_contract(got):
        out, K, m, probes = got['transcode_to_quality']
        assert out == c.transcode(data, cap=K) and m == c.measure(ref, out) and m.psnr >= t_target
        res['transcode'] = {'psnr_per_level': [v if math.isfinite(v) else None for v in per_level], 'target_psnr': t_target, 'level': K, 'probes': probes, 'file': dict(m._asdict()),
                            'loop_level': got['loop_transcode'], 'loop_calls': c.C + 1}
    res.update(alternate([('transcode_to_quality', lambda: c.transcode_to_quality(data, psnr=t_target)), ('loop_transcode', loop_transcode)], t_contract))
    res['transcode_quality_over_loop'] = ratio('transcode_to_quality', 'loop_transcode')
    line = json.dumps(res)
    print(line)
    if flags.out:
        with open(flags.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
