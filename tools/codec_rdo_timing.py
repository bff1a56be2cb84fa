"""Rate-aware symbol choice at encode (compress --rdo): what a lambda costs in time and quality and saves in bytes on a 512 x 768
picture at --tile 128, formats 5 and 12, models `plain` and `sharp` of tests/codec_golden_cases.py, lambda over a decade ladder from
0.  Per lambda: the sweep's time (PredictionNetwork.choose_tiles_batch on the picture's z), compress with --rdo against the same
run's compress without (alternated within the repeats), file bytes, symbols that differ from the quantiser's, latent MSE, and PSNR /
MS-SSIM by Codec.measure.  Beside them the decoder call of the same file: the prediction to confirm or refute is that the sweep costs
about what the format-12 decoder call costs -- the same phases without a coder.  Medians and spread (max - min) are written to
profiles/codec_rdo_timing.json.

    python tools/codec_rdo_timing.py [--out profiles/codec_rdo_timing.json] [--repeats 5]

Synthetic weights: the byte and quality figures say nothing about a trained model; the times per front do not depend on the weights."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LADDER = (0.0, 0.001, 0.01, 0.1, 1.0)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default='profiles/codec_rdo_timing.json')
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--device', default='cuda:0')
    flags = p.parse_args()
    import torch
    from imgcomp_cvpr_amd import codec, weights as W
    from tests import codec_golden_cases as gc
    H, W_, tile = 512, 768, 128
    img = np.ascontiguousarray(W.synthetic_image((1, 3, H, W_), 'natural', seed=4)[0].transpose(1, 2, 0))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def stats(ms):
        return {'ms': [round(v, 3) for v in ms], 'median_ms': round(float(np.median(ms)), 3), 'spread_ms': round(max(ms) - min(ms), 3)}

    result = {'image': '{}x{} synthetic natural, seed 4'.format(H, W_), 'tile': tile, 'repeats': flags.repeats,
              'weights': 'synthetic (tests/codec_golden_cases.py): bytes and quality say nothing about a trained model',
              'device': torch.cuda.get_device_name(0), 'lambda_ladder': list(LADDER), 'cases': []}
    for model in ('plain', 'sharp'):
        ae_cfg, pc_cfg = gc.configs(model)
        c = codec.Codec(ae_cfg, pc_cfg, gc.weights(model), flags.device)
        cells = tile // c.factor
        centers = c.ae.get_centers_variable().detach().float()
        for fmt in (5, 12):
            c.tile, c.order, c.rans = (cells, cells), ('wavefront' if fmt == 5 else 'raster'), ('default' if fmt == 12 else None)
            enc, _ = c.encode_symbols(img)
            z = enc.z[0].contiguous()
            plain_file = c.compress(img)
            head = codec.parse_container(plain_file)
            kw = {'order': 'rans', 'lanes': head.lanes} if fmt == 12 else {'order': 'wavefront'}
            decoder = lambda: c.pred.decode_tiles_batch([(head.streams, head.first_syms, (head.C, head.h, head.w))], head.th, head.tw, want='q', **kw)
            decoder()
            c.compress(img, rdo=LADDER[1])                                     # warm-up of both paths
            case = {'model': model, 'format': fmt, 'tiles': len(head.streams), 'symbols': int(z.numel()), 'rows': []}
            dec_ms = []
            for lam in LADDER:
                times = {'sweep': [], 'compress_rdo': [], 'compress': []}
                for _ in range(flags.repeats):                                 # alternated within a repeat
                    times['sweep'].append(timed(lambda: c.pred.choose_tiles_batch([z], cells, cells, lam))[1])
                    times['compress'].append(timed(lambda: c.compress(img))[1])
                    times['compress_rdo'].append(timed(lambda: c.compress(img, rdo=lam))[1])
                    dec_ms.append(timed(decoder)[1])
                data, changed, count = c.compress_counting(img, lam)
                sym = torch.as_tensor(c.decode_symbols(data)[0]).to(c.device)
                m = c.measure(img, data)
                row = {'lambda': lam, 'file_bytes': len(data), 'changed_symbols': changed,
                       'latent_mse': float(((z.double() - centers[sym].double()) ** 2).mean()),
                       'psnr': m.psnr, 'ms_ssim': m.ms_ssim, 'bpp': m.bpp}
                for what, ms in times.items():
                    row[what] = stats(ms)
                case['rows'].append(row)
                print('{} format {} lambda {:g}: sweep {:.2f} ms, compress {:.2f} -> {:.2f} ms, {} -> {} bytes, {} of {} symbols changed, '
                      'PSNR {:.3f}, MS-SSIM {:.5f}'.format(model, fmt, lam, row['sweep']['median_ms'], row['compress']['median_ms'],
                                                            row['compress_rdo']['median_ms'], len(plain_file), len(data), changed, count,
                                                            m.psnr, m.ms_ssim), flush=True)
            case['decoder_call_same_file'] = stats(dec_ms)
            print('{} format {}: decoder call of the file without --rdo {:.2f} ms'.format(model, fmt, case['decoder_call_same_file']['median_ms']), flush=True)
            result['cases'].append(case)
    os.makedirs(os.path.dirname(os.path.abspath(flags.out)), exist_ok=True)
    with open(flags.out, 'w') as f:
        json.dump(result, f)
        f.write('\n')


if __name__ == '__main__':
    main()
