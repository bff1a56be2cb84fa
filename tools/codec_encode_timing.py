"""Range-encoder timing on one Kodak-sized symbol volume (32 x 64 x 96 = 196,608 symbols): PredictionNetwork.encode_stream (tables
and coder on the device, only the stream copied back) against the host path (get_all: every table to the host, then
arithmetic_coding.encode_sequence), alternated, each call ended by a device synchronise.  Prints one JSON line; --out writes it.

    python tools/codec_encode_timing.py [--repeats 5] [--out profiles/codec_encode_timing.json] [--device_only]
"""
import argparse
import io
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--out')
    p.add_argument('--device_only', action='store_const', const=True, help='only the device encoder (for a kernel trace)')
    flags = p.parse_args()
    from imgcomp_cvpr_amd import arithmetic_coding as ac, autoencoder, codec, config_parser as cp, probclass, weights as W
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda:0')
    ae_cfg, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc_cfg, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    wts = W.synthetic_weights(ae_cfg, pc_cfg)
    c = codec.Codec(ae_cfg, pc_cfg, wts, dev)
    x = torch.as_tensor(W.synthetic_image((1, 3, 512, 768), 'natural', seed=4)).float().to(dev)
    sym_dev = c.ae.encode(x, is_training=False).symbols[0]
    sym = sym_dev.cpu().numpy()

    def device_path():
        out = c.pred.encode_stream(sym_dev)
        torch.cuda.synchronize()
        return out[0]

    def host_path():
        out = c._host_encode_stream(sym)
        torch.cuda.synchronize()
        return out[0]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        return time.perf_counter() - t0, r

    for _ in range(2):
        a = device_path()
    if flags.device_only:
        for _ in range(flags.repeats):
            device_path()
        print(json.dumps({'device_only': True, 'bytes': len(a)}))
        return
    b = host_path()
    assert a == b, 'streams differ'
    td, th = [], []
    for _ in range(flags.repeats):
        td.append(timed(device_path)[0])
        th.append(timed(host_path)[0])
    # the image to container bytes, end to end, with either encoder
    img = np.ascontiguousarray(W.synthetic_image((1, 3, 512, 768), 'natural', seed=4)[0].transpose(1, 2, 0))
    tc = {}
    for name, flag in (('device', True), ('host', False)):
        c.device_encode = flag
        c.compress(img)
        tc[name] = [timed(lambda: c.compress(img))[0] for _ in range(flags.repeats)]
    data = c.compress(img)
    c.decompress(data)
    tdec = [timed(lambda: c.decompress(data))[0] for _ in range(3)]
    ms = lambda v: [round(1e3 * t, 3) for t in v]
    res = {'symbols': int(sym.size), 'stream_bytes': len(a), 'repeats': flags.repeats,
           'encode_stream_ms': ms(td), 'host_get_all_plus_encode_sequence_ms': ms(th),
           'encode_stream_median_ms': round(1e3 * float(np.median(td)), 3), 'host_median_ms': round(1e3 * float(np.median(th)), 3),
           'compress_512x768_device_encoder_ms': ms(tc['device']), 'compress_512x768_host_encoder_ms': ms(tc['host']),
           'decompress_512x768_ms': ms(tdec), 'device': torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if flags.out:
        with open(flags.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
