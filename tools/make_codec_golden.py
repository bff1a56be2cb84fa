#!/usr/bin/env python
"""Writes tests/golden/codec_files.npz on a machine with the device: for every model x volume of tests/codec_golden_cases.py the
symbols, the sha256 of the context model's logits, the frequency tables (raw for codec_golden_cases.RAW_TABLES, their sha256 for
all) and the bytes of the file of every format the model supports, plus SHARP, the model fingerprints and the HIP version.

REGENERATING THE FIXTURE IS A FILE-FORMAT BREAK: its bytes are what files written by earlier builds hold ("What a
file depends on").  Run it once per intended break and say so in the commit.

    python tools/make_codec_golden.py [--out PATH] [--force] [--find-sharp]

Everything is computed twice and must agree byte for byte; every file is decoded back to its symbols and reproduced by the host
coder from the tables; the conditions that define SHARP are asserted (and that SHARP / 2 misses them).  The npz is written with
fixed time stamps, so the same records give the same file.  --find-sharp only prints the shares per power of two."""
import argparse
import io
import os
import sys
import zipfile
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import codec_golden_cases as G                    # noqa: E402


def scaled_tables(c, logits, scale):
    """the tables of `scale` times the logits, by the library's table pass"""
    import torch
    from imgcomp_cvpr_amd import _lib
    lg = (logits * scale).reshape(-1, c.L).contiguous()
    freqs = torch.empty(lg.shape, dtype=torch.int64, device=lg.device)
    _lib.check(_lib.lib.ic_pc_logits_to_freqs_f32(_lib.ptr(lg), lg.shape[0], c.L, G.RESOLUTION, _lib.ptr(freqs), None,
                                                  _lib.current_stream(lg.device)), 'ic_pc_logits_to_freqs_f32')
    return freqs.cpu().numpy()


def meets(shares):
    return shares[0] >= G.PEAK_SHARE and shares[1] >= 1


def find_sharp(codecs, iid):
    """sharp's logits are SHARP times plain's exactly, so the sweep scales plain's"""
    import torch
    plain = G.device_logits(codecs['plain'], iid)
    assert torch.equal(G.device_logits(codecs['sharp'], iid), plain * G.SHARP), 'the logits of sharp are not SHARP times those of plain'
    found = None
    for k in range(0, 11):
        shares = G.sharp_shares(scaled_tables(codecs['plain'], plain, float(2 ** k)))
        found = 2 ** k if found is None and meets(shares) else found
        print('SHARP = {:5d}: peaked positions {:.4f}, entries at the floor {}{}'.format(2 ** k, shares[0], shares[1], '   <- meets both' if meets(shares) else ''))
    print('the smallest power of two that meets both: {}'.format(found))
    return found


def record(codecs, volumes):
    out = OrderedDict()
    import torch
    out['meta_sharp'] = np.float64(G.SHARP)
    out['meta_rocm'] = np.array(str(torch.version.hip))
    for m, c in codecs.items():
        out['meta_fingerprint_' + m] = np.uint32(c.fingerprint)
    for m, v in G.PAIRS:
        c, sym = codecs[m], volumes[v]
        tables, tile_tables = G.device_tables(c, sym), G.device_tile_tables(c, sym)
        assert 1 <= tables.min() and max(tables.max(), tile_tables.max()) <= G.RESOLUTION < 2 ** 31
        out['symbols_' + v] = sym.astype(np.uint8)
        out[G.key(m, v, 'logits_sha256')] = np.array(G.sha256(G.device_logits(c, sym).cpu().numpy(), '<f4'))
        out[G.key(m, v, 'tables_sha256')] = np.array(G.sha256(tables, '<i4'))
        out[G.key(m, v, 'tile_tables_sha256')] = np.array(G.sha256(tile_tables, '<i4'))
        if (m, v) in G.RAW_TABLES:
            out[G.key(m, v, 'tables')] = tables.astype(np.int32)
            out[G.key(m, v, 'tile_tables')] = tile_tables.astype(np.int32)
        for fmt in G.formats_of(m):
            out[G.key(m, v, 'f{}'.format(fmt))] = np.frombuffer(G.device_file(c, fmt, sym), dtype=np.uint8)
    return out


def npz_bytes(arrays):
    """np.savez_compressed with fixed time stamps: the same arrays give the same bytes"""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, 'w', zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            member = io.BytesIO()
            np.lib.format.write_array(member, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, member.getvalue())
    return buf.getvalue()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=G.PATH)
    ap.add_argument('--force', action='store_true', help='overwrite an existing fixture: a file-format break')
    ap.add_argument('--find-sharp', action='store_true', help='print the shares per power of two and stop')
    flags = ap.parse_args(argv)
    if os.path.exists(flags.out) and not flags.force and not flags.find_sharp:
        sys.exit('{} exists: regenerating it is a file-format break; --force if that is meant'.format(flags.out))
    import torch
    from imgcomp_cvpr_amd import codec
    assert torch.cuda.is_available(), 'the fixture records what the device computes'
    device = torch.device('cuda:0')
    codecs = OrderedDict((m, G.load_codec(m, device)) for m in G.MODELS)
    fill = codec.fill_symbol(G.centers(G.weights('plain')))
    volumes = OrderedDict((v, G.volume(v, fill)) for v in G.VOLUMES)
    for m, c in codecs.items():
        assert c.fingerprint == G.fingerprint(G.weights(m)) and (c.ae_name, c.pc_name) == (G.AE, G.PC_OF[m])
        assert (c.layered_refusal is None and c.wavefront_refusal is None) == (G.formats_of(m) == G.FORMATS)
    found = find_sharp(codecs, volumes['iid'])
    if flags.find_sharp:
        return
    assert found == G.SHARP, 'SHARP = {} in tests/codec_golden_cases.py, the smallest power of two that meets the conditions is {}'.format(G.SHARP, found)

    first, second = record(codecs, volumes), record(codecs, volumes)
    assert list(first) == list(second)
    for name in first:
        assert first[name].dtype == second[name].dtype and first[name].tobytes() == second[name].tobytes(), '{} differs between two runs'.format(name)

    shares = G.sharp_shares(first[G.key('sharp', 'iid', 'tables')])
    print('SHARP = {}: {:.4f} of the positions of sharp/iid hold a frequency >= {} * resolution, {} entries at the floor of 1'.format(
        G.SHARP, shares[0], G.PEAK, shares[1]))
    assert meets(shares)
    for m, v in G.PAIRS:
        c, sym = codecs[m], volumes[v]
        for fmt in G.formats_of(m):
            data = first[G.key(m, v, 'f{}'.format(fmt))].tobytes()
            decoded, _ = c.decode_symbols(data)
            assert np.array_equal(decoded, sym), '{}/{} format {} does not decode to its symbols'.format(m, v, fmt)
            if (m, v) in G.RAW_TABLES:
                host = G.host_file(m, fmt, sym, first[G.key(m, v, 'tables')], first[G.key(m, v, 'tile_tables')], c.fingerprint)
                assert host == data, '{}/{} format {}: the host coder over the recorded tables writes other bytes'.format(m, v, fmt)
        print('{}/{}: '.format(m, v) + ', '.join('format {} {} bytes'.format(f, first[G.key(m, v, 'f{}'.format(f))].size) for f in G.formats_of(m)))

    data = npz_bytes(first)
    assert len(data) <= G.MAX_BYTES, 'the fixture has {} bytes, the limit is {}'.format(len(data), G.MAX_BYTES)
    os.makedirs(os.path.dirname(os.path.abspath(flags.out)), exist_ok=True)
    with open(flags.out, 'wb') as f:
        f.write(data)
    print('wrote {}: {} bytes, HIP {}'.format(flags.out, len(data), torch.version.hip))


if __name__ == '__main__':
    main()
