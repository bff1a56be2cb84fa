"""Wavefront tiles (container format 5), the parts that need no GPU: the schedule derived from the context model's masks, the
coding order of a tile, the host coder over permuted tables, the container and its two readers, verify, the option checks."""
import argparse
import struct
import zlib

import numpy as np
import pytest

from tests import codec_cases as cc

SHAPES = [(32, 16, 16), (32, 1, 1), (32, 1, 7), (5, 3, 16), (32, 16, 9)]
# What the order may cost per tile stream, in bytes, against the raster coding of the same tile (test_host_coder_* has the
# measurement and the reasoning); tests/test_gpu_codec_wavefront.py holds the device streams to the same figure.
LENGTH_MARGIN_PER_STREAM = 4


def _masks():
    from imgcomp_cvpr_amd import probclass, config_parser as cp
    pc_cfg, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    cls = probclass.get_network_cls(pc_cfg)
    net = cls(pc_cfg, num_centers=6)
    return (net.create_first_mask(), net.create_other_mask()), cls.get_num_layers(), net


# ---- the schedule -------------------------------------------------------------------------------------------------------------

def test_schedule_from_the_models_own_masks():
    from imgcomp_cvpr_amd import codec
    masks, layers, net = _masks()
    assert layers == 4
    deps = codec.wavefront_dependencies(masks, layers)
    assert len(deps) == 294 and (0, 0, 0) not in deps
    assert all(dw + 2 * dh + 4 * dd < 0 for dd, dh, dw in deps)
    assert codec.wavefront_is_valid(masks, layers, 2, 4) and codec.WAVEFRONT_COEFFS == (2, 4)
    for b in range(13):
        assert not codec.wavefront_is_valid(masks, layers, 1, b), b
    assert not codec.wavefront_is_valid(masks, layers, 2, 3)
    # the receptive field is the 5 x 9 x 9 context, and one layer alone is its mask
    assert min(d[0] for d in deps) == -4 and max(abs(d[1]) for d in deps) == 4 and max(abs(d[2]) for d in deps) == 4
    assert len(codec.wavefront_dependencies(masks, 1)) == 13
    assert codec.wavefront_coeffs(net) == (2, 4)


def test_coeffs_refuse_other_models():
    from imgcomp_cvpr_amd import codec
    masks, layers, net = _masks()

    class Wide(object):                                  # the same masks, a width the wavefront decoder does not cover
        _k = 64
        create_first_mask, create_other_mask = net.create_first_mask, net.create_other_mask
        get_num_layers = staticmethod(lambda: 4)

    with pytest.raises(ValueError, match='k = 24, this one has k = 64'):
        codec.wavefront_coeffs(Wide())

    class Unmasked(Wide):                                # a first layer that sees the current position and the ones behind it
        _k = 24
        create_first_mask = staticmethod(lambda: np.ones((2, 3, 3, 1, 1), np.float32))

    with pytest.raises(ValueError, match='does not order the dependencies'):
        codec.wavefront_coeffs(Unmasked())


@pytest.mark.parametrize('shape', SHAPES)
def test_wavefront_order(shape):
    from imgcomp_cvpr_amd import codec
    C, th, tw = shape
    order = codec.wavefront_order(C, th, tw)
    n = C * th * tw
    assert order.dtype == np.int64 and order.shape == (n,) and order[0] == 0
    assert np.array_equal(np.sort(order), np.arange(n))                   # a permutation
    c, y, x = np.unravel_index(order, shape)
    T = x + 2 * y + 4 * c
    assert (np.diff(T) >= 0).all()
    same = np.diff(T) == 0
    assert (np.diff(order)[same] > 0).all()                               # inside a front: (c, y, x), i.e. ascending raster index
    # every dependency that lies inside the tile comes earlier
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    rank = rank.reshape(shape)
    masks, layers, _ = _masks()
    cc_, yy, xx = np.meshgrid(np.arange(C), np.arange(th), np.arange(tw), indexing='ij')
    checked = 0
    for dc, dy, dx in codec.wavefront_dependencies(masks, layers):
        c2, y2, x2 = cc_ + dc, yy + dy, xx + dx
        inside = (c2 >= 0) & (c2 < C) & (y2 >= 0) & (y2 < th) & (x2 >= 0) & (x2 < tw)
        assert (rank[c2[inside], y2[inside], x2[inside]] < rank[inside]).all(), (dc, dy, dx)
        checked += int(inside.sum())
    assert checked > 0 or n == 1 or (th, tw) == (1, 1)
    with pytest.raises(ValueError, match='at least 1'):
        codec.wavefront_order(C, 0, tw)


def test_front_sizes_of_the_issue():
    from imgcomp_cvpr_amd import codec
    for shape, fronts, largest in (((32, 16, 16), 170, 64), ((32, 32, 32), 218, 256)):
        c, y, x = np.unravel_index(codec.wavefront_order(*shape), shape)
        counts = np.bincount(x + 2 * y + 4 * c)
        assert len(counts) == fronts and counts.max() == largest and counts.min() >= 1


# ---- the host coder over permuted tables --------------------------------------------------------------------------------------

def test_host_coder_over_permuted_tables_round_trip_and_length():
    """Symbols and tables permuted by wavefront_order, coded by the host coder and decoded back to the volume.  The ideal code
    length does not depend on the order (the same table codes the same symbol); what differs is the coder's rounding and where
    its last bits fall.  Measured here for the five shapes x three table kinds below (logits = relu(gain * N(0,1)), gain 1, 3, 12;
    symbols drawn from their own tables): wavefront minus raster = -1 .. +1 byte per stream (13 of 15 cases 0).  The bound is
    LENGTH_MARGIN_PER_STREAM = 4 bytes per stream: the termination costs at most two bytes either way, and the rest is margin."""
    from imgcomp_cvpr_amd import codec
    worst = 0
    for shape in SHAPES:
        for seed, gain in ((1, 1.0), (2, 3.0), (3, 12.0)):
            rs = np.random.RandomState(seed)
            n = int(np.prod(shape))
            tabs = cc.softmax_tables(np.maximum(rs.randn(n, 6) * gain, 0).astype(np.float32))
            cdf = np.cumsum(tabs / tabs.sum(axis=1, keepdims=True), axis=1)
            sym = np.minimum((rs.rand(n, 1) > cdf).sum(axis=1), 5).astype(np.int64)
            order = codec.wavefront_order(*shape)
            raster, _ = cc.host_encode(sym[1:], tabs[1:])
            wave, _ = cc.host_encode(sym[order][1:], tabs[order][1:])
            back = np.empty(n, np.int64)
            back[order] = [int(sym[0])] + cc.host_decode(wave, tabs[order][1:])
            assert np.array_equal(back, sym), (shape, seed)
            # the word-level model of the device encoder writes the same bytes for the permuted sequence
            assert cc.model_encode(*cc.triples(sym[order][1:], tabs[order][1:]))[0] == wave
            diff = len(wave) - len(raster)
            print('{} gain {}: raster {} bytes, wavefront {} bytes ({:+d})'.format(shape, gain, len(raster), len(wave), diff))
            worst = max(worst, abs(diff))
            assert abs(diff) <= LENGTH_MARGIN_PER_STREAM, (shape, seed, diff)
    print('largest difference: {} bytes per stream'.format(worst))


# ---- the decoder's schedule, restated ------------------------------------------------------------------------------------------

def _cdiv_pos(n, k):
    return 0 if n <= 0 else (n + k - 1) // k


def _front(S, ND, NI, NJ):
    """pc_front / pc_front_voxel of csrc/pc_decode.hip: the voxels of a box with j + 2 i + 4 d == S, in candidate order"""
    d_lo, d_hi = _cdiv_pos(S - (NJ - 1) - 2 * (NI - 1), 4), min(ND - 1, S >> 2)
    nd, iw, out = (0 if S < 0 else max(d_hi - d_lo + 1, 0)), min(NI, (NJ + 1) >> 1), []
    for e in range(nd * iw):
        dd, ii = divmod(e, iw)
        d = d_lo + dd
        R = S - 4 * d
        i = _cdiv_pos(R - (NJ - 1), 2) + ii
        j = R - 2 * i
        if i < NI and j >= 0:
            assert 0 <= d < ND and 0 <= j < NJ
            out.append((d, i, j))
    return out


@pytest.mark.parametrize('shape', [(5, 3, 16), (32, 1, 1), (6, 5, 8), (3, 4, 9), (2, 7, 1), (32, 16, 16)])
def test_decoder_schedule_writes_once_before_every_read(shape):
    """the four phases of pc_dec_wave_body per step T, on flags instead of values: every tap a phase reads lies inside its array
    and was written by an earlier phase or step, nothing is written twice, and the symbols come out in wavefront_order"""
    from imgcomp_cvpr_amd import codec
    C, h, w = shape
    other = [(0, a, b) for a in range(3) for b in range(3)] + [(1, 0, 0), (1, 0, 1), (1, 0, 2), (1, 1, 0), (1, 1, 1)]
    first = other[:13]
    V = np.ones((C + 4, h + 8, w + 8), bool)
    V[4:, 4:h + 4, 4:w + 4] = False
    A0, A1, A2 = np.zeros((C + 3, h + 6, w + 6), bool), np.zeros((C + 2, h + 4, w + 4), bool), np.zeros((C + 1, h + 2, w + 2), bool)
    order, steps = [], 0
    for T in range(7, (w + 3) + 2 * (h + 3) + 4 * (C + 3) + 1):
        steps += 1
        for out, src, taps, back in ((A0, V, first, 7), (A1, A0, other, 14), (A2, A1, other, 21)):
            todo = _front(T - back, *out.shape)
            for d, i, j in todo:
                assert not out[d, i, j] and all(src[d + a, i + b, j + c] for a, b, c in taps), (T, d, i, j)
                assert out is not A2 or A0[d + 2, i + 2, j + 2]
            for v in todo:
                out[v] = True
        todo = _front(T - 28, C, h, w)
        for c, y, x in todo:
            assert not V[c + 4, y + 4, x + 4] and all(A2[c + a, y + b, x + k] for a, b, k in other), (T, c, y, x)
        for c, y, x in todo:
            V[c + 4, y + 4, x + 4] = True
            order.append((c * h + y) * w + x)
    assert V.all() and np.array_equal(np.array(order), codec.wavefront_order(C, h, w))
    if shape == (32, 16, 16):
        assert steps == 191


# ---- the container ------------------------------------------------------------------------------------------------------------

def _fields(streams=(b'\x12\x34', b'', b'\x80', b'\x01\x02\x03', b'\xff', b'\x10\x20')):
    streams = list(streams) + [bytes([i + 1]) * (i + 1) for i in range(9 - len(streams))]
    return dict(ae_name='cvpr/low', pc_name='cvpr/res_shallow', H=61, W=93, C=32, h=8, w=12, L=6, resolution=1e9,
                fingerprint=0xdeadbeef, th=3, tw=5, first_syms=[t % 6 for t in range(9)], streams=streams)


def _resealed(body):
    return bytes(body) + struct.pack('<I', zlib.crc32(bytes(body)) & 0xffffffff)


def _offsets(f):
    th = 6 + 2 + len(f['ae_name']) + 2 + len(f['pc_name']) + 8 + 10 + 2 + 8 + 4
    table = th + 4 + 4
    plen = table + 10 * len(f['streams'])
    return th, th + 4, table, plen, plen + 8, plen + 12


def test_wavefront_container_round_trip():
    from imgcomp_cvpr_amd import codec
    f = _fields()
    data, v4 = codec.build_wavefront_container(**f), codec.build_checked_container(**f)
    assert codec.FORMAT_VERSION_WAVEFRONT == 5 and len(data) == len(v4)
    c = codec.parse_container(data)
    assert isinstance(c, codec.WavefrontContainer) and c.version == 5 and isinstance(c, codec._TILED)
    assert not isinstance(c, codec.CheckedContainer) and codec.WavefrontContainer._fields == codec.CheckedContainer._fields
    for k, v in f.items():
        assert getattr(c, k) == v, k
    assert c.stream_crcs == [zlib.crc32(b) & 0xffffffff for b in f['streams']] and c.payload == b''.join(f['streams'])
    # the layout of format 4: only the version word and the two CRCs that cover it differ
    th, nt, table, plen, hcrc, payload = _offsets(f)
    assert struct.unpack_from('<H', data, 4)[0] == 5
    assert data[6:hcrc] == v4[6:hcrc] and data[payload:-4] == v4[payload:-4]
    assert struct.unpack_from('<I', data, hcrc)[0] == zlib.crc32(data[:hcrc]) and struct.unpack('<I', data[-4:])[0] == zlib.crc32(data[:-4])
    s, damage, ok = codec.parse_salvage(data)
    assert s == c and isinstance(s, codec.WavefrontContainer) and damage == [] and ok is True
    assert codec.verify_file(data) == (True, 'ok (format 5, {} bytes)'.format(len(data)))
    assert codec._compress_line('a.icf', data, 61 * 93).endswith(', 9 tiles')


def test_wavefront_container_refusals():
    from imgcomp_cvpr_amd import codec
    f = _fields()
    good = codec.build_wavefront_container(**f)
    th, nt, table, plen, hcrc, payload = _offsets(f)
    for pos in range(len(good)):                          # any flipped bit
        bad = bytearray(good)
        bad[pos] ^= 0x04
        with pytest.raises(ValueError, match='magic|version|CRC|truncated'):
            codec.parse_container(bytes(bad))
    for n in range(len(good)):                            # any truncation
        with pytest.raises(ValueError, match='magic|version|CRC|truncated'):
            codec.parse_container(good[:n])
    body = bytearray(good[:-4])                           # under a recomputed file CRC: the inner CRCs name the damage
    body[table + 7] ^= 0x01                               # (inside the CRC word of tile 0 in the table)
    with pytest.raises(ValueError, match='header CRC mismatch'):
        codec.parse_container(_resealed(body))
    body = bytearray(good[:-4])
    body[payload + 2] ^= 0x20                             # the third payload byte belongs to tile 2
    with pytest.raises(ValueError, match='stream CRC mismatch in tile 2:'):
        codec.parse_container(_resealed(body))
    body = bytearray(good[:-4])                           # a tile count that is not the grid's, under correct CRCs
    struct.pack_into('<I', body, nt, 8)
    struct.pack_into('<I', body, hcrc, zlib.crc32(bytes(body[:hcrc])) & 0xffffffff)
    with pytest.raises(ValueError, match='tile count 8 does not equal the 9 tiles'):
        codec.parse_container(_resealed(body))
    with pytest.raises(ValueError, match='header damaged'):
        codec.parse_salvage(_resealed(body))


def test_version_3_is_still_refused_with_the_pinned_sentence():
    from imgcomp_cvpr_amd import codec
    body = bytearray(codec.build_wavefront_container(**_fields())[:-4])
    body[4:6] = struct.pack('<H', 3)
    with pytest.raises(ValueError, match=r'unsupported format version 3 \(this codec reads versions 1, 2 and 4\) and the wavefront version 5'):
        codec.parse_container(_resealed(body))
    with pytest.raises(ValueError, match='unsupported format version 3'):
        codec.parse_salvage(_resealed(body))
    ok, text = codec.verify_file(_resealed(body))
    assert not ok and 'unsupported format version 3' in text


def test_verify_and_salvage_reader_on_damaged_format_5():
    from imgcomp_cvpr_amd import codec
    f = _fields()
    good = codec.build_wavefront_container(**f)
    th, nt, table, plen, hcrc, payload = _offsets(f)
    n = len(b''.join(f['streams']))
    bad = bytearray(good)
    bad[payload] ^= 0x01                                   # tile 0
    bad[payload + 2] ^= 0x80                               # tile 2
    c, damage, ok = codec.parse_salvage(bytes(bad))
    assert isinstance(c, codec.WavefrontContainer) and damage == [(0, 'crc'), (2, 'crc')] and ok is False
    assert c.streams[0] is None and c.streams[2] is None and c.streams[1] == b'' and c.streams[3] == f['streams'][3]
    assert codec.verify_file(bytes(bad)) == (False, '2 of 9 tiles damaged: tile 0 (crc), tile 2 (crc)')
    # cut inside the last stream: that tile is truncated, the file CRC is gone
    cut = good[:payload + n - 3]
    c, damage, ok = codec.parse_salvage(cut)
    assert damage == [(8, 'truncated')] and ok is False and c.streams[8] is None and c.streams[7] == f['streams'][7]
    assert codec.verify_file(cut) == (False, '1 of 9 tiles damaged: tile 8 (truncated)')
    # the same damage in the format-4 file of the same fields names the same tiles
    bad4 = bytearray(codec.build_checked_container(**f))
    bad4[payload] ^= 0x01
    bad4[payload + 2] ^= 0x80
    assert codec.parse_salvage(bytes(bad4))[1] == [(0, 'crc'), (2, 'crc')]
    # a damaged header: nothing is believed
    bad = bytearray(good)
    bad[table + 1] ^= 0x01
    with pytest.raises(ValueError, match='header damaged: nothing can be recovered'):
        codec.parse_salvage(bytes(bad))
    ok, text = codec.verify_file(bytes(bad))
    assert not ok and 'header damaged' in text


# ---- the command line ---------------------------------------------------------------------------------------------------------

def test_wavefront_option_checks(tmp_path, capsys):
    from imgcomp_cvpr_amd import codec
    src, dst = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    (src / 'a.png').write_bytes(b'x')
    for args, msg in ((['compress', str(src / 'a.png'), str(dst), '--wavefront'], '--wavefront needs --tile'),
                      (['compress-dir', str(src), str(dst), '--wavefront'], '--wavefront needs --tile'),
                      (['decompress', str(src / 'a.png'), str(dst), '--wavefront', '--tile', '128'], '--wavefront belongs to compress'),
                      (['decompress', str(src / 'a.png'), str(dst), '--wavefront'], '--wavefront belongs to compress'),
                      (['decompress-dir', str(src), str(dst), '--wavefront'], '--wavefront belongs to compress')):
        assert codec.main(args + ['--device', 'no-such-device']) == 2, args
        assert msg in capsys.readouterr().err, args
    assert not dst.exists()
    with pytest.raises(SystemExit) as e:                  # verify takes paths only
        codec.main(['verify', str(src), '--wavefront'])
    assert e.value.code == 2
    capsys.readouterr()
    flags = argparse.Namespace(command='compress-dir', input=str(src), output=str(dst), tile=None, batch=3, checked=False, salvage=False,
                               wavefront=True)
    with pytest.raises(ValueError, match='--wavefront needs --tile'):
        codec.check_option_args(flags)
    with pytest.raises(ValueError, match='--wavefront needs --tile'):
        codec.check_dir_args(flags, 8)
    flags.tile = 128
    codec.check_option_args(flags)
    assert codec.check_dir_args(flags, 8) == ([(str(src / 'a.png'), str(dst / 'a.icf'))], (16, 16))
    flags.checked = True                                  # accepted, redundant
    codec.check_option_args(flags)
    flags.checked, flags.command = False, 'verify'
    with pytest.raises(ValueError, match='--wavefront belongs to compress'):
        codec.check_option_args(flags)
