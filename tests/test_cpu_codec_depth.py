"""Depth-mapped tiles (container format 10) on the host: the depth rule against brute force, the interval that codes nothing, the
container, the command line's refusals, verify and info, and a host model of the coded stream.  No device."""
import argparse
import struct
import zlib

import numpy as np
import pytest

from imgcomp_cvpr_amd import arithmetic_coding as ac
from imgcomp_cvpr_amd import codec
from tests import codec_cases as cc
from tests import depth_rule as dr

BLOCKS = (1, 2, 3, 4, 7)
FILL, L = 2, 6


def _profiles(C, h, w, B):
    """cell depths (h, w) per profile: patches of depth 0, C and values between, laid out so that there is a block of depth 0, a
    block of depth C and a ragged last block with something in it (where B leaves one)"""
    rs = np.random.RandomState(100 * C + 10 * h + w + B)
    nby, nbx = -(-h // B), -(-w // B)
    blocks = rs.randint(0, C + 1, size=(nby, nbx))
    blocks.flat[0] = 0                                                       # a dead first block
    blocks.flat[-1] = C                                                      # the last block, ragged where B does not divide: full depth
    if blocks.size > 2:
        blocks.flat[1] = max(1, C // 2)
    cells = np.repeat(np.repeat(blocks, B, 0), B, 1)[:h, :w]
    thin = cells.copy()                                                      # the same, but only one cell of a block reaches its depth
    for by in range(nby):
        for bx in range(nbx):
            patch = thin[by * B:(by + 1) * B, bx * B:(bx + 1) * B]
            keep = patch.flat[patch.size - 1]
            patch[...] = 0
            patch.flat[patch.size - 1] = keep
    return {'patches': (cells, blocks), 'one cell per block': (thin, blocks), 'all dead': (np.zeros((h, w), int), np.zeros((nby, nbx), int)),
            'all C': (np.full((h, w), C), np.full((nby, nbx), C))}


def _tiles(shape, tile):
    C, h, w = shape
    th, tw = tile if tile else (h, w)
    return codec.tile_grid(h, w, th, tw)


@pytest.mark.parametrize('B', BLOCKS)
@pytest.mark.parametrize('shape,tile', [((5, 6, 7), (4, 5)), ((3, 1, 1), None), ((8, 9, 3), None)])
def test_depth_rule_against_brute_force(shape, tile, B):
    C, h, w = shape
    for name, (cells, _) in _profiles(C, h, w, B).items():
        vol = dr.planted(shape, FILL, L, cells, seed=B + len(name))
        for y0, x0, a, b in _tiles(shape, tile):                             # blocks are counted from the TILE's corner
            sym = vol[:, y0:y0 + a, x0:x0 + b]
            want = dr.depth_plane(sym, FILL, B)
            got = codec.depth_plane(sym, FILL, B)
            assert got.dtype == np.uint8 and got.shape == (-(-a // B), -(-b // B)) and np.array_equal(got, want), (name, shape, B, y0, x0)
            mask = codec.depth_live_mask(C, a, b, got, B)
            assert mask.dtype == bool and np.array_equal(mask, dr.live_mask(C, a, b, want, B)), (name, shape, B, y0, x0)
            assert np.array_equal(codec.depth_live(C, a, b, got, B), dr.live(C, a, b, want, B))
            # every dead position holds the fill symbol: leaving them out loses nothing
            assert (sym[~dr.live(C, a, b, want, B)] == FILL).all()
            assert codec.depth_front_steps(a, b, int(got.max())) == dr.front_steps(C, a, b, want)
    # on the whole volume the planted block depths come back exactly
    for name, (cells, blocks) in _profiles(C, h, w, B).items():
        assert np.array_equal(codec.depth_plane(dr.planted(shape, FILL, L, cells, seed=1), FILL, B), blocks), (name, shape, B)


def test_depth_rule_refusals():
    sym = np.zeros((3, 2, 2), np.int64)
    for bad in (0, 256, 2.0, True, None):
        with pytest.raises(ValueError, match='1 .. 255'):
            codec.depth_plane(sym, 0, bad)
    with pytest.raises(ValueError, match='above 255'):
        codec.check_depth_block(4, 256)
    assert codec.check_depth_block(255, 255) == 255 and codec.DEFAULT_DEPTH_BLOCK == 4
    with pytest.raises(ValueError, match='expected 1 x 1'):
        codec.depth_live_mask(3, 2, 2, np.zeros((2, 2), np.uint8), 2)
    assert codec.depth_live_mask(3, 2, 2, np.array([[255]], np.uint8), 2).all()      # a depth above C counts as C


def test_whole_interval_codes_nothing():
    """(cum_lo, cum_hi, total) = (0, 1, 1) leaves low, high and the pending count as they are and writes no bit, in every state the
    coder can be in between two symbols -- so a stream with such steps in it is the stream without them"""
    rs = np.random.RandomState(3)
    tables = [cc.softmax_tables(rs.randn(1, 6) * s)[0] for s in (0.1, 2.0, 9.0, 30.0)]
    symbols = rs.randint(0, 6, size=400)
    rows = [tables[i % 4] for i in range(400)]
    plain, _ = cc.host_encode(symbols, rows)

    buf = cc._Keep()
    out = ac.CountingBitOutputStream(ac.BitOutputStream(buf))
    enc = ac.ArithmeticEncoder(out)
    enc.write_cum(0, 1, 1)                                                   # before the first symbol
    assert (enc.low, enc.high, enc._pending, out.num_bits) == (0, (1 << 32) - 1, 0, 0)
    seen_pending = 0
    for lo, hi, tot in zip(*cc.triples(symbols, rows)):
        enc.write_cum(lo, hi, tot)
        state = (enc.low, enc.high, enc._pending, out.num_bits)
        for _ in range(3):
            enc.write_cum(0, 1, 1)
            assert (enc.low, enc.high, enc._pending, out.num_bits) == state
        seen_pending = max(seen_pending, enc._pending)
    enc.finish()
    out.close()
    assert buf.kept == plain and seen_pending > 0
    assert cc.host_encode(np.zeros(0, np.int64), np.zeros((0, 6), np.int64))[0] == b'\x80'                             # nothing coded at all: the one byte of first == end


NAMES = dict(ae_name='cvpr/low', pc_name='cvpr/res_shallow')


def _build(B=2, C=5, h=6, w=7, th=4, tw=5, streams=None, depth_of=None):
    grid = codec.tile_grid(h, w, th, tw)
    if streams is None:
        rs = np.random.RandomState(B)
        streams = []
        for t, (_, _, a, b) in enumerate(grid):
            nd = -(-a // B) * -(-b // B)
            depth = bytes(rs.randint(0, C + 1, size=nd).astype(np.uint8)) if depth_of is None else depth_of(t, nd)
            streams.append(depth + bytes(rs.randint(0, 256, size=3 + t).astype(np.uint8)))
    firsts = [t % L for t in range(len(grid))]
    return codec.build_depth_container(NAMES['ae_name'], NAMES['pc_name'], 8 * h - 3, 8 * w, C, h, w, L, 1e9, 0xdeadbeef, th, tw, B,
                                       firsts, streams), streams, firsts


@pytest.mark.parametrize('B', (1, 2, 3, 255))
def test_container_round_trip(B):
    data, streams, firsts = _build(B)
    c = codec.parse_container(data)
    assert isinstance(c, codec.DepthContainer) and c.version == codec.FORMAT_VERSION_DEPTH == 10 and c.depth_block == B
    assert c.streams == streams and c.first_syms == firsts and (c.C, c.h, c.w, c.th, c.tw, c.L) == (5, 6, 7, 4, 5, L)
    assert c.stream_crcs == [zlib.crc32(s) & 0xffffffff for s in streams]    # the tile's CRC covers plane and coder bytes
    again = codec.build_depth_container(c.ae_name, c.pc_name, c.H, c.W, c.C, c.h, c.w, c.L, c.resolution, c.fingerprint, c.th, c.tw,
                                        c.depth_block, c.first_syms, c.streams)
    assert again == data
    # the layout of format 5 with one '<H' behind the tile extent
    five = codec.build_wavefront_container(c.ae_name, c.pc_name, c.H, c.W, c.C, c.h, c.w, c.L, c.resolution, c.fingerprint, c.th, c.tw,
                                           c.first_syms, c.streams)
    at = 4 + 2 + 2 + len(c.ae_name) + 2 + len(c.pc_name) + 8 + 10 + 2 + 8 + 4 + 4
    assert data[6:at] == five[6:at] and data[at:at + 2] == struct.pack('<H', B) and len(data) == len(five) + 2
    assert struct.unpack('<H', data[4:6])[0] == 10 and struct.unpack('<H', five[4:6])[0] == 5
    for cut in (len(data) - 1, at + 1, 10):
        with pytest.raises(ValueError):
            codec.parse_container(data[:cut])
    flipped = bytearray(data)
    flipped[-9] ^= 0x10
    with pytest.raises(ValueError, match='CRC'):
        codec.parse_container(bytes(flipped))


def test_container_refusals():
    B, C = 2, 5
    grid = codec.tile_grid(6, 7, 4, 5)
    nd = [-(-a // B) * -(-b // B) for _, _, a, b in grid]
    good = [bytes([1] * n) + b'\x80' for n in nd]
    assert isinstance(codec.parse_container(_build(B, streams=good)[0]), codec.DepthContainer)
    exact = list(good)
    exact[1] = bytes([0] * nd[1])                                            # the plane and no coder byte: still a stream
    codec.parse_container(_build(B, streams=exact)[0])
    short = list(good)
    short[2] = bytes([1] * (nd[2] - 1))
    with pytest.raises(ValueError, match=r'stream of tile 2 holds {} bytes, its depth plane of .* alone has {}'.format(nd[2] - 1, nd[2])):
        codec.parse_container(_build(B, streams=short)[0])
    deep = list(good)
    deep[3] = bytes([C + 1] + [0] * (nd[3] - 1)) + b'\x80'
    with pytest.raises(ValueError, match=r'depth plane of tile 3 holds 6, above C = 5'):
        codec.parse_container(_build(B, streams=deep)[0])
    edge = list(good)
    edge[3] = bytes([C] * nd[3]) + b'\x80'                                    # C itself is a depth
    codec.parse_container(_build(B, streams=edge)[0])
    with pytest.raises(ValueError, match='1 .. 255'):
        _build(0, streams=good)
    # a block of 0 in the header
    data = bytearray(_build(B, streams=good)[0])
    at = 4 + 2 + 2 + len(NAMES['ae_name']) + 2 + len(NAMES['pc_name']) + 8 + 10 + 2 + 8 + 4 + 4
    data[at:at + 2] = struct.pack('<H', 0)
    head_end = len(data) - 4 - sum(len(s) for s in good) - 4
    data[head_end:head_end + 4] = struct.pack('<I', zlib.crc32(bytes(data[:head_end])) & 0xffffffff)
    data[-4:] = struct.pack('<I', zlib.crc32(bytes(data[:-4])) & 0xffffffff)
    with pytest.raises(ValueError, match='depth block 0'):
        codec.parse_container(bytes(data))


def test_version_9_and_the_unsupported_sentence():
    data = bytearray(_build()[0])
    for v in (0, 3, 7, 9, 11):
        data[4:6] = struct.pack('<H', v)
        with pytest.raises(ValueError, match='unsupported format version {}'.format(v)):
            codec.parse_container(bytes(data))
    assert codec._unsupported(9) == ('unsupported format version 9 (this codec reads versions 1, 2 and 4) and the wavefront version 5 and '
                                     'the layered version 6 and the front-layered version 8')


def test_other_readers_refuse_in_one_sentence():
    data = _build()[0]
    for call in (codec.parse_salvage, codec.parse_partial, codec.parse_recover, codec.stream_header_bytes,
                 lambda d: codec.stream_header_bytes(d, fronts=True), lambda d: codec.stream_header_bytes(d[:6])):
        with pytest.raises(ValueError, match=r'format version 10 \(depth-mapped tiles\) is not read by .*--checked.*--wavefront.*--layers'):
            call(data)


def _flags(command, **kw):
    base = dict(command=command, tile=None, checked=False, wavefront=False, salvage=False, channels=None, layers=None, progressive=False,
                front_layers=None, front_progressive=False, partial=False, recover=False, chunk=None, batch=8, depth=False, depth_block=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_option_clashes():
    for command in ('compress', 'compress-dir', 'transcode', 'transcode-dir', 'rd'):
        codec.check_option_args(_flags(command, tile=128, depth=True))
        codec.check_option_args(_flags(command, tile=128, depth=True, depth_block=1))
        codec.check_option_args(_flags(command, tile=128, depth=True, depth_block=255, checked=True))    # checked is implied anyway
    for flags, why in ((_flags('compress', depth=True), '--depth needs --tile'),
                       (_flags('compress', tile=128, depth_block=2), '--depth-block needs --depth'),
                       (_flags('compress', tile=128, depth=True, wavefront=True), '--depth does not go with --wavefront'),
                       (_flags('compress-dir', tile=128, depth=True, layers='4,32'), '--depth does not go with --layers'),
                       (_flags('compress', tile=128, depth=True, progressive=True), '--depth does not go with --progressive'),
                       (_flags('transcode', tile=128, depth=True, front_layers='4,32'), '--depth does not go with --front-layers'),
                       (_flags('rd', tile=128, depth=True, front_progressive=True), '--depth does not go with --front-progressive'),
                       (_flags('compress', tile=128, depth=True, depth_block=0), '--depth-block 0 is not in 1 .. 255'),
                       (_flags('compress', tile=128, depth=True, depth_block=256), '--depth-block 256 is not in 1 .. 255'),
                       (_flags('decompress', depth=True), '--depth belongs to compress'),
                       (_flags('decompress-dir', tile=128, depth=True), '--depth belongs to compress'),
                       (_flags('measure', depth=True), '--depth belongs to compress')):
        with pytest.raises(ValueError, match=why):
            codec.check_option_args(flags)
    old = argparse.Namespace(command='compress', tile=128, checked=False, wavefront=True, salvage=False, channels=None)
    codec.check_option_args(old)                                              # a namespace without the keys reads as no option
    assert codec._depth_option(_flags('compress', tile=128)) is None
    assert codec._depth_option(_flags('compress', tile=128, depth=True)) == 4
    assert codec._depth_option(_flags('compress', tile=128, depth=True, depth_block=2)) == 2


def test_verify_and_info(tmp_path, capsys):
    B, C = 2, 5
    grid = codec.tile_grid(6, 7, 4, 5)
    planes = [np.array([[0, 3, 5], [1, 0, 2]], np.uint8), np.array([[4], [0]], np.uint8), np.zeros((1, 3), np.uint8), np.array([[5]], np.uint8)]
    assert [p.shape for p in planes] == [(-(-a // B), -(-b // B)) for _, _, a, b in grid]
    streams = [p.tobytes() + b'\x12\x34' for p in planes]
    data = _build(B, streams=streams)[0]
    ok, text = codec.verify_file(data)
    assert ok and text == 'ok (format 10, {} bytes, depth blocks of 2 cells)'.format(len(data))
    bad = bytearray(data)
    bad[-7] ^= 1
    ok, text = codec.verify_file(bytes(bad))
    assert not ok and 'CRC' in text
    live = sum(int(dr.live(C, a, b, p, B).sum()) for (_, _, a, b), p in zip(grid, planes))
    text = codec.info_file(data)
    assert 'format 10' in text and 'depth blocks of 2 x 2 cells, 12 bytes of depth planes' in text
    assert 'live share {:.4f} ({} of {} positions are coded)'.format(live / 210.0, live, 210) in text
    steps = [dr.front_steps(C, a, b, p) for (_, _, a, b), p in zip(grid, planes)]
    assert steps[2] == 0 and 'front steps per tile: {} (all 5 channels: {})'.format(
        ','.join(str(s) for s in steps), ','.join(str(dr.front_steps(C, a, b, np.array([[C]]))) for _, _, a, b in grid)) in text
    path = tmp_path / 'a.icf'
    path.write_bytes(data)
    assert codec.main(['verify', str(path)]) == 0 and 'depth blocks of 2 cells' in capsys.readouterr().out
    assert codec.main(['info', str(path)]) == 0 and 'live share' in capsys.readouterr().out


@pytest.mark.parametrize('B', (1, 2, 3))
def test_host_model_round_trip(B):
    """host_encode over the kept subsequence <-> the depth-aware host decoder, with frequency rows given per position"""
    shape = (5, 4, 5)
    C, th, tw = shape
    rs = np.random.RandomState(40 + B)
    rows = np.maximum((rs.dirichlet(np.ones(L) * 0.3, size=shape) * 1e6).astype(np.int64), 1)
    for name, (cells, _) in _profiles(C, th, tw, B).items():
        sym = dr.planted(shape, FILL, L, cells, seed=7)
        depth = codec.depth_plane(sym, FILL, B)
        data = dr.host_encode(sym, rows, depth, B)
        keep = codec.depth_live_mask(C, th, tw, depth, B)
        order = codec.wavefront_order(C, th, tw)
        flat, frows = sym.reshape(-1)[order], rows.reshape(-1, L)[order]
        assert data == cc.host_encode(flat[1:][keep[1:]], frows[1:][keep[1:]])[0], name      # the mask says the same as the positions
        if not keep[1:].any():
            assert data == b'\x80'
        got = dr.host_decode(data, lambda vol, p: rows[p], shape, depth, B, int(sym[0, 0, 0]), FILL)
        assert np.array_equal(got, sym), name
        for K in (1, 3):
            want = codec.preview_symbols(sym, K, FILL)
            assert np.array_equal(dr.host_decode(data, lambda vol, p: rows[p], shape, depth, B, int(sym[0, 0, 0]), FILL, channels=K), want), (name, K)
        # the depth wins over the first symbol
        other = (FILL + 1) % L
        if not keep[0]:
            assert dr.host_decode(data, lambda vol, p: rows[p], shape, depth, B, other, FILL)[0, 0, 0] == FILL
