"""Layered tiles (container format 6) on the host: the container and its strict reader, the prefix reader, the options -- and, first,
the statement the format rests on: the reference range coder survives a cut at any symbol (the coder restarted there codes the
rest as a stream of its own, over the same table rows), also in its hard states."""
import argparse
import struct
import zlib

import numpy as np
import pytest

from imgcomp_cvpr_amd import codec
from tests import codec_cases as cc


# ---- the coder model: run first ---------------------------------------------------------------------------------------------

def _segments(symbols, freqs, cuts):
    """the symbols cut at `cuts` (positions in 1 .. n - 1, increasing) -> [(bytes, a, b)]: every piece coded by a fresh host coder"""
    edges = [0] + list(cuts) + [len(symbols)]
    return [(cc.host_encode(symbols[a:b], freqs[a:b])[0], a, b) for a, b in zip(edges, edges[1:])]


def _check_cuts(symbols, freqs, cuts):
    got = []
    for data, a, b in _segments(symbols, freqs, cuts):
        piece = cc.host_decode(data, list(freqs[a:b]))          # each segment against its own table rows
        assert piece == [int(v) for v in symbols[a:b]], (cuts, a, b)
        model, status = cc.model_decode(data, list(freqs[a:b]))     # and the device decoder's word-level model, restarted alike
        assert status == 0 and model == piece
        got += piece
    assert got == [int(v) for v in symbols]


def test_coder_survives_a_cut_at_any_symbol_random_tables():
    rs = np.random.RandomState(1)
    logits = rs.uniform(0, 4, size=(120, 6)).astype(np.float32)
    freqs = cc.softmax_tables(logits)
    symbols = rs.randint(0, 6, size=120).astype(np.int64)
    whole = cc.host_encode(symbols, freqs)[0]
    assert _segments(symbols, freqs, [])[0][0] == whole                   # G = 1 is the whole stream, byte for byte
    for cut in range(1, 120):
        _check_cuts(symbols, freqs, [cut])
    _check_cuts(symbols, freqs, list(range(1, 120)))                      # one symbol per segment
    _check_cuts(symbols, freqs, [7, 8, 64, 65, 119])


def test_coder_survives_a_cut_inside_a_pending_run():
    logits, symbols = cc.pending_run_logits()
    freqs = cc.softmax_tables(logits)
    whole, pending = cc.host_encode(symbols, freqs)
    assert pending > 64, 'the construction no longer reaches a long pending run'
    assert _segments(symbols, freqs, [])[0][0] == whole
    for cut in range(1, len(symbols)):                                    # every position: before, inside and behind the run
        _check_cuts(symbols, freqs, [cut])
    _check_cuts(symbols, freqs, [20, 40, 60, 80, 100])


def test_coder_survives_a_cut_at_the_worst_case_cost():
    logits, symbols = cc.worst_case_logits(120)
    freqs = cc.softmax_tables(logits)
    assert int(freqs[0][0]) == 1
    assert _segments(symbols, freqs, [])[0][0] == cc.host_encode(symbols, freqs)[0]
    for cut in range(1, len(symbols)):
        _check_cuts(symbols, freqs, [cut])
    _check_cuts(symbols, freqs, list(range(1, len(symbols), 7)))


def test_empty_segment_is_one_byte():
    assert cc.host_encode(np.zeros(0, np.int64), np.zeros((0, 6), np.int64))[0] == b'\x80'
    assert cc.model_encode([], [], [])[0] == b'\x80'


# ---- the container ----------------------------------------------------------------------------------------------------------

HEAD = dict(ae_name='cvpr/low', pc_name='cvpr/res_shallow', H=40, W=56, C=8, h=5, w=7, L=6, resolution=1e9, fingerprint=0x1234abcd, th=4, tw=4)
ENDS = [1, 2, 8]


def _file(ends=ENDS, seed=3, first_syms=None, head=HEAD):
    rs = np.random.RandomState(seed)
    nt = len(codec.tile_grid(head['h'], head['w'], head['th'], head['tw']))
    segments = [[rs.randint(0, 256, size=int(rs.randint(1, 9))).astype(np.uint8).tobytes() for _ in range(nt)] for _ in ends]
    first_syms = list(rs.randint(0, head['L'], size=nt)) if first_syms is None else first_syms
    args = [head[k] for k in ('ae_name', 'pc_name', 'H', 'W', 'C', 'h', 'w', 'L', 'resolution', 'fingerprint', 'th', 'tw')]
    return codec.build_layered_container(*(args + [[int(f) for f in first_syms], ends, segments])), segments, [int(f) for f in first_syms]


def _front_len(head=HEAD):
    """bytes up to and including ntiles"""
    return 4 + 2 + 2 + len(head['ae_name']) + 2 + len(head['pc_name']) + 8 + 10 + 2 + 8 + 4 + 4 + 4


def test_round_trip_and_layout():
    data, segments, firsts = _file()
    c = codec.parse_container(data)
    assert isinstance(c, codec.LayeredContainer) and isinstance(c, codec._TILED) and c.version == 6
    assert c.layer_ends == ENDS and c.segments == segments and c.first_syms == firsts
    assert c.streams == [[segments[g][t] for g in range(3)] for t in range(4)]
    assert c.segment_crcs == [[zlib.crc32(b) & 0xffffffff for b in layer] for layer in segments]
    assert (c.ae_name, c.pc_name, c.H, c.W, c.C, c.h, c.w, c.L, c.resolution, c.fingerprint, c.th, c.tw) == tuple(
        HEAD[k] for k in ('ae_name', 'pc_name', 'H', 'W', 'C', 'h', 'w', 'L', 'resolution', 'fingerprint', 'th', 'tw'))
    assert c.payload == b''.join(b for layer in segments for b in layer)            # LAYER-major
    # the header up to ntiles is the format-4 header apart from the version word
    args = [HEAD[k] for k in ('ae_name', 'pc_name', 'H', 'W', 'C', 'h', 'w', 'L', 'resolution', 'fingerprint', 'th', 'tw')]
    four = codec.build_checked_container(*(args + [firsts, [b'x'] * 4]))
    n = _front_len()
    assert data[:4] == four[:4] and data[6:n] == four[6:n] and struct.unpack('<H', data[4:6])[0] == 6 and struct.unpack('<H', four[4:6])[0] == 4
    # the length is the layout's formula
    G, nt, payload = 3, 4, sum(len(b) for layer in segments for b in layer)
    assert len(data) == n + 2 + 2 * G + 2 * nt + 8 * G * nt + 8 + 4 + payload + 4
    assert struct.unpack_from('<H', data, n)[0] == G and list(struct.unpack_from('<3H', data, n + 2)) == ENDS
    assert list(struct.unpack_from('<4H', data, n + 2 + 2 * G)) == firsts
    table = n + 2 + 2 * G + 2 * nt
    assert struct.unpack_from('<II', data, table + 8 * (1 * nt + 2)) == (len(segments[1][2]), zlib.crc32(segments[1][2]) & 0xffffffff)
    assert [codec.layer_prefix_bytes(c, g) for g in range(4)] == [codec.layer_prefix_bytes(data, g) for g in range(4)]
    assert codec.layer_prefix_bytes(c, 0) == table + 8 * G * nt + 8 + 4 and codec.layer_prefix_bytes(c, 3) == len(data) - 4
    assert codec.layer_prefix_bytes(c, 1) - codec.layer_prefix_bytes(c, 0) == sum(len(b) for b in segments[0])
    for bad in (-1, 4, 1.5, True):
        with pytest.raises(ValueError, match='outside 0 .. G = 3'):
            codec.layer_prefix_bytes(data, bad)
    one, segs1, _ = _file(ends=[8])
    assert codec.parse_container(one).layer_ends == [8]


def _resealed(data, edit):
    """a copy of a valid file with `edit(bytearray of everything before the header CRC)` applied and both CRCs made right again"""
    cut = codec.layer_prefix_bytes(data, 0) - 4
    head, payload = bytearray(data[:cut]), data[cut + 4:-4]
    head = bytes(edit(head) or head)
    body = head + struct.pack('<I', zlib.crc32(head) & 0xffffffff) + payload
    return body + struct.pack('<I', zlib.crc32(body) & 0xffffffff)


def test_refusals_name_their_cause():
    data, segments, firsts = _file()
    n, G, nt = _front_len(), 3, 4
    assert codec.parse_container(_resealed(data, lambda h: None)).segments == segments

    def put(off, fmt, *vals):
        def edit(h):
            struct.pack_into(fmt, h, off, *vals)
        return edit

    def drop_layers(h):                                           # G = 0: no ends, no table
        return h[:n] + struct.pack('<H', 0) + h[n + 2 + 2 * G:n + 2 + 2 * G + 2 * nt] + struct.pack('<Q', 0)
    with pytest.raises(ValueError, match=r'layer count G = 0 is outside 1 \.\. 16'):
        codec.parse_container(_resealed(data, drop_layers))
    with pytest.raises(ValueError, match=r'layer count G = 17 is outside 1 \.\. 16'):
        codec.parse_container(_resealed(data, put(n, '<H', 17)))
    with pytest.raises(ValueError, match='not increasing'):
        codec.parse_container(_resealed(data, put(n + 2, '<3H', 2, 2, 8)))
    with pytest.raises(ValueError, match='not increasing'):
        codec.parse_container(_resealed(data, put(n + 2, '<3H', 0, 2, 8)))
    with pytest.raises(ValueError, match='last layer end 7 is not C = 8'):
        codec.parse_container(_resealed(data, put(n + 2, '<3H', 1, 2, 7)))
    # a table longer than the file, behind a file CRC that is right: the header cut inside the segment table, then a header CRC and
    # the CRC over the file, put together by hand
    table = n + 2 + 2 * G + 2 * nt
    short = data[:table + 20]
    short += struct.pack('<I', zlib.crc32(short) & 0xffffffff)
    short += struct.pack('<I', zlib.crc32(short) & 0xffffffff)
    assert len(short) == table + 28 < table + 8 * G * nt
    with pytest.raises(ValueError, match='truncated file: segment table needs 96 bytes'):
        codec.parse_container(short)
    with pytest.raises(ValueError, match='segment lengths .* sum to'):
        codec.parse_container(_resealed(data, put(table, '<I', len(segments[0][0]) + 1)))
    with pytest.raises(ValueError, match='first symbol 6 of tile 1 is not below L = 6'):
        codec.parse_container(_resealed(data, put(n + 2 + 2 * G + 2, '<H', 6)))
    with pytest.raises(ValueError, match='payload length .* does not equal'):
        whole = _resealed(data, lambda h: None)
        body = whole[:-4] + b'\x00'
        codec.parse_container(body + struct.pack('<I', zlib.crc32(body) & 0xffffffff))
    # a segment CRC and the header CRC are checked behind a file CRC that is right
    flipped = bytearray(data)
    flipped[codec.layer_prefix_bytes(data, 1) + 1] ^= 0x10
    body = bytes(flipped[:-4])
    with pytest.raises(ValueError, match='segment CRC mismatch in layer 1, tile 0'):
        codec.parse_container(body + struct.pack('<I', zlib.crc32(body) & 0xffffffff))
    flipped = bytearray(data)
    flipped[n - 10] ^= 0x01                                               # the model fingerprint: every field still parses
    body = bytes(flipped[:-4])
    with pytest.raises(ValueError, match='header CRC mismatch'):
        codec.parse_container(body + struct.pack('<I', zlib.crc32(body) & 0xffffffff))
    for bad, why in (([], 'G = 0'), (list(range(1, 18)), 'G = 17'), ([2, 2, 8], 'not increasing'), ([1, 2, 7], 'not C = 8'), ([1.5, 8], 'integers')):
        with pytest.raises(ValueError, match=why):
            codec.check_layer_ends(bad, 8)
    assert codec.check_layer_ends((1, np.int64(8)), 8) == [1, 8]


def test_every_flip_and_every_truncation_is_refused():
    data, _, _ = _file()
    for i in range(len(data)):
        bad = bytearray(data)
        bad[i] ^= 1 << (i % 8)
        with pytest.raises(ValueError, match='magic|version|CRC|truncated'):
            codec.parse_container(bytes(bad))
    for n in range(len(data)):
        with pytest.raises(ValueError, match='magic|version|CRC|truncated'):
            codec.parse_container(data[:n])


def test_versions():
    data, _, _ = _file()

    def with_version(v):
        body = data[:4] + struct.pack('<H', v) + data[6:-4]
        return body + struct.pack('<I', zlib.crc32(body) & 0xffffffff)
    # the sentences the existing tests pin still match
    with pytest.raises(ValueError, match=r'unsupported format version 3 \(this codec reads versions 1, 2 and 4\) and the wavefront version 5'):
        codec.parse_container(with_version(3))
    with pytest.raises(ValueError, match=r'unsupported format version 7 .* and the layered version 6'):
        codec.parse_container(with_version(7))
    with pytest.raises(ValueError, match='unsupported format version 3'):
        codec.parse_salvage(with_version(3))
    with pytest.raises(ValueError, match='salvage of layered files is out of scope'):
        codec.parse_salvage(data)
    with pytest.raises(ValueError, match='header damaged: format version 4 is not the layered version 6'):
        codec.parse_partial(with_version(4))
    ok, text = codec.verify_file(data)
    assert ok and 'format 6' in text and 'G = 3' in text and 'ends 1,2,8' in text
    assert 'prefix lengths ' + ','.join(str(codec.layer_prefix_bytes(data, g)) for g in range(4)) in text
    ok, text = codec.verify_file(data[:codec.layer_prefix_bytes(data, 2)])
    assert not ok and '2 of 3 layers complete' in text


# ---- the prefix reader ------------------------------------------------------------------------------------------------------

def test_every_cut_gives_what_the_prefix_lengths_predict():
    data, segments, _ = _file()
    bounds = [codec.layer_prefix_bytes(data, g) for g in range(4)]
    assert bounds == sorted(bounds) and bounds[-1] == len(data) - 4
    last = -1
    for n in range(len(data) + 1):
        if n < bounds[0]:
            with pytest.raises(ValueError, match='header damaged'):
                codec.parse_partial(data[:n])
            continue
        c, complete, file_crc_ok = codec.parse_partial(data[:n])
        assert complete == sum(1 for b in bounds[1:] if n >= b), n
        assert complete >= last and file_crc_ok == (n == len(data))
        last = complete
        assert c.layer_ends == ENDS and c.segments[:complete] == segments[:complete]
        assert all(b is None or b == segments[g][t] for g in range(3) for t, b in enumerate(c.segments[g]))
        assert all(any(b is None for b in c.segments[g]) for g in range(complete, 3) if n < bounds[g + 1])
        assert c.streams == [[c.segments[g][t] for g in range(3)] for t in range(4)]
    assert last == 3
    assert codec.parse_partial(data + b'trailing')[1:] == (3, True)       # bytes behind the declared end are ignored


def test_a_flipped_byte_in_a_segment_ends_the_complete_layers_there():
    data, segments, _ = _file()
    for g in range(3):
        for t in range(4):
            pos = codec.layer_prefix_bytes(data, g) + sum(len(b) for b in segments[g][:t])
            bad = bytearray(data)
            bad[pos + len(segments[g][t]) // 2] ^= 0x40
            c, complete, file_crc_ok = codec.parse_partial(bytes(bad))
            assert complete == g and not file_crc_ok and c.segments[g][t] is None, (g, t)
            assert sum(b is None for layer in c.segments for b in layer) == 1
    bad = bytearray(data)
    bad[_front_len() + 2] ^= 0x01                                          # a layer end: the header's own CRC speaks
    with pytest.raises(ValueError, match='header damaged'):
        codec.parse_partial(bytes(bad))


# ---- options ----------------------------------------------------------------------------------------------------------------

def test_default_layer_ends():
    for C in range(1, 41):
        ends = codec.default_layer_ends(C)
        assert ends == sorted(set(ends)) and ends[0] >= 1 and ends[-1] == C and 1 <= len(ends) <= 4
        assert codec.check_layer_ends(ends, C) == ends
        assert set(ends) == set(e for e in (max(1, C // 8), C // 4, C // 2, C) if e > 0)
    assert codec.default_layer_ends(32) == [4, 8, 16, 32]


def _flags(command, **kw):
    base = dict(command=command, tile=None, checked=False, wavefront=False, salvage=False, channels=None, layers=None, progressive=False,
                partial=False, batch=8)
    base.update(kw)
    return argparse.Namespace(**base)


def test_option_clashes():
    codec.check_option_args(_flags('compress', tile=128, layers='4,8,16,32'))
    codec.check_option_args(_flags('compress-dir', tile=128, progressive=True))
    codec.check_option_args(_flags('decompress', partial=True))
    codec.check_option_args(_flags('decompress-dir', partial=True))
    for flags, why in ((_flags('compress', layers='4,32'), '--layers needs --tile'),
                       (_flags('compress', progressive=True), '--progressive needs --tile'),
                       (_flags('compress', tile=128, layers='4,32', wavefront=True), '--layers does not go with --wavefront'),
                       (_flags('compress-dir', tile=128, progressive=True, wavefront=True), '--progressive does not go with --wavefront'),
                       (_flags('compress', tile=128, layers='4,32', progressive=True), '--layers does not go with --progressive'),
                       (_flags('decompress', layers='4,32'), '--layers belongs to compress'),
                       (_flags('decompress-dir', progressive=True), '--progressive belongs to compress'),
                       (_flags('compress', tile=128, layers='4,x'), 'comma-separated list of integers'),
                       (_flags('compress', tile=128, layers='8,4'), 'increasing'),
                       (_flags('compress', tile=128, layers='0,4'), 'increasing'),
                       (_flags('compress', partial=True), '--partial belongs to decompress'),
                       (_flags('decompress', partial=True, salvage=True), '--partial does not go with --salvage'),
                       (_flags('decompress-dir', partial=True, channels=4), '--partial does not go with --channels')):
        with pytest.raises(ValueError, match=why):
            codec.check_option_args(flags)
    assert codec.parse_layers_arg('4,8,16,32') == [4, 8, 16, 32]
