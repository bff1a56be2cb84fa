"""Lane-parallel rANS tiles (container format 12) on the host: the coder's table, the slots and rounds, the interleaved coder and its
word order against the rule of tests/rans_rule.py, the container, the command line's refusals, verify and info.  No device."""
import argparse
import hashlib
import struct
import zlib

import numpy as np
import pytest

from imgcomp_cvpr_amd import codec
from tests import rans_rule as rr

SHAPES = ((1, 1, 1), (3, 1, 9), (4, 5, 7), (8, 16, 16), (16, 16, 16))
NAMES = dict(ae_name='cvpr/low', pc_name='cvpr/res_shallow')


def test_constants():
    assert codec.FORMAT_VERSION_RANS == 12 and codec.RANS_LANES == (8, 16, 32, 64) == rr.LANES and codec.DEFAULT_RANS_LANES in codec.RANS_LANES
    assert codec.RANS_M == rr.M == 65536 and codec.RANS_MAX_TOTAL == rr.MAX_TOTAL
    for bad in (0, 4, 12, 128, True, 16.0, '16', None):
        with pytest.raises(ValueError, match='W one of 8, 16, 32, 64'):
            codec.check_rans_lanes(bad)


# ---- the table -------------------------------------------------------------------------------------------------------------------

def _check_table(f):
    g = codec.rans_table(f)
    want = rr.table(f)
    assert g.dtype == np.int64 and g.tolist() == want, (f, g.tolist(), want)
    assert int(g.sum()) == 65536 and int(g.min()) >= 1
    # the deficit went to the FIRST largest entry: without it every entry is the floor (or 1)
    L, T = len(f), sum(int(v) for v in f)
    floors = [max(1, int(v) * (65536 - L) // T) for v in f]
    first_max = [int(v) for v in f].index(max(int(v) for v in f))
    assert [a - b for a, b in zip(want, floors)] == [65536 - sum(floors) if j == first_max else 0 for j in range(L)]
    assert 65536 - sum(floors) >= 1


@pytest.mark.parametrize('L', (1, 2, 6, 16))
def test_table_random_rows(L):
    rs = np.random.RandomState(L)
    for _ in range(200):
        kind = rs.randint(3)
        if kind == 0:
            f = rs.randint(1, 1000, size=L)
        elif kind == 1:
            f = np.maximum((rs.dirichlet(np.ones(L) * 0.2) * 1e9).astype(np.int64), 1)
        else:
            f = np.maximum((rs.dirichlet(np.ones(L) * 5) * 2.0 ** 24).astype(np.int64), 1)
        _check_table(f)


def test_table_hard_rows():
    _check_table([1, 1, 1, 1, 1, 10 ** 9])
    assert codec.rans_table([1, 1, 1, 1, 1, 10 ** 9]).tolist() == [1, 1, 1, 1, 1, 65531]
    _check_table([10 ** 9, 1, 1, 1, 1, 1])
    _check_table([1] * 16)                                                    # every entry a maximum: the first takes the deficit
    assert codec.rans_table([1] * 16).tolist() == [4095 + 16] + [4095] * 15
    _check_table([7, 7])
    assert codec.rans_table([7, 7]).tolist() == [32769, 32767]
    _check_table([5])
    assert codec.rans_table([5]).tolist() == [65536]                          # L = 1: g = M, the encoder's 64-bit compare
    top = (1 << 30) + 2                                                       # a total AT the limit
    _check_table([top - 5, 1, 1, 1, 1, 1])
    _check_table([top // 2, top - top // 2])
    _check_table([1] * 15 + [top - 15])
    for bad in ([], [1] * 17, [0, 5], [3, -1]):
        with pytest.raises(ValueError):
            codec.rans_table(bad)


# ---- slots and rounds --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', SHAPES)
def test_slots(shape):
    C, th, tw = shape
    order = codec.wavefront_order(C, th, tw)
    for t, positions in rr.fronts(C, th, tw).items():
        es = [codec.rans_slot(C, th, tw, *p) for p in positions]
        assert es == [rr.slot(C, th, tw, *p) for p in positions]
        assert es == sorted(es) and len(set(es)) == len(es) and es[0] >= 0    # distinct, ascending in (c, y, x) order
    # e orders a front as wavefront_order does
    keyed = sorted(range(C * th * tw), key=lambda i: ((i % tw) + 2 * ((i // tw) % th) + 4 * (i // (th * tw)),
                                                      codec.rans_slot(C, th, tw, i // (th * tw), (i // tw) % th, i % tw)))
    assert keyed == order.tolist()
    with pytest.raises(ValueError):
        codec.rans_slot(C, th, tw, C, 0, 0)


def test_the_shape_with_two_chunks_on_a_front():
    C, th, tw = 16, 16, 16
    widest = max(max(codec.rans_slot(C, th, tw, *p) for p in ps) + 1 for ps in rr.fronts(C, th, tw).values())
    assert widest > 64                                                        # why the shape is in SHAPES: a front of more than one chunk of 64
    assert all(max(rr.slot(c, a, b, *p) for ps in rr.fronts(c, a, b).values() for p in ps) < 64 for c, a, b in SHAPES[:4])


@pytest.mark.parametrize('W', codec.RANS_LANES)
@pytest.mark.parametrize('shape', SHAPES)
def test_rounds(shape, W):
    C, th, tw = shape
    got = codec.rans_rounds(C, th, tw, W)
    want = rr.rounds(C, th, tw, W)
    assert got.dtype == np.int64 and got.shape == (len(want), W) and got.tolist() == want
    flat = got.reshape(-1)
    assert sorted(flat[flat >= 0].tolist()) == list(range(1, C * th * tw))   # every position exactly once, the first one not at all
    assert not (flat == 0).any()
    if shape == (1, 1, 1):
        assert got.shape == (0, W)
    assert all((row >= 0).any() for row in got)                               # no round of holes only
    # rounds ascend in (t, e div W), coder = e mod W
    last = (-1, -1)
    for row in got:
        keys = set()
        for l, i in enumerate(row):
            if i >= 0:
                c, y, x = i // (th * tw), (i // tw) % th, i % tw
                e = codec.rans_slot(C, th, tw, c, y, x)
                assert e % W == l
                keys.add((x + 2 * y + 4 * c, e // W))
        assert len(keys) == 1 and min(keys) > last
        last = min(keys)
    with pytest.raises(ValueError):
        codec.rans_rounds(C, th, tw, 12)
    with pytest.raises(ValueError):
        codec.rans_rounds(0, th, tw, 8)


# ---- the coder -------------------------------------------------------------------------------------------------------------------------

def _case(shape, W, L, seed, peaked=False):
    C, th, tw = shape
    rs = np.random.RandomState(seed)
    rounds = codec.rans_rounds(C, th, tw, W)
    n = rounds.size
    if peaked:
        rows = np.maximum((rs.dirichlet(np.ones(L) * 0.05, size=n) * 1e8).astype(np.int64), 1).reshape(n, L)
    else:
        rows = rs.randint(1, 5000, size=(n, L)).astype(np.int64)
    sym = np.array([rs.choice(L, p=r / r.sum()) for r in rows], np.int64) if n else np.zeros(0, np.int64)
    sym[rounds.reshape(-1) < 0] = -1
    return rounds, rows, sym


def _decode_both(data, rounds, W, rows, n_out, **kw):
    at = {int(v): i for i, v in enumerate(rounds.reshape(-1)) if v >= 0}
    a, b = np.full(n_out, -7, np.int64), np.full(n_out, -7, np.int64)
    sa = codec.rans_decode(data, rounds, W, lambda out, i: rows[at[i]], a, **kw)
    sb = rr.decode(data, rounds.tolist(), W, lambda out, i: rows[at[i]], b, **kw)
    assert sa == sb and np.array_equal(a, b)
    return a, sa, at


@pytest.mark.parametrize('W', codec.RANS_LANES)
@pytest.mark.parametrize('shape,L,peaked', [((1, 1, 1), 6, False), ((3, 1, 9), 1, False), ((3, 1, 9), 2, True), ((4, 5, 7), 6, False),
                                            ((4, 5, 7), 16, True), ((8, 16, 16), 6, True)])
def test_round_trip_and_word_order(shape, L, peaked, W):
    rounds, rows, sym = _case(shape, W, L, seed=W + L, peaked=peaked)
    n_out = shape[0] * shape[1] * shape[2]
    data = codec.rans_encode(rows, sym, W)
    want, status = rr.encode(rows.tolist(), sym.tolist(), W)                  # written from the coder's definition ...
    assert status == 0 and data == want
    assert len(data) >= 4 * W and (len(data) - 4 * W) % 2 == 0
    got, st, at = _decode_both(data, rounds, W, rows, n_out)                  # ... read from the stream's definition
    assert st == 0
    for i, k in at.items():
        assert got[i] == sym[k]
    assert got[0] == -7                                                       # the first position is not the coder's
    if L == 1 or not at:
        assert data == struct.pack('<{}I'.format(W), *([65536] * W))          # g = M: a symbol costs nothing, no word is ever emitted


def test_a_preview_stops_early_and_is_not_end_checked():
    shape, W, L = (4, 5, 7), 8, 6
    rounds, rows, sym = _case(shape, W, L, seed=3)
    data = codec.rans_encode(rows, sym, W)
    stop = rr.preview_rounds(4, 5, 7, W, 2)
    assert 0 < stop < len(rounds)
    got, st, at = _decode_both(data, rounds, W, rows, 140, stop=stop)
    assert st == 0
    done = set(int(v) for v in rounds[:stop].reshape(-1) if v >= 0)
    assert set(range(1, 2 * 35)) <= done                                      # every position of channels 0 and 1
    assert all(got[i] == sym[at[i]] for i in done) and all(got[i] == -7 for i in at if i not in done)


def test_strings_no_encoder_wrote():
    shape, W, L = (4, 5, 7), 8, 6
    rounds, rows, sym = _case(shape, W, L, seed=5)
    real = codec.rans_encode(rows, sym, W)
    rs = np.random.RandomState(9)
    strings = [b'', b'\x00', b'\xff', real[:-1], real[:-2], real + b'\x00\x00', real + b'\x01']
    strings += [real[:n] for n in range(0, 4 * W + 9)]
    strings += [bytes(rs.randint(0, 256, size=n).astype(np.uint8)) for n in (1, 3, 31, 32, 33, 100, 400, 2000)]
    strings += [struct.pack('<{}I'.format(W), *([v] * W)) + real[4 * W:] for v in (0, 0xffffffff, 65535, 65536)]
    for s in strings:
        got, st, at = _decode_both(s, rounds, W, rows, 140)
        assert st in (0, 4) and all(0 <= got[i] < L for i in at)
    assert _decode_both(real, rounds, W, rows, 140)[1] == 0
    assert _decode_both(real[:-2], rounds, W, rows, 140)[1] == 4
    assert _decode_both(real + b'\x00\x00', rounds, W, rows, 140)[1] == 4     # bytes left over
    assert _decode_both(b'', rounds, W, rows, 140)[1] == 4


def test_status_1_and_3():
    W, L = 8, 6
    rounds, rows, sym = _case((3, 1, 9), W, L, seed=1)
    big = rows.copy()
    k = int(np.flatnonzero(sym >= 0)[3])
    big[k] = [(1 << 30) - 2, 1, 1, 1, 1, 1]                                   # total 2^30 + 3: one over the limit
    with pytest.raises(ValueError, match='total is too large'):
        codec.rans_encode(big, sym, W)
    assert rr.encode(big.tolist(), sym.tolist(), W) == (None, 1)
    big[k] = [(1 << 30) - 3, 1, 1, 1, 1, 1]                                   # at the limit: coded
    data = codec.rans_encode(big, sym, W)
    assert (data, 0) == rr.encode(big.tolist(), sym.tolist(), W)
    assert _decode_both(data, rounds, W, big, 27)[1] == 0
    big[k] = [(1 << 30) - 2, 1, 1, 1, 1, 1]
    assert _decode_both(data, rounds, W, big, 27)[1] & 1                      # the decoder goes on and says so
    wrong = sym.copy()
    wrong[k] = L
    with pytest.raises(ValueError, match='outside'):
        codec.rans_encode(rows, wrong, W)
    assert rr.encode(rows.tolist(), wrong.tolist(), W) == (None, 3)
    with pytest.raises(ValueError, match='whole rounds'):
        codec.rans_encode(rows[:-1], sym[:-1], W)


def test_the_bytes_are_pinned():
    """one fixed input: the format's bytes do not move"""
    W, L = 16, 6
    rounds, rows, sym = _case((4, 5, 7), W, L, seed=2026, peaked=True)
    assert hashlib.sha256(rows.tobytes() + sym.tobytes()).hexdigest() == PINNED_INPUT
    data = codec.rans_encode(rows, sym, W)
    assert rr.encode(rows.tolist(), sym.tolist(), W) == (data, 0)
    assert hashlib.sha256(data).hexdigest() == PINNED_STREAM


PINNED_INPUT = 'e9f62c3f8e0534919b87bd4e4e89b4ba07c431320e6fccae5ed26d49236144f1'
PINNED_STREAM = '5503bac8ce0835d2e1491b180c2cae51af5aa1340438546ed038c74a14e839e1'


# ---- container and command line -------------------------------------------------------------------------------------------------------------

def _build(W=16, h=6, w=7, th=4, tw=5, C=5, L=6, streams=None):
    grid = codec.tile_grid(h, w, th, tw)
    if streams is None:
        rs = np.random.RandomState(W)
        streams = [struct.pack('<{}I'.format(W), *([65536 + t] * W)) + bytes(rs.randint(0, 256, size=2 * (3 + t)).astype(np.uint8))
                   for t in range(len(grid))]
    firsts = [t % L for t in range(len(grid))]
    return codec.build_rans_container(NAMES['ae_name'], NAMES['pc_name'], 8 * h - 3, 8 * w, C, h, w, L, 1e9, 0xdeadbeef, th, tw, W,
                                      firsts, streams), streams, firsts


@pytest.mark.parametrize('W', codec.RANS_LANES)
def test_container_round_trip(W):
    data, streams, firsts = _build(W)
    c = codec.parse_container(data)
    assert isinstance(c, codec.RansContainer) and isinstance(c, codec._TILED) and c.version == 12 and c.lanes == W
    assert c.streams == streams and c.first_syms == firsts and (c.C, c.h, c.w, c.th, c.tw, c.L) == (5, 6, 7, 4, 5, 6)
    assert c.stream_crcs == [zlib.crc32(s) & 0xffffffff for s in streams]
    again = codec.build_rans_container(c.ae_name, c.pc_name, c.H, c.W, c.C, c.h, c.w, c.L, c.resolution, c.fingerprint, c.th, c.tw,
                                       c.lanes, c.first_syms, c.streams)
    assert again == data
    # the layout of format 10, W where it keeps its block size
    ten = codec.build_depth_container(c.ae_name, c.pc_name, c.H, c.W, c.C, c.h, c.w, c.L, c.resolution, c.fingerprint, c.th, c.tw,
                                      W, c.first_syms, c.streams)
    assert data[6:] != ten[6:] and len(data) == len(ten)                      # (the CRCs cover the version)
    at = 4 + 2 + 2 + len(c.ae_name) + 2 + len(c.pc_name) + 8 + 10 + 2 + 8 + 4 + 4
    assert data[6:at + 2] == ten[6:at + 2] and data[at:at + 2] == struct.pack('<H', W)
    assert struct.unpack('<H', data[4:6])[0] == 12
    for cut in (len(data) - 1, at + 1, 10):
        with pytest.raises(ValueError):
            codec.parse_container(data[:cut])
    for pos in (-9, at, at + 30, 8):                                          # a flipped byte anywhere is refused
        flipped = bytearray(data)
        flipped[pos] ^= 0x10
        with pytest.raises(ValueError):
            codec.parse_container(bytes(flipped))
    flipped = bytearray(data)
    flipped[-9] ^= 0x10
    with pytest.raises(ValueError, match='CRC'):
        codec.parse_container(bytes(flipped))


def test_container_refusals():
    W = 8
    good = [struct.pack('<8I', *([65536] * 8)) + b'\x01\x02'] * 4
    assert codec.parse_container(_build(W, streams=good)[0]).lanes == 8
    bare = list(good)
    bare[1] = good[1][:32]                                                    # the states and no word: a stream
    codec.parse_container(_build(W, streams=bare)[0])
    short = list(good)
    short[2] = good[2][:31]
    with pytest.raises(ValueError, match='stream of tile 2 holds 31 bytes: the states of its 8 coders have 32'):
        codec.parse_container(_build(W, streams=short)[0])
    odd = list(good)
    odd[3] = good[3] + b'\x00'
    with pytest.raises(ValueError, match='stream of tile 3 holds 35 bytes'):
        codec.parse_container(_build(W, streams=odd)[0])
    with pytest.raises(ValueError, match='W one of'):
        _build(12, streams=good)
    data = bytearray(_build(W, streams=good)[0])                              # another W in the header, every CRC right
    at = 4 + 2 + 2 + len(NAMES['ae_name']) + 2 + len(NAMES['pc_name']) + 8 + 10 + 2 + 8 + 4 + 4
    data[at:at + 2] = struct.pack('<H', 12)
    head_end = len(data) - 4 - sum(len(s) for s in good) - 4
    data[head_end:head_end + 4] = struct.pack('<I', zlib.crc32(bytes(data[:head_end])) & 0xffffffff)
    data[-4:] = struct.pack('<I', zlib.crc32(bytes(data[:-4])) & 0xffffffff)
    with pytest.raises(ValueError, match='12 coders per tile: format 12 has W in 8, 16, 32, 64'):
        codec.parse_container(bytes(data))


def test_version_11_stays_unsupported():
    data = bytearray(_build()[0])
    for v in (0, 3, 7, 9, 11, 13):
        data[4:6] = struct.pack('<H', v)
        with pytest.raises(ValueError, match='unsupported format version {}'.format(v)):
            codec.parse_container(bytes(data))


def test_other_readers_refuse_in_one_sentence():
    data = _build()[0]
    for call in (codec.parse_salvage, codec.parse_partial, codec.parse_recover, codec.stream_header_bytes,
                 lambda d: codec.stream_header_bytes(d, fronts=True), lambda d: codec.stream_header_bytes(d[:6])):
        with pytest.raises(ValueError, match=r'format version 12 \(lane-parallel rANS tiles\) is not read by .*--checked.*--wavefront.*--layers'):
            call(data)
    for what in ('--salvage', '--partial / --recover / stream', 'repair'):
        with pytest.raises(ValueError) as e:
            codec._refuse(data, what)
        assert str(e.value) == ('format version 12 (lane-parallel rANS tiles) is not read by {}: a file to be salvaged is written with --tile '
                                '--checked or --tile --wavefront (versions 4 and 5), a file to be read from a prefix, recovered or streamed '
                                'with the layered formats --layers / --front-layers (versions 6 and 8); an intact file decodes with '
                                'decompress'.format(what))
    codec._refuse(codec.build_wavefront_container('a', 'p', 8, 8, 1, 1, 1, 6, 1e9, 0, 1, 1, [0], [b'\x80']), 'repair')     # another format: not its business


def _flags(command, **kw):
    base = dict(command=command, tile=None, checked=False, wavefront=False, salvage=False, channels=None, layers=None, progressive=False,
                front_layers=None, front_progressive=False, partial=False, recover=False, chunk=None, batch=8, depth=False, depth_block=None,
                rans=False, lanes=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_option_clashes():
    for command in ('compress', 'compress-dir', 'transcode', 'transcode-dir', 'rd'):
        codec.check_option_args(_flags(command, tile=128, rans=True))
        for W in codec.RANS_LANES:
            codec.check_option_args(_flags(command, tile=128, rans=True, lanes=W))
    for flags, why in ((_flags('compress', rans=True), '--rans needs --tile'),
                       (_flags('compress', tile=128, lanes=16), '--lanes needs --rans'),
                       (_flags('compress', tile=128, rans=True, checked=True), '--rans does not go with --checked'),
                       (_flags('compress', tile=128, rans=True, wavefront=True), '--rans does not go with --wavefront'),
                       (_flags('compress', tile=128, rans=True, depth=True), '--rans does not go with --depth'),
                       (_flags('compress-dir', tile=128, rans=True, layers='4,32'), '--rans does not go with --layers'),
                       (_flags('compress', tile=128, rans=True, progressive=True), '--rans does not go with --progressive'),
                       (_flags('transcode', tile=128, rans=True, front_layers='4,32'), '--rans does not go with --front-layers'),
                       (_flags('rd', tile=128, rans=True, front_progressive=True), '--rans does not go with --front-progressive'),
                       (_flags('compress', tile=128, rans=True, lanes=12), '--lanes 12 is not one of 8, 16, 32, 64'),
                       (_flags('compress', tile=128, rans=True, lanes=0), '--lanes 0 is not one of'),
                       (_flags('decompress', rans=True), '--rans belongs to compress'),
                       (_flags('decompress-dir', tile=128, rans=True), '--rans belongs to compress'),
                       (_flags('measure', rans=True), '--rans belongs to compress')):
        with pytest.raises(ValueError, match=why):
            codec.check_option_args(flags)
    old = argparse.Namespace(command='compress', tile=128, checked=False, wavefront=True, salvage=False, channels=None)
    codec.check_option_args(old)                                              # a namespace without the keys reads as no option
    assert codec._rans_option(_flags('compress', tile=128)) is None
    assert codec._rans_option(_flags('compress', tile=128, rans=True)) == 'default'
    assert codec._rans_option(_flags('compress', tile=128, rans=True, lanes=64)) == 64
    for kw, why in ((dict(tile=None), 'needs a tile extent'), (dict(checked=True), 'checked=True'), (dict(order='wavefront'), "order='wavefront'"),
                    (dict(depth_block=4), 'depth_block'), (dict(layers='default'), 'layers or front_layers'),
                    (dict(front_layers=[4, 32]), 'layers or front_layers'), (dict(rans=12), 'W one of')):
        args = dict(rans=16, tile=(16, 16), checked=False, order='raster', layers=None, front_layers=None, depth_block=None)
        args.update(kw)
        with pytest.raises(ValueError, match=why):
            codec.Codec._check_rans(**args)
    codec.Codec._check_rans('default', (16, 16), False, 'raster', None, None, None)


def test_verify_and_info(tmp_path, capsys):
    data, streams, _ = _build(16)
    ok, text = codec.verify_file(data)
    assert ok and text == 'ok (format 12, {} bytes, W = 16 coders per tile)'.format(len(data))
    bad = bytearray(data)
    bad[-7] ^= 1
    ok, text = codec.verify_file(bytes(bad))
    assert not ok and 'CRC' in text
    text = codec.info_file(data)
    payload = sum(len(s) for s in streams)
    assert 'format 12' in text and 'payload {} bytes'.format(payload) in text
    assert 'W = 16 interleaved coders per tile, 256 bytes of coder states: {:.4f} of the payload'.format(256.0 / payload) in text
    path = tmp_path / 'a.icf'
    path.write_bytes(data)
    assert codec.main(['verify', str(path)]) == 0 and 'W = 16 coders per tile' in capsys.readouterr().out
    assert codec.main(['info', str(path)]) == 0 and 'bytes of coder states' in capsys.readouterr().out
