"""Tiled codec (container format 2), the parts that need no GPU: the tile grid, the container, and the host-side argument checks
of ic_pc_decode_tiles_f32, which decide everything about a tile table before the first device call."""
import ctypes
import struct
import zlib

import numpy as np
import pytest


def _fields(streams=(b'\x12\x34', b'', b'\x80', b'\x01\x02\x03', b'\xff', b'\x10\x20')):
    # the 8 x 12 latent plane of a 61 x 93 image cut into 3 x 5 tiles: 3 x 3 = 9 tiles
    streams = list(streams) + [bytes([i]) * i for i in range(9 - len(streams))]
    return dict(ae_name='cvpr/low', pc_name='cvpr/res_shallow', H=61, W=93, C=32, h=8, w=12, L=6, resolution=1e9,
                fingerprint=0xdeadbeef, th=3, tw=5, first_syms=[t % 6 for t in range(9)], streams=streams)


def _resealed(body):
    return bytes(body) + struct.pack('<I', zlib.crc32(bytes(body)) & 0xffffffff)


def _offsets(f):
    """byte offsets of th, ntiles, the table and the payload length in a format-2 file of fields f"""
    th = 6 + 2 + len(f['ae_name']) + 2 + len(f['pc_name']) + 8 + 10 + 2 + 8 + 4
    table = th + 4 + 4
    return th, th + 4, table, table + 6 * len(f['streams'])


@pytest.mark.parametrize('h,w,th,tw', [(8, 12, 3, 5), (64, 96, 16, 16), (5, 7, 16, 16), (1, 1, 1, 1)])
def test_tile_grid(h, w, th, tw):
    from imgcomp_cvpr_amd import codec
    grid = codec.tile_grid(h, w, th, tw)
    assert len(grid) == -(-h // th) * -(-w // tw)
    cover = np.zeros((h, w), np.int64)
    for y0, x0, a, b in grid:
        assert 1 <= a <= th and 1 <= b <= tw and y0 % th == 0 and x0 % tw == 0
        cover[y0:y0 + a, x0:x0 + b] += 1
    assert (cover == 1).all(), 'every latent position in exactly one tile'
    assert grid == sorted(grid), 'raster order'
    # edge sizes: only the last row / column is smaller, by exactly the remainder
    for y0, x0, a, b in grid:
        assert a == (th if y0 + th <= h else h - y0) and b == (tw if x0 + tw <= w else w - x0)
    if (h, w, th, tw) == (8, 12, 3, 5):
        assert grid == [(0, 0, 3, 5), (0, 5, 3, 5), (0, 10, 3, 2), (3, 0, 3, 5), (3, 5, 3, 5), (3, 10, 3, 2),
                        (6, 0, 2, 5), (6, 5, 2, 5), (6, 10, 2, 2)]
    if (h, w, th, tw) == (5, 7, 16, 16):
        assert grid == [(0, 0, 5, 7)]
    for bad in ((0, 4, 1, 1), (4, 4, 0, 1), (4, 4, 1, 0)):
        with pytest.raises(ValueError):
            codec.tile_grid(*bad)


def test_tiled_container_round_trip():
    from imgcomp_cvpr_amd import codec
    f = _fields()
    data = codec.build_tiled_container(**f)
    c = codec.parse_container(data)
    assert isinstance(c, codec.TiledContainer) and c.version == codec.FORMAT_VERSION_TILED == 2
    for k, v in f.items():
        assert getattr(c, k) == v, k
    assert c.payload == b''.join(f['streams'])
    assert data[:4] == b'ICVF' and struct.unpack('<I', data[-4:])[0] == zlib.crc32(data[:-4])
    th, nt, table, plen = _offsets(f)
    assert struct.unpack_from('<HHI', data, th) == (3, 5, 9)
    assert struct.unpack_from('<HI', data, table + 6) == (1, len(f['streams'][1]))
    assert struct.unpack_from('<Q', data, plen)[0] == len(c.payload) == len(data) - 4 - plen - 8
    # one tile with an empty stream is a legal file
    e = codec.parse_container(codec.build_tiled_container(**dict(f, th=8, tw=12, first_syms=[5], streams=[b''])))
    assert e.streams == [b''] and e.first_syms == [5] and e.payload == b''


def test_format_1_still_parses_and_version_3_is_refused():
    from imgcomp_cvpr_amd import codec
    v1 = codec.build_container('cvpr/low', 'cvpr/res_shallow', 61, 93, 32, 8, 12, 6, 3, 1e9, 0xdeadbeef, b'\x12\x34\x56\x80')
    c = codec.parse_container(v1)
    assert isinstance(c, codec.Container) and c.version == codec.FORMAT_VERSION == 1 and c.first_sym == 3
    for data in (v1, codec.build_tiled_container(**_fields())):
        body = bytearray(data[:-4])
        body[4:6] = struct.pack('<H', 3)
        with pytest.raises(ValueError, match='unsupported format version 3'):
            codec.parse_container(_resealed(body))


def test_tiled_container_refuses_every_flip_and_truncation():
    from imgcomp_cvpr_amd import codec
    data = codec.build_tiled_container(**_fields())
    for pos in range(len(data)):
        for bit in (0x01, 0x40):
            bad = bytearray(data)
            bad[pos] ^= bit
            with pytest.raises(ValueError, match='magic|version|CRC|truncated'):
                codec.parse_container(bytes(bad))
    for n in range(len(data)):
        with pytest.raises(ValueError, match='magic|version|CRC|truncated'):
            codec.parse_container(data[:n])
    with pytest.raises(ValueError, match='truncated|CRC'):
        codec.parse_container(data + b'\x00')


def test_tiled_container_refuses_lies_under_a_correct_crc():
    from imgcomp_cvpr_amd import codec
    f = _fields()
    good = codec.build_tiled_container(**f)
    th, nt, table, plen = _offsets(f)

    def patched(off, fmt, *vals):
        body = bytearray(good[:-4])
        struct.pack_into(fmt, body, off, *vals)
        return _resealed(body)

    for ntiles in (0, 8, 10, 1 << 20, 0xffffffff):              # 2^32 - 1: refused by arithmetic, nothing of that size is built
        with pytest.raises(ValueError, match='tile count {}'.format(ntiles)):
            codec.parse_container(patched(nt, '<I', ntiles))
    with pytest.raises(ValueError, match='tile extent 0 x 5'):
        codec.parse_container(patched(th, '<H', 0))
    with pytest.raises(ValueError, match='tile extent 3 x 0'):
        codec.parse_container(patched(th + 2, '<H', 0))
    # a tile extent that gives another grid than the table has: the count no longer fits
    with pytest.raises(ValueError, match='tile count 9'):
        codec.parse_container(patched(th, '<H', 4))
    # a huge volume whose grid count happens to equal a huge ntiles: the table is checked against the bytes that are there
    body = bytearray(good[:-4])
    struct.pack_into('<II', body, th - 4 - 8 - 2 - 8, 60000, 60000)         # h, w
    struct.pack_into('<HHI', body, th, 1, 1, 3600000000)
    with pytest.raises(ValueError, match='truncated'):
        codec.parse_container(_resealed(body))
    with pytest.raises(ValueError, match='stream lengths'):
        codec.parse_container(patched(table + 6 * 4 + 2, '<I', len(f['streams'][4]) + 1))
    with pytest.raises(ValueError, match='stream lengths'):
        codec.parse_container(patched(plen, '<Q', 1 << 40))
    with pytest.raises(ValueError, match='first symbol 6 of tile 7'):
        codec.parse_container(patched(table + 6 * 7, '<H', 6))
    # lengths that agree with each other but not with the file
    body = bytearray(good[:-4])
    struct.pack_into('<I', body, table + 2, len(f['streams'][0]) + 3)
    struct.pack_into('<Q', body, plen, len(b''.join(f['streams'])) + 3)
    with pytest.raises(ValueError, match='payload length'):
        codec.parse_container(_resealed(body))
    with pytest.raises(ValueError, match='payload length'):
        codec.parse_container(_resealed(bytes(good[:-4]) + b'\x00\x00'))


def test_model_checks_for_a_tiled_container(configs, syn_weights):
    """check_container on a TiledContainer: the same model checks as for version 1, without a device."""
    from imgcomp_cvpr_amd import codec

    class _Pred(object):
        freqs_resolution = 1e9
    shell = codec.Codec.__new__(codec.Codec)
    shell.ae_name, shell.pc_name, shell.fingerprint, shell.C, shell.L, shell.factor, shell.pred = 'cvpr/low', 'cvpr/res_shallow', 7, 32, 6, 8, _Pred()
    good = dict(_fields(), fingerprint=7)
    shell.check_container(codec.parse_container(codec.build_tiled_container(**good)))
    one = dict(th=16, tw=16, first_syms=[0], streams=[b''])
    for change, word in ((dict(fingerprint=8), 'fingerprint'), (dict(ae_name='cvpr/hi'), 'config'), (dict(pc_name='x'), 'config'),
                         (dict(C=16), 'C = 16'), (dict(L=12), 'L = 12'), (dict(one, h=9), 'symbol volume'),
                         (dict(one, w=13), 'symbol volume'), (dict(H=0), 'image size'), (dict(resolution=2e9), 'resolution')):
        with pytest.raises(ValueError, match=word):
            shell.check_container(codec.parse_container(codec.build_tiled_container(**dict(good, **change))))
    # a first symbol that is below the file's L but not below the model's is caught by the L check; one at the file's L by the parser
    with pytest.raises(ValueError, match='first symbol'):
        codec.parse_container(codec.build_tiled_container(**dict(good, first_syms=[0] * 8 + [6])))
    with pytest.raises(ValueError, match='outside 1 .. 65535'):
        codec.Codec(None, None, None, tile=(0, 16))


def test_cli_refuses_a_tile_that_is_no_multiple_of_the_factor_in_the_parser():
    """the argument exists and is an integer; the multiple-of-factor check needs the model and is a GPU test"""
    from imgcomp_cvpr_amd import codec
    with pytest.raises(SystemExit):
        codec.main(['compress', 'a', 'b', '--tile', 'big'])


# ---- ic_pc_decode_tiles_f32: the argument checks run on the host, before any device call -------------------------------------

IC_ERR_ARG, IC_ERR_UNSUPPORTED, IC_ERR_WORKSPACE = -1, -2, -3


def _call(tiles, total_bytes=100, C=4, h=8, w=12, k=24, L=6, workspace_bytes=None, ntiles=None, null=None):
    """the ABI with pointers that are never followed on a refused call: distinct non-null host addresses"""
    from imgcomp_cvpr_amd import _lib
    keep = ctypes.create_string_buffer(64)
    p = ctypes.addressof(keep)
    table = _lib.tile_table(tiles) if tiles else None
    n = len(tiles) if ntiles is None else ntiles
    th_max = max([t[2] for t in tiles if t[2] > 0] or [1])
    tw_max = max([t[3] for t in tiles if t[3] > 0] or [1])
    need = _lib.lib.ic_pc_decode_tiles_workspace_bytes(C, th_max, tw_max, max(n, 1), k)
    args = dict(bits=p, tiles=table, wtab=_lib.ptr_table([None] * 9), centers=p + 8, symbols=p + 16, status=p + 24, ws=p + 32)
    if null:
        args[null] = None
    return _lib.lib.ic_pc_decode_tiles_f32(args['bits'], total_bytes, args['tiles'], n, args['wtab'], args['centers'], k, L, 1e9,
                                           args['symbols'], args['status'], C, h, w, args['ws'],
                                           need if workspace_bytes is None else workspace_bytes, 0, None)


def test_decode_tiles_refuses_bad_descriptors_on_the_host():
    good = (3, 5, 3, 5, 10, 20, 2)                             # y0, x0, th, tw, stream_off, stream_bytes, first_sym
    for what, tile in (('th = 0', (3, 5, 0, 5, 10, 20, 2)), ('tw = 0', (3, 5, 3, 0, 10, 20, 2)), ('th < 0', (3, 5, -3, 5, 10, 20, 2)),
                       ('y0 < 0', (-1, 5, 3, 5, 10, 20, 2)), ('x0 < 0', (3, -1, 3, 5, 10, 20, 2)),
                       ('y0 + th > h', (6, 5, 3, 5, 10, 20, 2)), ('x0 + tw > w', (3, 8, 3, 5, 10, 20, 2)),
                       ('y0 + th overflows int', (2 ** 31 - 1, 5, 3, 5, 10, 20, 2)),
                       ('stream_off < 0', (3, 5, 3, 5, -1, 20, 2)), ('stream_bytes < 0', (3, 5, 3, 5, 10, -1, 2)),
                       ('stream beyond the end', (3, 5, 3, 5, 90, 11, 2)), ('stream_off beyond the end', (3, 5, 3, 5, 101, 0, 2)),
                       ('off + bytes overflows', (3, 5, 3, 5, 2 ** 62, 2 ** 62, 2)),
                       ('first_sym = L', (3, 5, 3, 5, 10, 20, 6)), ('first_sym < 0', (3, 5, 3, 5, 10, 20, -1))):
        # the bad descriptor last: the good ones before it do not let it through
        assert _call([good, good, tile]) == IC_ERR_ARG, what
        assert _call([tile]) == IC_ERR_ARG, what
    assert _call([good], ntiles=0) == IC_ERR_ARG
    assert _call([good], total_bytes=-1) == IC_ERR_ARG
    for null in ('bits', 'tiles', 'centers', 'symbols', 'status', 'ws'):
        assert _call([good], null=null) == IC_ERR_ARG, null
    assert _call([good], L=17) == IC_ERR_UNSUPPORTED
    # a stream that ends exactly at the end of the buffer, and an empty one at the very end, are legal descriptors: they get as far
    # as the workspace check
    for tile in ((3, 5, 3, 5, 90, 10, 2), (3, 5, 3, 5, 100, 0, 2), (0, 0, 8, 12, 0, 100, 5)):
        assert _call([tile], workspace_bytes=0) == IC_ERR_WORKSPACE


@pytest.mark.parametrize('k', [24, 64])
def test_decode_tiles_short_workspace(k):
    from imgcomp_cvpr_amd import _lib
    tiles = [(0, 0, 3, 5, 0, 10, 0), (3, 0, 5, 12, 10, 10, 0)]           # the workspace follows the largest th and the largest tw
    need = _lib.lib.ic_pc_decode_tiles_workspace_bytes(4, 5, 12, 2, k)
    assert need > 0
    for short in (0, 1, need // 2, need - 1):
        assert _call(tiles, k=k, workspace_bytes=short) == IC_ERR_WORKSPACE, short


def test_decode_tiles_workspace_bytes():
    """pure host arithmetic: 0 for a non-positive argument, monotone in each extent (C, th_max, tw_max, ntiles) for every k.
    k is not an extent: it selects the code path (24: one slot per tile; 24 and 64: the matrix-core forms with their packed
    filters, as in ic_pc_workspace_bytes, which this size is built on), so the size is monotone in k within a path only."""
    from imgcomp_cvpr_amd import _lib
    ws = _lib.lib.ic_pc_decode_tiles_workspace_bytes
    base = (32, 16, 16, 24, 24)
    assert ws(*base) > 0
    for i in range(5):
        for v in (0, -1, -(2 ** 31)):
            a = list(base)
            a[i] = v
            assert ws(*a) == 0, a
    for k in (8, 23, 24, 25, 64):
        for i in range(4):
            prev = 0
            for v in (1, 2, 3, 7, 16, 17, 64, 100):
                a = [32, 16, 16, 24, k]
                a[i] = v
                cur = ws(*a)
                assert cur >= prev and cur > 0, (a, cur, prev)
                prev = cur
    for ks in ((1, 2, 8, 16, 23), (25, 32, 48, 63), (65, 80, 100)):
        sizes = [ws(32, 16, 16, 24, k) for k in ks]
        assert sizes == sorted(sizes), (ks, sizes)
    # one slot per tile: the padded volume and the three caches of a (32, 16, 16) tile, about 4 MB
    per_tile = ws(32, 16, 16, 25, 24) - ws(32, 16, 16, 24, 24)
    floats = 36 * 24 * 24 + 24 * (35 * 22 * 22 + 34 * 20 * 20 + 33 * 18 * 18)
    assert 4 * floats <= per_tile <= 4 * floats + 4 * 256 + 256
    # it covers what the single-volume decoder needs for the largest tile (the slow path runs inside it)
    for k in (24, 64):
        assert ws(32, 16, 16, 1, k) >= _lib.lib.ic_pc_decode_workspace_bytes(32, 16, 16, k) + 32 * 16 * 16 * 8


# (C, th, tw, ntiles, nvolumes, k) -> ic_pc_workspace_bytes(1, C, th, tw, k), ic_pc_decode_workspace_bytes(C, th, tw, k),
# ic_pc_decode_tiles_workspace_bytes(C, th, tw, ntiles, k), ic_pc_decode_tiles_batch_workspace_bytes(C, th, tw, ntiles, nvolumes, k),
# recorded from the library before the decoder moved into a source file of its own
PINNED_WORKSPACE_BYTES = {
    (4, 3, 5, 2, 2, 24): (270144, 304992, 305760, 306016),
    (4, 3, 5, 2, 2, 64): (949760, 711680, 712448, 712704),
    (32, 16, 16, 24, 8, 24): (4108800, 4222048, 96996352, 96996608),
    (32, 16, 16, 24, 8, 64): (11186176, 790016, 856576, 856832),
    (1, 1, 1, 1, 1, 24): (178272, 210528, 211040, 211296),
    (1, 1, 1, 1, 1, 64): (704768, 708864, 709376, 709632),
}

# (C, th, tw, ntiles, nvolumes, k, nlayers) -> ic_pc_decode_tiles_batch_<kind>_workspace_bytes of these kinds, in this order; recorded
# from the library while every size function was a sum of its own, before one layout stood behind all of them
SEGMENTED_KINDS = ('layers', 'layers_pertile', 'fronts', 'fronts_pertile', 'layers_resume', 'fronts_resume')
PINNED_SEGMENTED_WORKSPACE_BYTES = {
    (4, 3, 5, 2, 2, 24, 1): (306528, 306784, 306528, 306784, 307296, 307808),
    (4, 3, 5, 2, 2, 24, 4): (306528, 306784, 306528, 306784, 307296, 307808),
    (4, 3, 5, 2, 2, 24, 16): (306784, 307040, 306784, 307040, 307552, 308064),
    (32, 16, 16, 24, 8, 24, 1): (96997376, 96997632, 96997376, 96997632, 96998144, 97194752),
    (32, 16, 16, 24, 8, 24, 4): (96998400, 96998656, 96998400, 96998656, 96999168, 97195776),
    (32, 16, 16, 24, 8, 24, 16): (97003008, 97003264, 97003008, 97003264, 97003776, 97200384),
    (1, 1, 1, 1, 1, 24, 1): (211808, 212064, 211808, 212064, 212576, 212832),
    (1, 1, 1, 1, 1, 24, 4): (211808, 212064, 211808, 212064, 212576, 212832),
    (1, 1, 1, 1, 1, 24, 16): (211808, 212064, 211808, 212064, 212576, 212832),
}


def test_workspace_bytes_pinned():
    """the workspace sizes are ABI: callers allocate by them and the entries lay their workspace out by them, so they are what
    they were -- byte for byte, for both k paths, a small ragged shape, the 24-tile Kodak shape and the smallest volume"""
    from imgcomp_cvpr_amd import _lib
    lib = _lib.lib
    for (C, th, tw, ntiles, nvolumes, k), want in PINNED_WORKSPACE_BYTES.items():
        got = (lib.ic_pc_workspace_bytes(1, C, th, tw, k), lib.ic_pc_decode_workspace_bytes(C, th, tw, k),
               lib.ic_pc_decode_tiles_workspace_bytes(C, th, tw, ntiles, k),
               lib.ic_pc_decode_tiles_batch_workspace_bytes(C, th, tw, ntiles, nvolumes, k))
        assert got == want, ((C, th, tw, ntiles, nvolumes, k), got, want)
    for (C, th, tw, ntiles, nvolumes, k, nlayers), want in PINNED_SEGMENTED_WORKSPACE_BYTES.items():
        got = tuple(getattr(lib, 'ic_pc_decode_tiles_batch_{}_workspace_bytes'.format(kind))(C, th, tw, ntiles, nvolumes, k, nlayers)
                    for kind in SEGMENTED_KINDS)
        assert got == want, ((C, th, tw, ntiles, nvolumes, k, nlayers), got, want)
        for none in (0, 17):                                 # no such number of layers: no size
            got = tuple(getattr(lib, 'ic_pc_decode_tiles_batch_{}_workspace_bytes'.format(kind))(C, th, tw, ntiles, nvolumes, k, none)
                        for kind in SEGMENTED_KINDS)
            assert got == (0,) * len(SEGMENTED_KINDS), ((C, th, tw, ntiles, nvolumes, k, none), got)
