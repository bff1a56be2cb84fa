"""No GPU: the host side of the batch codec -- the two descriptor tables of ic_pc_decode_tiles_batch_f32 and the checks that decide
everything about them before the first device call, the chunking arithmetic of decode_tiles_batch as a pure function, and the
directory listing / argument checks of the compress-dir and decompress-dir commands."""
import argparse
import ctypes
import os
import random

import pytest

IC_ERR_ARG, IC_ERR_UNSUPPORTED, IC_ERR_WORKSPACE = -1, -2, -3


# ---- the tables ---------------------------------------------------------------------------------------------------------------

def test_tile_and_volume_table_layout():
    """ic_pc_tile_t keeps its size and field offsets: `volume` sits where `reserved` sat, 0 unless the caller names one"""
    from imgcomp_cvpr_amd import _lib
    T, V = _lib.PcTile, _lib.PcVolume
    assert ctypes.sizeof(T) == 40
    assert [(n, getattr(T, n).offset, getattr(T, n).size) for n, _ in T._fields_] == [
        ('y0', 0, 4), ('x0', 4, 4), ('th', 8, 4), ('tw', 12, 4), ('stream_off', 16, 8), ('stream_bytes', 24, 8),
        ('first_sym', 32, 4), ('volume', 36, 4)]
    assert ctypes.sizeof(V) == 24
    assert [(n, getattr(V, n).offset, getattr(V, n).size) for n, _ in V._fields_] == [
        ('h', 0, 4), ('w', 4, 4), ('symbols_off', 8, 8), ('q_off', 16, 8)]
    t = _lib.tile_table([(1, 2, 3, 4, 5, 6, 7), (8, 9, 10, 11, 2 ** 40, 2 ** 41, 12, 3)])
    assert ctypes.sizeof(t) == 80
    assert [t[0].y0, t[0].x0, t[0].th, t[0].tw, t[0].stream_off, t[0].stream_bytes, t[0].first_sym, t[0].volume] == [1, 2, 3, 4, 5, 6, 7, 0]
    assert [t[1].stream_off, t[1].stream_bytes, t[1].first_sym, t[1].volume] == [2 ** 40, 2 ** 41, 12, 3]
    raw = bytes(t)
    assert int.from_bytes(raw[36:40], 'little') == 0 and int.from_bytes(raw[76:80], 'little') == 3
    v = _lib.volume_table([(8, 12, 0, 100), (3, 5, 2 ** 40, 7)])
    assert [(x.h, x.w, x.symbols_off, x.q_off) for x in v] == [(8, 12, 0, 100), (3, 5, 2 ** 40, 7)]


def test_packed_volume_table():
    from imgcomp_cvpr_amd import _lib
    v, offs, total = _lib.packed_volume_table([(32, 8, 12), (32, 64, 96), (32, 1, 1)])
    assert offs == [0, 32 * 8 * 12, 32 * 8 * 12 + 32 * 64 * 96] and total == offs[2] + 32
    assert [(x.h, x.w, x.symbols_off, x.q_off) for x in v] == [(8, 12, offs[0], offs[0]), (64, 96, offs[1], offs[1]), (1, 1, offs[2], offs[2])]


# ---- ic_pc_decode_tiles_batch_f32: the argument checks run on the host, before any device call --------------------------------

VOLS = [(8, 12, 0, 0), (16, 6, 4 * 8 * 12, 4 * 8 * 12)]            # h, w, symbols_off, q_off: two volumes of C = 4


def _call(tiles, volumes=VOLS, total_bytes=100, C=4, k=24, L=6, workspace_bytes=None, ntiles=None, nvolumes=None, null=()):
    """the ABI with pointers that are never followed on a refused call: distinct non-null host addresses"""
    from imgcomp_cvpr_amd import _lib
    keep = ctypes.create_string_buffer(64)
    p = ctypes.addressof(keep)
    n = len(tiles) if ntiles is None else ntiles
    nv = len(volumes) if nvolumes is None else nvolumes
    th_max = max([t[2] for t in tiles if t[2] > 0] or [1])
    tw_max = max([t[3] for t in tiles if t[3] > 0] or [1])
    need = _lib.lib.ic_pc_decode_tiles_batch_workspace_bytes(C, th_max, tw_max, max(n, 1), max(nv, 1), k)
    args = dict(bits=p, tiles=_lib.tile_table(tiles), volumes=_lib.volume_table(volumes), centers=p + 8, symbols=p + 16, q=p + 20,
                status=p + 24, ws=p + 32)
    for name in ([null] if isinstance(null, str) else null):
        args[name] = None
    return _lib.lib.ic_pc_decode_tiles_batch_f32(args['bits'], total_bytes, args['tiles'], n, args['volumes'], nv,
                                                 _lib.ptr_table([None] * 9), args['centers'], k, L, 1e9, args['symbols'], args['q'],
                                                 args['status'], C, args['ws'], need if workspace_bytes is None else workspace_bytes,
                                                 0, None)


def test_batch_refuses_bad_descriptors_on_the_host():
    good0, good1 = (3, 5, 3, 5, 10, 20, 2, 0), (10, 1, 6, 5, 30, 5, 0, 1)    # y0, x0, th, tw, stream_off, stream_bytes, first_sym, volume
    for what, tile in (('volume = nvolumes', (3, 5, 3, 5, 10, 20, 2, 2)), ('volume < 0', (3, 5, 3, 5, 10, 20, 2, -1)),
                       ('inside volume 1, outside its own volume 0', (10, 1, 6, 5, 30, 5, 0, 0)),
                       ('inside volume 0, outside its own volume 1', (3, 5, 3, 5, 10, 20, 2, 1)),
                       ('th = 0', (3, 5, 0, 5, 10, 20, 2, 0)), ('tw < 0', (3, 5, 3, -5, 10, 20, 2, 1)),
                       ('y0 < 0', (-1, 5, 3, 5, 10, 20, 2, 0)), ('x0 < 0', (3, -1, 3, 5, 10, 20, 2, 0)),
                       ('y0 + th overflows int', (2 ** 31 - 1, 5, 3, 5, 10, 20, 2, 0)),
                       ('stream_off < 0', (3, 5, 3, 5, -1, 20, 2, 0)), ('stream beyond the end', (3, 5, 3, 5, 90, 11, 2, 0)),
                       ('off + bytes overflows', (3, 5, 3, 5, 2 ** 62, 2 ** 62, 2, 0)),
                       ('first_sym = L', (3, 5, 3, 5, 10, 20, 6, 0)), ('first_sym < 0', (3, 5, 3, 5, 10, 20, -1, 0))):
        assert _call([good0, good1, tile]) == IC_ERR_ARG, what
        assert _call([tile]) == IC_ERR_ARG, what
    for what, vols in (('h = 0', [(0, 12, 0, 0), VOLS[1]]), ('w < 0', [VOLS[0], (16, -6, 0, 0)]),
                       ('symbols_off < 0', [(8, 12, -1, 0), VOLS[1]]), ('q_off < 0', [VOLS[0], (16, 6, 0, -1)])):
        assert _call([good0, good1], volumes=vols) == IC_ERR_ARG, what
    assert _call([good0], ntiles=0) == IC_ERR_ARG
    assert _call([good0], nvolumes=0) == IC_ERR_ARG
    assert _call([good0, good1], nvolumes=1) == IC_ERR_ARG               # the second tile's volume is outside the shorter table
    assert _call([good0], total_bytes=-1) == IC_ERR_ARG
    for null in ('bits', 'tiles', 'volumes', 'centers', 'status', 'ws', ('symbols', 'q')):
        assert _call([good0, good1], null=null) == IC_ERR_ARG, null
    assert _call([good0], L=17) == IC_ERR_UNSUPPORTED
    # legal tables get as far as the workspace check, with either output alone as well
    for null in ((), 'symbols', 'q'):
        assert _call([good0, good1], workspace_bytes=0, null=null) == IC_ERR_WORKSPACE, null


@pytest.mark.parametrize('k', [24, 64])
def test_batch_short_workspace(k):
    from imgcomp_cvpr_amd import _lib
    tiles = [(0, 0, 3, 5, 0, 10, 0, 0), (3, 0, 5, 6, 10, 10, 0, 1)]
    need = _lib.lib.ic_pc_decode_tiles_batch_workspace_bytes(4, 5, 6, 2, 2, k)
    assert need > _lib.lib.ic_pc_decode_tiles_workspace_bytes(4, 5, 6, 2, k) > 0         # the volume table is in it
    for short in (0, 1, need // 2, need - 1):
        assert _call(tiles, k=k, workspace_bytes=short) == IC_ERR_WORKSPACE, short
    ws = _lib.lib.ic_pc_decode_tiles_batch_workspace_bytes
    for i in range(6):
        a = [32, 16, 16, 24, 4, k]
        a[i] = 0
        assert ws(*a) == 0, a
    assert ws(32, 16, 16, 48, 8, k) >= ws(32, 16, 16, 24, 8, k) >= ws(32, 16, 16, 24, 4, k)


# ---- chunking -----------------------------------------------------------------------------------------------------------------

def _check_chunks(shapes, need, budget):
    from imgcomp_cvpr_amd import codec
    chunks = codec.chunk_tiles(shapes, need, budget)
    assert chunks[0][0] == 0 and chunks[-1][1] == len(shapes)
    for (a, b), (c, d) in zip(chunks, chunks[1:]):
        assert b == c                                                     # every tile in exactly one chunk, order kept
    for a, b in chunks:
        assert b > a
        used = need(max(s[0] for s in shapes[a:b]), max(s[1] for s in shapes[a:b]), b - a)
        assert used <= budget, (a, b, used, budget)
        if b < len(shapes):                                               # greedy: the next tile would not have fitted
            assert need(max(s[0] for s in shapes[a:b + 1]), max(s[1] for s in shapes[a:b + 1]), b + 1 - a) > budget
    return chunks


def test_chunk_tiles_with_a_linear_cost():
    need = lambda th, tw, n: 100 + n * th * tw
    shapes = [(16, 16)] * 24 + [(16, 9), (9, 16), (9, 9)] + [(3, 5)] * 9
    assert _check_chunks(shapes, need, 10 ** 9) == [(0, len(shapes))]
    assert _check_chunks(shapes, need, 100 + 256) == [(i, i + 1) for i in range(26)] + [(26, 29), (29, 36)]
    # 5 tiles of 16 x 16 per chunk (the fifth chunk ends with the 16 x 9 tile), then 8 tiles at 9 x 16, then the last three
    assert _check_chunks(shapes, need, 100 + 5 * 256) == [(0, 5), (5, 10), (10, 15), (15, 20), (20, 25), (25, 33), (33, 36)]
    rng = random.Random(4)
    for _ in range(50):
        shapes = [(rng.randint(1, 16), rng.randint(1, 16)) for _ in range(rng.randint(1, 60))]
        _check_chunks(shapes, need, rng.randint(100 + 256, 100 + 40 * 256))
    from imgcomp_cvpr_amd import codec
    assert codec.chunk_tiles([], need, 1) == []
    with pytest.raises(ValueError, match='tile 2 of 16 x 16 needs a workspace of 356 bytes, the budget is 355'):
        codec.chunk_tiles([(3, 5), (3, 5), (16, 16)], need, 355)


def test_chunk_tiles_with_the_library_cost():
    """the workspace query of the ABI is the cost decode_tiles_batch chunks by: 8 Kodak-sized files at 16 x 16 tiles under 2 GiB"""
    from imgcomp_cvpr_amd import _lib
    need = lambda th, tw, n: int(_lib.lib.ic_pc_decode_tiles_batch_workspace_bytes(32, th, tw, n, 8, 24))
    shapes = [(16, 16)] * (8 * 24)
    assert need(16, 16, 1) < 8 << 20
    assert _check_chunks(shapes, need, 1 << 31) == [(0, 192)]
    chunks = _check_chunks(shapes, need, 100 << 20)
    assert len(chunks) >= 8 and sum(b - a for a, b in chunks) == 192
    from imgcomp_cvpr_amd import codec
    with pytest.raises(ValueError, match='budget'):
        codec.chunk_tiles(shapes, need, need(16, 16, 1) - 1)


# ---- compress-dir / decompress-dir --------------------------------------------------------------------------------------------

def _touch(d, names):
    for n in names:
        with open(os.path.join(str(d), n), 'wb') as f:
            f.write(b'x')


def test_list_dir_jobs(tmp_path):
    from imgcomp_cvpr_amd import codec
    src, dst = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    _touch(src, ['b.png', 'a.jpg', 'C.PNG', 'notes.txt', 'd.icf', 'e.jpeg.bak'])
    (src / 'sub.png').mkdir()                                           # a directory is no image
    jobs = codec.list_dir_jobs(str(src), str(dst), 'compress-dir')
    assert jobs == [(str(src / n), str(dst / o)) for n, o in (('C.PNG', 'C.icf'), ('a.jpg', 'a.icf'), ('b.png', 'b.icf'))]
    assert codec.list_dir_jobs(str(src), str(dst), 'decompress-dir') == [(str(src / 'd.icf'), str(dst / 'd.png'))]
    assert not dst.exists()                                             # listing creates nothing
    _touch(src, ['a.png'])
    with pytest.raises(ValueError, match='a.jpg and a.png would both be written to a.icf'):
        codec.list_dir_jobs(str(src), str(dst), 'compress-dir')
    with pytest.raises(ValueError, match='is not a directory'):
        codec.list_dir_jobs(str(src / 'nowhere'), str(dst), 'compress-dir')
    empty = tmp_path / 'empty'
    empty.mkdir()
    with pytest.raises(ValueError, match=r'no \*.png / \*.jpg file'):
        codec.list_dir_jobs(str(empty), str(dst), 'compress-dir')
    with pytest.raises(ValueError, match=r'no \*.icf file'):
        codec.list_dir_jobs(str(empty), str(dst), 'decompress-dir')


def test_dir_argument_errors_need_no_device(tmp_path, capsys):
    """main() refuses these before a model is built: exit code 2, the cause on stderr, nothing written"""
    from imgcomp_cvpr_amd import codec
    src, dst = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    _touch(src, ['a.png'])
    for args, msg in ((['compress-dir', str(src), str(dst), '--tile', '100'], 'multiple of the subsampling factor 8'),
                      (['compress-dir', str(src), str(dst), '--tile', '0'], 'multiple of the subsampling factor 8'),
                      (['compress-dir', str(src), str(dst), '--batch', '0'], '--batch 0 is not at least 1'),
                      (['decompress-dir', str(src), str(dst), '--tile', '128'], '--tile belongs to compress'),
                      (['decompress-dir', str(src), str(dst)], 'no *.icf file'),
                      (['compress-dir', str(tmp_path / 'nowhere'), str(dst)], 'is not a directory'),
                      (['compress-dir', str(src), str(src / 'a.png')], 'exists and is not a directory'),
                      (['compress-dir', str(src), str(dst), '--ae_config', 'cvpr/none'], 'not found')):
        assert codec.main(args + ['--device', 'no-such-device']) == 2, args
        assert msg in capsys.readouterr().err, args
    assert not dst.exists()
    with pytest.raises(SystemExit):
        codec.main(['compress-dir', str(src), str(dst), '--batch', 'many'])
    flags = argparse.Namespace(command='compress-dir', input=str(src), output=str(dst), tile=128, batch=3)
    assert codec.check_dir_args(flags, 8) == ([(str(src / 'a.png'), str(dst / 'a.icf'))], (16, 16))
    flags.tile = None
    assert codec.check_dir_args(flags, 8)[1] is None
