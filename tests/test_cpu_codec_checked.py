"""Checked tiles (container format 4), the parts that need no GPU: the container and its two readers (strict: parse_container,
salvage: parse_salvage), the verify command, the option checks of the command line, the NumPy statement of the concealment rule
on hand-made cases, and the host-side argument checks of ic_pc_conceal_tiles."""
import ctypes
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fields(streams=(b'\x12\x34', b'', b'\x80', b'\x01\x02\x03', b'\xff', b'\x10\x20')):
    # the 8 x 12 latent plane of a 61 x 93 image cut into 3 x 5 tiles: 9 tiles, streams of different lengths, one empty
    streams = list(streams) + [bytes([i + 1]) * (i + 1) for i in range(9 - len(streams))]
    return dict(ae_name='cvpr/low', pc_name='cvpr/res_shallow', H=61, W=93, C=32, h=8, w=12, L=6, resolution=1e9,
                fingerprint=0xdeadbeef, th=3, tw=5, first_syms=[t % 6 for t in range(9)], streams=streams)


def _resealed(body):
    return bytes(body) + struct.pack('<I', zlib.crc32(bytes(body)) & 0xffffffff)


def _offsets(f):
    """byte offsets in a format-4 file of fields f: th, ntiles, the table, the payload length, the header CRC, the payload"""
    th = 6 + 2 + len(f['ae_name']) + 2 + len(f['pc_name']) + 8 + 10 + 2 + 8 + 4
    table = th + 4 + 4
    plen = table + 10 * len(f['streams'])
    return th, th + 4, table, plen, plen + 8, plen + 12


def _reheaded(body, f):
    """body (without the file CRC) with the header CRC recomputed, then resealed: a lie under two correct CRCs"""
    body = bytearray(body)
    hcrc = _offsets(f)[4]
    struct.pack_into('<I', body, hcrc, zlib.crc32(bytes(body[:hcrc])) & 0xffffffff)
    return _resealed(body)


def _owner(f):
    """payload byte -> the tile that owns it"""
    return [t for t, b in enumerate(f['streams']) for _ in b]


# ---- the container and the strict reader --------------------------------------------------------------------------------------

def test_checked_container_round_trip_and_size():
    from imgcomp_cvpr_amd import codec
    f = _fields()
    data, v2 = codec.build_checked_container(**f), codec.build_tiled_container(**f)
    assert codec.FORMAT_VERSION_CHECKED == 4
    assert len(data) == len(v2) + 4 * len(f['streams']) + 4
    c, c2 = codec.parse_container(data), codec.parse_container(v2)
    assert isinstance(c, codec.CheckedContainer) and c.version == 4 and not isinstance(c, codec.TiledContainer)
    assert codec.CheckedContainer._fields == codec.TiledContainer._fields + ('stream_crcs',)
    for k, v in f.items():
        assert getattr(c, k) == v, k
    assert c.streams == c2.streams and c.payload == c2.payload == b''.join(f['streams']) and c.first_syms == c2.first_syms
    assert c.stream_crcs == [zlib.crc32(b) & 0xffffffff for b in f['streams']]
    th, nt, table, plen, hcrc, payload = _offsets(f)
    assert struct.unpack_from('<H', data, 4)[0] == 4 and struct.unpack_from('<HHI', data, th) == (3, 5, 9)
    assert struct.unpack_from('<HII', data, table + 10 * 3) == (3, 3, zlib.crc32(b'\x01\x02\x03'))
    assert struct.unpack_from('<Q', data, plen)[0] == len(c.payload)
    assert struct.unpack_from('<I', data, hcrc)[0] == zlib.crc32(data[:hcrc])
    assert data[payload:-4] == c.payload and struct.unpack('<I', data[-4:])[0] == zlib.crc32(data[:-4])
    # everything before the tile table is the format-2 header with another version word
    assert data[6:table] == v2[6:table]
    # one tile with an empty stream is a legal file
    one = dict(f, th=8, tw=12, first_syms=[5], streams=[b''])
    e = codec.parse_container(codec.build_checked_container(**one))
    assert e.streams == [b''] and e.first_syms == [5] and e.payload == b'' and e.stream_crcs == [0]
    s, damage, ok = codec.parse_salvage(codec.build_checked_container(**one))
    assert s == e and damage == [] and ok is True


def test_version_3_stays_refused_and_the_message_names_4():
    from imgcomp_cvpr_amd import codec
    body = bytearray(codec.build_checked_container(**_fields())[:-4])
    body[4:6] = struct.pack('<H', 3)
    with pytest.raises(ValueError, match=r'unsupported format version 3 \(this codec reads versions 1, 2 and 4\)'):
        codec.parse_container(_resealed(body))
    with pytest.raises(ValueError, match='unsupported format version 3'):
        codec.parse_salvage(_resealed(body))


def test_strict_reader_refuses_every_flip_and_truncation():
    from imgcomp_cvpr_amd import codec
    data = codec.build_checked_container(**_fields())
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


def test_strict_reader_names_the_inner_crc_that_fails():
    """a damaged byte under a recomputed file CRC: the header CRC or the tile's stream CRC refuses it, the tile by name"""
    from imgcomp_cvpr_amd import codec
    f = _fields()
    good = codec.build_checked_container(**f)
    th, nt, table, plen, hcrc, payload = _offsets(f)
    owner = _owner(f)
    for i, t in enumerate(owner):
        body = bytearray(good[:-4])
        body[payload + i] ^= 0x10
        with pytest.raises(ValueError, match='stream CRC mismatch in tile {}:'.format(t)):
            codec.parse_container(_resealed(body))
    for pos in (6, th - 3, table + 7, plen + 1, hcrc):
        body = bytearray(good[:-4])
        body[pos] ^= 0x01
        with pytest.raises(ValueError):
            codec.parse_container(_resealed(body))
    body = bytearray(good[:-4])
    body[th - 8] ^= 0x01                                  # inside `resolution`: no length, no count -- only the header CRC can tell
    with pytest.raises(ValueError, match='header CRC mismatch'):
        codec.parse_container(_resealed(body))


def test_both_readers_refuse_lies_under_correct_crcs():
    from imgcomp_cvpr_amd import codec
    f = _fields()
    good = codec.build_checked_container(**f)
    th, nt, table, plen, hcrc, payload = _offsets(f)

    def patched(off, fmt, *vals):
        body = bytearray(good[:-4])
        struct.pack_into(fmt, body, off, *vals)
        return _reheaded(body, f)

    readers = (codec.parse_container, codec.parse_salvage)
    for read in readers:
        for ntiles in (0, 8, 10, 1 << 20, 0xffffffff):          # 2^32 - 1: refused by arithmetic, nothing of that size is built
            with pytest.raises(ValueError, match='tile count {}'.format(ntiles)):
                read(patched(nt, '<I', ntiles))
        with pytest.raises(ValueError, match='tile extent 0 x 5'):
            read(patched(th, '<H', 0))
        with pytest.raises(ValueError, match='tile extent 3 x 0'):
            read(patched(th + 2, '<H', 0))
        with pytest.raises(ValueError, match='tile count 9'):
            read(patched(th, '<H', 4))
        # a huge volume whose grid count equals a huge ntiles: the table is checked against the bytes that are there
        body = bytearray(good[:-4])
        struct.pack_into('<II', body, th - 4 - 8 - 2 - 8, 60000, 60000)         # h, w
        struct.pack_into('<HHI', body, th, 1, 1, 3600000000)
        with pytest.raises(ValueError, match='truncated'):
            read(_resealed(body))
        with pytest.raises(ValueError, match='stream lengths'):
            read(patched(table + 10 * 4 + 2, '<I', len(f['streams'][4]) + 1))
        with pytest.raises(ValueError, match='stream lengths'):
            read(patched(plen, '<Q', 1 << 40))
        with pytest.raises(ValueError, match='first symbol 6 of tile 7'):
            read(patched(table + 10 * 7, '<H', 6))
    # lengths that agree with each other but not with the file: the strict reader refuses, the salvage reader calls the last
    # tile truncated
    body = bytearray(good[:-4])
    struct.pack_into('<I', body, table + 10 * 8 + 2, len(f['streams'][8]) + 3)
    struct.pack_into('<Q', body, plen, len(b''.join(f['streams'])) + 3)
    with pytest.raises(ValueError, match='payload length'):
        codec.parse_container(_reheaded(body, f))
    with pytest.raises(ValueError, match='payload length'):
        codec.parse_container(_resealed(bytes(good[:-4]) + b'\x00\x00'))
    c, damage, ok = codec.parse_salvage(_reheaded(body, f)[:-4])
    assert damage == [(8, 'truncated')] and ok is False and c.streams[:8] == f['streams'][:8]


# ---- the salvage reader, exhaustively on the small file ----------------------------------------------------------------------

def test_salvage_reader_on_an_intact_file():
    from imgcomp_cvpr_amd import codec
    data = codec.build_checked_container(**_fields())
    c, damage, ok = codec.parse_salvage(data)
    assert c == codec.parse_container(data) and damage == [] and ok is True
    # bytes behind the declared end are ignored
    c2, damage, ok = codec.parse_salvage(data + b'trailing')
    assert c2 == c and damage == [] and ok is True


def test_salvage_reader_every_payload_flip_damages_exactly_its_tile():
    from imgcomp_cvpr_amd import codec
    f = _fields()
    data = codec.build_checked_container(**f)
    payload = _offsets(f)[5]
    owner = _owner(f)
    assert len(owner) == len(data) - 4 - payload and set(owner) == set(range(9)) - {1}
    for i, t in enumerate(owner):
        for bit in (0x01, 0x40):
            bad = bytearray(data)
            bad[payload + i] ^= bit
            c, damage, ok = codec.parse_salvage(bytes(bad))
            assert damage == [(t, 'crc')] and ok is False, (i, t, damage)
            assert c.streams == [None if u == t else b for u, b in enumerate(f['streams'])]
            assert c.first_syms == f['first_syms'] and c.stream_crcs == [zlib.crc32(b) & 0xffffffff for b in f['streams']]


def test_salvage_reader_every_header_flip_is_refused():
    from imgcomp_cvpr_amd import codec
    f = _fields()
    data = codec.build_checked_container(**f)
    payload = _offsets(f)[5]
    for pos in range(payload):                             # up to and including the header CRC
        for bit in (0x01, 0x40):
            bad = bytearray(data)
            bad[pos] ^= bit
            with pytest.raises(ValueError, match='header damaged: nothing can be recovered' if pos >= 6 else 'magic|version'):
                codec.parse_salvage(bytes(bad))
    for pos in range(len(data) - 4, len(data)):            # the trailing CRC: nothing is lost
        bad = bytearray(data)
        bad[pos] ^= 0x40
        c, damage, ok = codec.parse_salvage(bytes(bad))
        assert damage == [] and ok is False and c.streams == f['streams']


def test_salvage_reader_every_truncation():
    from imgcomp_cvpr_amd import codec
    f = _fields()
    data = codec.build_checked_container(**f)
    payload = _offsets(f)[5]
    ends, pos = [], 0
    for b in f['streams']:
        pos += len(b)
        ends.append(pos)
    for n in range(payload, len(data)):
        c, damage, ok = codec.parse_salvage(data[:n])
        have = min(n - payload, ends[-1])
        want = [(t, 'truncated') for t, b in enumerate(f['streams']) if b and ends[t] > have]
        assert damage == want and ok is False, (n, damage, want)
        assert c.streams == [None if (t, 'truncated') in want else b for t, b in enumerate(f['streams'])]
    assert codec.parse_salvage(data[:payload])[1] == [(t, 'truncated') for t in range(9) if t != 1]      # the empty stream never
    assert codec.parse_salvage(data[:-4])[1:] == ([], False) and codec.parse_salvage(data[:-1])[1:] == ([], False)
    for n in range(payload):
        with pytest.raises(ValueError, match='truncated|header damaged'):
            codec.parse_salvage(data[:n])
    # an empty stream at the very end is never damaged
    g = _fields()
    g['streams'][8] = b''
    d = codec.build_checked_container(**g)
    for n in range(_offsets(g)[5], len(d)):
        assert 8 not in [t for t, _ in codec.parse_salvage(d[:n])[1]]


def test_salvage_reader_refuses_formats_1_and_2_and_says_why():
    from imgcomp_cvpr_amd import codec
    v1 = codec.build_container('cvpr/low', 'cvpr/res_shallow', 61, 93, 32, 8, 12, 6, 3, 1e9, 0xdeadbeef, b'\x12\x34\x56\x80')
    for version, data in ((1, v1), (2, codec.build_tiled_container(**_fields()))):
        with pytest.raises(ValueError, match='format version {} has nothing to salvage with: one CRC over the whole file'.format(version)):
            codec.parse_salvage(data)


def test_model_checks_and_report_for_a_checked_container(configs):
    """check_container treats a CheckedContainer as a TiledContainer; the report's rectangles, without a device"""
    from imgcomp_cvpr_amd import codec

    class _Pred(object):
        freqs_resolution = 1e9
    shell = codec.Codec.__new__(codec.Codec)
    shell.ae_name, shell.pc_name, shell.fingerprint, shell.C, shell.L, shell.factor, shell.pred = 'cvpr/low', 'cvpr/res_shallow', 7, 32, 6, 8, _Pred()
    good = dict(_fields(), fingerprint=7)
    c = codec.parse_container(codec.build_checked_container(**good))
    shell.check_container(c)
    for change, word in ((dict(fingerprint=8), 'fingerprint'), (dict(ae_name='cvpr/hi'), 'config'), (dict(C=16), 'C = 16'),
                         (dict(L=12), 'L = 12'), (dict(H=0), 'image size'), (dict(resolution=2e9), 'resolution')):
        with pytest.raises(ValueError, match=word):
            shell.check_container(codec.parse_container(codec.build_checked_container(**dict(good, **change))))
        with pytest.raises(ValueError, match=word):
            shell._salvage_head(codec.build_checked_container(**dict(good, **change)))
    # 61 x 93 pads to 64 x 96: 1 row above, 1 column left.  Tile 0 = latent (0, 0, 3, 5) = padded pixels 0..24 x 0..40
    r = shell._report(c, {0: 'crc', 8: 'truncated'}, [(0, 'missing'), (4, 'decoder'), (8, 'missing')], False)
    assert r.ntiles == 9 and r.file_crc_ok is False
    assert r.damaged == [codec.DamagedTile(0, 'crc', (0, 0, 3, 5), (0, 0, 23, 39)),
                         codec.DamagedTile(4, 'decoder', (3, 5, 3, 5), (23, 39, 24, 40)),
                         codec.DamagedTile(8, 'truncated', (6, 10, 2, 2), (47, 79, 14, 14))]
    with pytest.raises(ValueError, match='checked=True needs a tile extent'):
        codec.Codec(None, None, None, checked=True)


# ---- verify -------------------------------------------------------------------------------------------------------------------

def _verify_dir(tmp_path):
    from imgcomp_cvpr_amd import codec
    f = _fields()
    d = tmp_path / 'archive'
    d.mkdir()
    v4 = codec.build_checked_container(**f)
    bad = bytearray(v4)
    payload = _offsets(f)[5]
    bad[payload] ^= 0x01                                   # tile 0
    bad[payload + 2] ^= 0x01                               # tile 2 (tile 1 is empty)
    files = {'a_v1.icf': codec.build_container('cvpr/low', 'cvpr/res_shallow', 61, 93, 32, 8, 12, 6, 3, 1e9, 1, b'\x12\x34'),
             'b_v2.icf': codec.build_tiled_container(**f), 'c_v4.icf': v4, 'd_bad.icf': bytes(bad)}
    for name, data in files.items():
        (d / name).write_bytes(data)
    (d / 'notes.txt').write_bytes(b'not a codec file')
    return d, files


def test_verify_lines_and_exit_status(tmp_path, capsys):
    from imgcomp_cvpr_amd import codec
    d, files = _verify_dir(tmp_path)
    assert codec.main(['verify', str(d)]) == 1
    lines = capsys.readouterr().out.strip().splitlines()
    assert [os.path.basename(l.split(':')[0]) for l in lines] == ['a_v1.icf', 'b_v2.icf', 'c_v4.icf', 'd_bad.icf']
    assert [l.split(': ', 1)[1][:13] for l in lines[:3]] == ['ok (format 1,', 'ok (format 2,', 'ok (format 4,']
    assert lines[3].endswith('2 of 9 tiles damaged: tile 0 (crc), tile 2 (crc)')
    good = [str(d / n) for n in ('a_v1.icf', 'b_v2.icf', 'c_v4.icf')]
    assert codec.main(['verify'] + good) == 0
    assert len(capsys.readouterr().out.strip().splitlines()) == 3
    # formats 1 and 2: the strict reader's refusal; a truncated format 4: its tiles; a damaged header: that
    (d / 'a_v1.icf').write_bytes(files['a_v1.icf'][:-1] + bytes([files['a_v1.icf'][-1] ^ 0x01]))
    (d / 'b_v2.icf').write_bytes(files['b_v2.icf'][:-9])
    (d / 'c_v4.icf').write_bytes(files['c_v4.icf'][:-4 - 3 - 2 - 1])          # tiles 6, 7, 8 have 1, 2, 3 bytes
    head = bytearray(files['c_v4.icf'])
    head[30] ^= 0x01
    (d / 'e_head.icf').write_bytes(bytes(head))
    assert codec.main(['verify', str(d / 'a_v1.icf'), str(d)]) == 1
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 6 and 'CRC mismatch' in lines[0] and 'CRC mismatch' in lines[1] and 'CRC mismatch' in lines[2]
    assert lines[3].endswith('3 of 9 tiles damaged: tile 6 (truncated), tile 7 (truncated), tile 8 (truncated)')
    assert 'header damaged: nothing can be recovered' in lines[5]
    assert codec.main(['verify', str(d / 'nowhere.icf')]) == 1 and 'cannot read' in capsys.readouterr().out
    with pytest.raises(SystemExit):
        codec.main(['verify'])
    # the four existing commands still take exactly input and output
    with pytest.raises(SystemExit):
        codec.main(['decompress', 'a'])


def test_verify_needs_neither_torch_nor_the_hip_library(tmp_path):
    d, _ = _verify_dir(tmp_path)
    script = ('import sys\n'
              'sys.modules["torch"] = None\n'
              'sys.path.insert(0, {!r})\n'
              'from imgcomp_cvpr_amd import codec\n'
              'rc = codec.main(["verify", {!r}])\n'
              'assert "imgcomp_cvpr_amd._lib" not in sys.modules and sys.modules["torch"] is None\n'
              'sys.exit(10 + rc)\n').format(ROOT, str(d))
    r = subprocess.run([sys.executable, '-c', script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert r.returncode == 11, r.stderr
    assert r.stdout.count('ok (format') == 3 and 'tile 0 (crc), tile 2 (crc)' in r.stdout


# ---- the command line ---------------------------------------------------------------------------------------------------------

def test_checked_without_tile_is_refused_before_any_device(tmp_path, capsys):
    import argparse
    from imgcomp_cvpr_amd import codec
    src, dst = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    (src / 'a.png').write_bytes(b'x')
    for args, msg in ((['compress', str(src / 'a.png'), str(dst), '--checked'], '--checked needs --tile'),
                      (['compress-dir', str(src), str(dst), '--checked'], '--checked needs --tile'),
                      (['decompress', str(src / 'a.png'), str(dst), '--checked', '--tile', '128'], '--checked belongs to compress'),
                      (['decompress-dir', str(src), str(dst), '--checked'], '--checked belongs to compress'),
                      (['compress', str(src / 'a.png'), str(dst), '--salvage'], '--salvage belongs to decompress'),
                      (['compress-dir', str(src), str(dst), '--salvage'], '--salvage belongs to decompress')):
        assert codec.main(args + ['--device', 'no-such-device']) == 2, args
        assert msg in capsys.readouterr().err, args
    assert not dst.exists()
    flags = argparse.Namespace(command='compress-dir', input=str(src), output=str(dst), tile=None, batch=3, checked=True, salvage=False)
    with pytest.raises(ValueError, match='--checked needs --tile'):
        codec.check_dir_args(flags, 8)
    flags.tile = 128
    assert codec.check_dir_args(flags, 8) == ([(str(src / 'a.png'), str(dst / 'a.icf'))], (16, 16))


# ---- the rule in NumPy, on cases small enough to do by hand -------------------------------------------------------------------

def test_numpy_rule_by_hand():
    from tests import conceal_rule as R
    # one channel, 4 x 6 plane, 2 x 3 tiles: a 2 x 2 grid
    s = np.array([[[1, 1, 1, 2, 2, 2],
                   [1, 1, 1, 2, 2, 3],
                   [4, 4, 0, 5, 5, 5],
                   [4, 4, 4, 5, 5, 5]]], dtype=np.int64)
    out = R.conceal(s, [0], 2, 3, 6, 3)
    # ring of tile 0: below (4, 4, 0), right (2, 2) -> 4 and 2 twice each: the tie goes to the smaller symbol
    assert (out[0, :2, :3] == 2).all() and np.array_equal(out[0, 2:], s[0, 2:]) and np.array_equal(out[0, :2, 3:], s[0, :2, 3:])
    out = R.conceal(s, [0, 1], 2, 3, 6, 3)                 # adjacent damaged tiles ignore each other
    assert (out[0, :2, :3] == 4).all() and (out[0, :2, 3:] == 5).all()
    out = R.conceal(s, [0, 1, 2, 3], 2, 3, 6, 3)           # nothing intact: the fallback everywhere
    assert (out == 3).all()
    assert (R.conceal(s, [0], 4, 6, 6, 1) == 1).all()      # a one-tile volume
    assert np.array_equal(R.conceal(s, [], 2, 3, 6, 3), s)
    assert R.fallback_symbol([-2.0, -0.5, 0.5, 2.0]) == 1 and R.fallback_symbol([3, -1, 0.25, 7]) == 2
    assert R.grid(8, 12, 3, 5)[8] == (6, 10, 2, 2) and len(R.grid(8, 12, 3, 5)) == 9


# ---- ic_pc_conceal_tiles: the argument checks run on the host, before any device call -----------------------------------------

IC_ERR_ARG, IC_ERR_UNSUPPORTED, IC_ERR_WORKSPACE = -1, -2, -3
VOLS = [(8, 12, 0, 0), (16, 6, 4 * 8 * 12, 4 * 8 * 12)]            # h, w, symbols_off, q_off: two volumes of C = 4; 3 x 5 tiles: 9 + 12 cells


def _conceal_call(tiles, volumes=VOLS, marks=None, C=4, L=6, fallback=2, th=3, tw=5, workspace_bytes=None, ntiles=None, nvolumes=None,
                  null=()):
    """the ABI with pointers that are never followed on a refused call: distinct non-null host addresses"""
    from imgcomp_cvpr_amd import _lib
    keep = ctypes.create_string_buffer(64)
    p = ctypes.addressof(keep)
    n = len(tiles) if ntiles is None else ntiles
    nv = len(volumes) if nvolumes is None else nvolumes
    marks = bytes([1] * 21) if marks is None else bytes(marks)
    need = _lib.lib.ic_pc_conceal_tiles_workspace_bytes(max(n, 1), max(nv, 1), 21)
    args = dict(symbols=p, q=p + 8, tiles=_lib.tile_table(tiles), volumes=_lib.volume_table(volumes),
                marks=ctypes.create_string_buffer(marks, len(marks)), centers=p + 16, ws=p + 32)
    for name in ([null] if isinstance(null, str) else null):
        args[name] = None
    return _lib.lib.ic_pc_conceal_tiles(args['symbols'], args['q'], args['tiles'], n, args['volumes'], nv, args['marks'], args['centers'],
                                        L, fallback, C, th, tw, args['ws'], need if workspace_bytes is None else workspace_bytes, None)


def test_conceal_refuses_bad_descriptors_on_the_host():
    from imgcomp_cvpr_amd import _lib
    good0, good1 = (3, 5, 3, 5, 0, 0, 0, 0), (15, 5, 1, 1, 0, 0, 0, 1)       # y0, x0, th, tw, -, -, -, volume: cell 4 of volume 0, the last of volume 1
    for what, tile in (('volume = nvolumes', (3, 5, 3, 5, 0, 0, 0, 2)), ('volume < 0', (3, 5, 3, 5, 0, 0, 0, -1)),
                       ('outside its volume', (9, 5, 3, 5, 0, 0, 0, 0)), ('inside volume 0, outside its own volume 1', (3, 10, 3, 2, 0, 0, 0, 1)),
                       ('th = 0', (3, 5, 0, 5, 0, 0, 0, 0)), ('tw < 0', (3, 5, 3, -5, 0, 0, 0, 0)),
                       ('y0 < 0', (-3, 5, 3, 5, 0, 0, 0, 0)), ('x0 < 0', (3, -5, 3, 5, 0, 0, 0, 0)),
                       ('y0 + th overflows int', (2 ** 31 - 1, 5, 3, 5, 0, 0, 0, 0)),
                       ('not on the grid', (2, 5, 3, 5, 0, 0, 0, 0)), ('not on the grid in x', (3, 4, 3, 5, 0, 0, 0, 0)),
                       ('smaller than its cell', (3, 5, 2, 5, 0, 0, 0, 0)), ('two cells', (3, 0, 3, 10, 0, 0, 0, 0)),
                       ('the edge cell at the nominal extent', (6, 10, 3, 5, 0, 0, 0, 0))):
        assert _conceal_call([good0, good1, tile]) == IC_ERR_ARG, what
        assert _conceal_call([tile]) == IC_ERR_ARG, what
    # a listed tile that the map calls intact could be read while it is written
    marks = [1] * 21
    marks[4] = 0
    assert _conceal_call([good0, good1], marks=marks) == IC_ERR_ARG
    marks = [0] * 21
    marks[4] = marks[20] = 1
    assert _conceal_call([good0, good1], marks=marks, workspace_bytes=0) == IC_ERR_WORKSPACE
    for what, vols in (('h = 0', [(0, 12, 0, 0), VOLS[1]]), ('w < 0', [VOLS[0], (16, -6, 0, 0)]),
                       ('symbols_off < 0', [(8, 12, -1, 0), VOLS[1]]), ('q_off < 0', [VOLS[0], (16, 6, 0, -1)])):
        assert _conceal_call([good0], volumes=vols) == IC_ERR_ARG, what
    for kw in (dict(ntiles=0), dict(nvolumes=0), dict(C=0), dict(C=65536), dict(L=0), dict(th=0), dict(tw=-1), dict(fallback=6),
               dict(fallback=-1), dict(L=17, fallback=17)):
        assert _conceal_call([good0], **kw) == IC_ERR_ARG, kw
    assert _conceal_call([good0, good1], nvolumes=1) == IC_ERR_ARG
    for null in ('symbols', 'tiles', 'volumes', 'marks', 'centers', 'ws'):
        assert _conceal_call([good0, good1], null=null) == IC_ERR_ARG, null
    assert _conceal_call([good0], L=17, fallback=16) == IC_ERR_UNSUPPORTED
    # legal tables get as far as the workspace check, with and without q
    need = _lib.lib.ic_pc_conceal_tiles_workspace_bytes(2, 2, 21)
    assert need >= 2 * 40 + 2 * 24 + 21
    for null in ((), 'q'):
        for short in (0, 1, need // 2, need - 1):
            assert _conceal_call([good0, good1], workspace_bytes=short, null=null) == IC_ERR_WORKSPACE, (null, short)
    ws = _lib.lib.ic_pc_conceal_tiles_workspace_bytes
    assert ws(0, 2, 21) == ws(2, 0, 21) == ws(2, 2, 0) == 0 and ws(48, 2, 21) >= ws(2, 2, 21) and ws(2, 2, 1 << 20) >= (1 << 20)
