"""-m gpu: checked tiles (container format 4) on the device.  ic_pc_conceal_tiles against the NumPy statement of its rule
(tests/conceal_rule.py), exactly; format 4 against format 2 (the same streams, the same pixels); salvage of intact and of damaged
files against the symbols the rule gives and the decoder's own pixels for them.  No damaged stream is ever handed to the range
decoder: a tile that the reader calls damaged is skipped, which is the point of the format."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import conceal_rule as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5
SENTINEL_Q = -12345.625


def _image(H, W_, seed=9):
    from imgcomp_cvpr_amd import weights as W
    return np.ascontiguousarray(W.synthetic_image((1, 3, H, W_), 'natural', seed=seed)[0].transpose(1, 2, 0))


# ---- 1: the kernel against the rule, through the C ABI ------------------------------------------------------------------------

def _raw_conceal(cuda, vols, th, tw, L, centers, fallback, with_q=True, gap=384):
    """ic_pc_conceal_tiles through the ABI.  vols: [((C,h,w) int64 numpy, [damaged tile indices])].  The volumes lie `gap` elements
    apart in `symbols` and `q`; symbols outside the volumes hold -7, q holds a sentinel EVERYWHERE (the kernel is the only writer of
    q here), the workspace has a guarded tail.  -> ([symbols per volume], [q per volume] or None)"""
    from imgcomp_cvpr_amd import _lib
    shapes, offs, total, tiles, marks = [], [], gap, [], []
    for n, (sym, damaged) in enumerate(vols):
        C, h, w = sym.shape
        grid = R.grid(h, w, th, tw)
        m = bytearray(len(grid))
        for t in damaged:
            m[t] = 1
            tiles.append(grid[t] + (0, 0, 0, n))
        marks.append(bytes(m))
        shapes.append((C, h, w))
        offs.append(total)
        total += C * h * w + gap
    marks = b''.join(marks)
    host = np.full(total, -7, np.int64)
    for (sym, _), o in zip(vols, offs):
        host[o:o + sym.size] = sym.reshape(-1)
    sym_dev = torch.as_tensor(host).to(cuda)
    q_dev = torch.full((total,), SENTINEL_Q, dtype=torch.float32, device=cuda) if with_q else None
    table = _lib.tile_table(tiles)
    vtable = _lib.volume_table([(h, w, o, o) for (_, h, w), o in zip(shapes, offs)])
    need = int(_lib.lib.ic_pc_conceal_tiles_workspace_bytes(len(tiles), len(shapes), len(marks)))
    ws = torch.full((need + 4096,), GUARD, dtype=torch.uint8, device=cuda)
    cen = torch.as_tensor(np.asarray(centers, np.float32)).to(cuda)
    host_marks = ctypes.create_string_buffer(marks, len(marks))
    _lib.check(_lib.lib.ic_pc_conceal_tiles(_lib.ptr(sym_dev), _lib.ptr(q_dev), table, len(tiles), vtable, len(shapes), host_marks,
                                            _lib.ptr(cen), L, fallback, shapes[0][0], th, tw, _lib.ptr(ws), need,
                                            _lib.current_stream(cuda)), 'ic_pc_conceal_tiles')
    torch.cuda.synchronize()
    assert bool((ws[need:] == GUARD).all()), 'workspace: written behind its stated size'
    got = sym_dev.cpu().numpy()
    keep = np.ones(total, bool)
    for (c, h, w), o in zip(shapes, offs):
        keep[o:o + c * h * w] = False
    assert (got[keep] == -7).all(), 'symbols: written outside the volumes'
    syms = [got[o:o + c * h * w].reshape(c, h, w) for (c, h, w), o in zip(shapes, offs)]
    if not with_q:
        return syms, None
    qall = q_dev.cpu().numpy()
    assert (qall[keep] == np.float32(SENTINEL_Q)).all(), 'q: written outside the volumes'
    return syms, [qall[o:o + c * h * w].reshape(c, h, w) for (c, h, w), o in zip(shapes, offs)]


def _check_against_rule(cuda, vols, th, tw, L, centers, fallback, with_q=True):
    syms, qs = _raw_conceal(cuda, vols, th, tw, L, centers, fallback, with_q)
    cen = np.asarray(centers, np.float32)
    for n, (sym, damaged) in enumerate(vols):
        want = R.conceal(sym, damaged, th, tw, L, fallback)
        assert np.array_equal(syms[n], want), 'volume {}: symbols differ from the rule'.format(n)
        inside = np.zeros(sym.shape[1:], bool)
        grid = R.grid(sym.shape[1], sym.shape[2], th, tw)
        for t in damaged:
            y0, x0, a, b = grid[t]
            inside[y0:y0 + a, x0:x0 + b] = True
        assert np.array_equal(syms[n][:, ~inside], sym[:, ~inside]), 'volume {}: a cell outside the damaged tiles changed'.format(n)
        if with_q:
            assert np.array_equal(qs[n][:, inside].view(np.uint32), cen[want][:, inside].view(np.uint32)), 'q is not centers[symbols] bit for bit'
            assert (qs[n][:, ~inside] == np.float32(SENTINEL_Q)).all(), 'volume {}: q outside the damaged tiles was written'.format(n)
    return syms


def _centers(L, seed=0):
    c = np.sort(np.random.RandomState(seed).uniform(-2, 2, L).astype(np.float32))
    return c


# (h, w, th, tw): 4 x 6 tiles that divide, 3 x 3 tiles that do not (last row 2 high, last column 2 wide)
GRIDS = [(16, 24, 4, 4), (8, 12, 3, 5)]


def _damage_sets(h, w, th, tw):
    gh, gw = -(-h // th), -(-w // tw)
    n = gh * gw
    centre = (gh // 2) * gw + gw // 2
    sets = {'corner': [0], 'last corner': [n - 1], 'edge': [1], 'interior': [centre], 'adjacent': [centre, centre + 1],
            'below each other': [centre - gw, centre], 'every tile': list(range(n)),
            # the centre tile and its four neighbours: the centre has no intact neighbour -> fallback
            'all neighbours damaged': sorted({centre, centre - 1, centre + 1, centre - gw, centre + gw} & set(range(n)))}
    return sets


@pytest.mark.parametrize('L', [6, 16])
@pytest.mark.parametrize('h,w,th,tw', GRIDS)
def test_kernel_equals_the_numpy_rule(cuda, L, h, w, th, tw):
    rng = np.random.RandomState(L * 100 + h)
    centers = _centers(L)
    fallback = R.fallback_symbol(centers)
    for name, damaged in _damage_sets(h, w, th, tw).items():
        # few distinct symbols per ring, so that the most frequent one is a real decision and ties happen
        sym = rng.randint(0, L, size=(5, h, w)).astype(np.int64)
        sym[1] = rng.randint(0, 2, size=(h, w)) * (L - 1)
        sym[2] = 3
        got = _check_against_rule(cuda, [(sym, damaged)], th, tw, L, centers, fallback)[0]
        if name == 'every tile':
            assert (got == fallback).all()
        if name == 'all neighbours damaged' and len(damaged) == 5:
            y0, x0, a, b = R.grid(h, w, th, tw)[damaged[2]]
            assert (got[:, y0:y0 + a, x0:x0 + b] == fallback).all()
        # damaged tiles never read each other, nor themselves: other contents inside them change nothing
        other = sym.copy()
        for t in damaged:
            y0, x0, a, b = R.grid(h, w, th, tw)[t]
            other[:, y0:y0 + a, x0:x0 + b] = rng.randint(0, L, size=(5, a, b))
        assert np.array_equal(_check_against_rule(cuda, [(other, damaged)], th, tw, L, centers, fallback)[0], got), name


def test_kernel_one_tile_volume_two_volumes_tie_and_no_q(cuda):
    L = 6
    centers = np.array([-2.0, -1.0, -0.25, 0.5, 1.0, 2.0], np.float32)
    fallback = R.fallback_symbol(centers)
    assert fallback == 2
    rng = np.random.RandomState(5)
    one = rng.randint(0, L, size=(3, 5, 7)).astype(np.int64)
    got = _check_against_rule(cuda, [(one, [0])], 16, 16, L, centers, fallback)[0]            # a one-tile volume: the fallback
    assert (got == fallback).all()
    # two volumes of different (h, w) in one call, with and without q
    a = rng.randint(0, L, size=(3, 8, 12)).astype(np.int64)
    b = rng.randint(0, L, size=(3, 7, 4)).astype(np.int64)
    for with_q in (True, False):
        _check_against_rule(cuda, [(a, [0, 4, 5, 8]), (b, [1, 2])], 3, 5, L, centers, fallback, with_q)
        _check_against_rule(cuda, [(b, [0]), (one[:, :, :4], []), (a, list(range(9)))], 3, 5, L, centers, fallback, with_q)
    # a constructed tie: tile 4 of the 3 x 5 grid of an 8 x 12 plane is rows 3..5, columns 5..9; its ring has 5 + 5 + 3 + 3 cells
    tie = np.zeros((2, 8, 12), np.int64)
    tie[:, 2, 5:10] = 5                                    # above: five 5s
    tie[:, 6, 5:10] = 1                                    # below: five 1s
    tie[:, 3:6, 4] = 4                                     # left and right: three 4s each -> six 4s in channel 0
    tie[:, 3:6, 10] = 4
    tie[1, 3, 4] = 0                                       # channel 1: 5, 1 and 4 five times each, one 0
    got = _check_against_rule(cuda, [(tie, [4])], 3, 5, L, centers, fallback)[0]
    assert (got[0, 3:6, 5:10] == 4).all() and (got[1, 3:6, 5:10] == 1).all()


# ---- 2, 3: format 4 against format 2; salvage of an intact file ---------------------------------------------------------------

@pytest.fixture(scope='module')
def codecs(cuda, configs, syn_weights):
    from imgcomp_cvpr_amd import codec
    return {'v2': codec.Codec(configs[0], configs[1], syn_weights, cuda, tile=(8, 8)),
            'v4': codec.Codec(configs[0], configs[1], syn_weights, cuda, tile=(8, 8), checked=True)}


@pytest.fixture(scope='module')
def images():
    return [_image(256, 384, seed=31), _image(61, 93, seed=32), _image(128, 72, seed=33)]


@pytest.fixture(scope='module')
def files(codecs, images):
    return {k: [c.compress(img) for img in images] for k, c in codecs.items()}


def test_format_4_holds_the_streams_and_pixels_of_format_2(codecs, images, files):
    from imgcomp_cvpr_amd import codec
    for i, (a, b) in enumerate(zip(files['v4'], files['v2'])):
        c4, c2 = codec.parse_container(a), codec.parse_container(b)
        assert isinstance(c4, codec.CheckedContainer) and c4.version == 4 and c2.version == 2
        assert c4.streams == c2.streams and c4.first_syms == c2.first_syms and len(a) == len(b) + 4 * len(c2.streams) + 4
        assert c4[1:-1] == c2[1:]
        for reader in codecs.values():                     # the file says what it is, not the object
            assert np.array_equal(reader.decompress(a), reader.decompress(b)), i
    assert codecs['v4'].compress_many(images) == files['v4']
    got = codecs['v2'].decompress_many(files['v4'] + files['v2'])
    for i, img in enumerate(got):
        assert np.array_equal(img, codecs['v2'].decompress(files['v2'][i % 3])), i


def test_salvage_of_an_intact_file_is_decompress(codecs, files):
    c = codecs['v2']
    for data in files['v4']:
        img, report = c.salvage(data)
        assert np.array_equal(img, c.decompress(data))
        assert report.damaged == [] and report.file_crc_ok is True and report.ntiles == len(c.decode_symbols(data)[1].streams)
    for data in (files['v2'][0], ):
        with pytest.raises(ValueError, match='format version 2 has nothing to salvage with'):
            c.salvage(data)


# ---- 4: damaged files ---------------------------------------------------------------------------------------------------------

def _payload_start(data):
    from imgcomp_cvpr_amd import codec
    c = codec.parse_container(data)
    return len(data) - 4 - len(c.payload), np.concatenate([[0], np.cumsum([len(b) for b in c.streams])]).astype(np.int64), c


def _flipped(data, tiles):
    start, offs, c = _payload_start(data)
    bad = bytearray(data)
    for t in tiles:
        assert len(c.streams[t]) >= 2
        bad[start + int(offs[t]) + len(c.streams[t]) // 2] ^= 0x20
    return bytes(bad)


def _truncated(data, tile):
    start, offs, c = _payload_start(data)
    assert len(c.streams[tile]) >= 2
    return data[:start + int(offs[tile]) + len(c.streams[tile]) // 2]


def _check_salvage(c, good, bad, want_damage):
    """want_damage: [(tile, reason)].  Symbols through decode_tiles_batch(conceal=True), pixels through salvage."""
    from imgcomp_cvpr_amd import codec
    with pytest.raises(ValueError, match='CRC|truncated'):
        c.decompress(bad)
    orig, head = c.decode_symbols(good)
    sal, damage, ok = codec.parse_salvage(bad)
    assert damage == want_damage and ok is False
    tiles = [t for t, _ in want_damage]
    assert [b is None for b in sal.streams] == [t in tiles for t in range(len(sal.streams))]
    res, dmg = c.pred.decode_tiles_batch([(sal.streams, sal.first_syms, (sal.C, sal.h, sal.w))], sal.th, sal.tw, want='both',
                                         conceal=True)
    q, s = res[0]
    assert dmg == [[(t, 'missing') for t in tiles]]
    centers = c.ae.get_centers_variable().detach().float()
    fallback = R.fallback_symbol(centers.cpu().numpy())
    assert c.pred.conceal_fallback() == fallback
    want = R.conceal(orig, tiles, sal.th, sal.tw, c.L, fallback)
    assert np.array_equal(s.cpu().numpy(), want), 'symbols: not the original outside the damaged tiles and the rule inside'
    assert torch.equal(q, centers[s]), 'q is not centers[symbols] bit for bit'
    img, report = c.salvage(bad)
    x_out = c.ae.decode(centers[torch.as_tensor(want).to(s.device)][None].contiguous(), is_training=False).to(torch.uint8)
    assert np.array_equal(img, c._crop(x_out[0], head)), 'pixels: not the decoder\'s output for the concealed symbols'
    assert report.ntiles == len(sal.streams) and report.file_crc_ok is False
    assert [(d.index, d.reason) for d in report.damaged] == want_damage
    return img, report


def test_salvage_of_flipped_and_truncated_files(codecs, images, files):
    c, good = codecs['v2'], files['v4'][0]                 # 256 x 384 at 64-pixel tiles: a 4 x 6 grid
    assert len(_payload_start(good)[2].streams) == 24
    img, report = _check_salvage(c, good, _flipped(good, [0, 9, 10, 23]), [(t, 'crc') for t in (0, 9, 10, 23)])
    for d in report.damaged:
        ty, tx = divmod(d.index, 6)
        assert d.latent == (8 * ty, 8 * tx, 8, 8) and d.pixels == (64 * ty, 64 * tx, 64, 64)
    whole = c.decompress(good)
    assert img.shape == whole.shape and not np.array_equal(img, whole)
    img, report = _check_salvage(c, good, _truncated(good, 17), [(t, 'truncated') for t in range(17, 24)])
    assert [d.pixels for d in report.damaged] == [(64 * (t // 6), 64 * (t % 6), 64, 64) for t in range(17, 24)]
    # 61 x 93 pads to 64 x 96 (one row above, one column left): two tiles, 8 and 4 latent columns; clipped rectangles
    small = files['v4'][1]
    img, report = _check_salvage(c, small, _flipped(small, [0]), [(0, 'crc')])
    assert report.damaged[0].latent == (0, 0, 8, 8) and report.damaged[0].pixels == (0, 0, 61, 63)


def test_salvage_many_equals_the_loop(codecs, files):
    c = codecs['v2']
    datas = [files['v4'][0], _flipped(files['v4'][0], [3, 14]), _truncated(files['v4'][2], 1), files['v4'][1], _flipped(files['v4'][2], [0, 1])]
    got = c.salvage_many(datas)
    assert len(got) == len(datas)
    for i, (data, (img, report)) in enumerate(zip(datas, got)):
        one_img, one_report = c.salvage(data)
        assert np.array_equal(img, one_img), i
        assert report == one_report, i
    assert [len(r.damaged) for _, r in got] == [0, 2, 3, 0, 2]        # 128 x 72: 2 x 2 tiles, cut inside tile 1
    assert c.salvage_many([]) == []
    with pytest.raises(ValueError, match='file 1: format version 2 has nothing to salvage with'):
        c.salvage_many([files['v4'][0], files['v2'][0]])
    head = bytearray(files['v4'][1])
    head[20] ^= 1
    with pytest.raises(ValueError, match='file 2: header damaged: nothing can be recovered'):
        c.salvage_many([files['v4'][0], datas[1], bytes(head)])


def test_a_skipped_tile_without_concealment_is_zero(codecs, files):
    """decode_tiles_batch with a None stream and conceal off: the other tiles as before, the skipped one symbol 0 / q 0.0"""
    from imgcomp_cvpr_amd import codec
    c = codecs['v2']
    h = codec.parse_container(files['v4'][2])
    ref = c.pred.decode_tiles_batch([(h.streams, h.first_syms, (h.C, h.h, h.w))], h.th, h.tw, want='both')
    streams = list(h.streams)
    streams[1] = None
    got = c.pred.decode_tiles_batch([(streams, h.first_syms, (h.C, h.h, h.w))], h.th, h.tw, want='both')
    y0, x0, a, b = codec.tile_grid(h.h, h.w, h.th, h.tw)[1]
    for r, g in zip(ref[0], got[0]):
        assert bool((g[:, y0:y0 + a, x0:x0 + b] == 0).all())
        g = g.clone()
        g[:, y0:y0 + a, x0:x0 + b] = r[:, y0:y0 + a, x0:x0 + b]
        assert torch.equal(g, r)


# ---- 5: the command line ------------------------------------------------------------------------------------------------------

def _cli(args, timeout):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    return subprocess.run([sys.executable, '-m', 'imgcomp_cvpr_amd.codec'] + args, cwd=ROOT, env=env, timeout=timeout,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


def test_cli_checked_and_salvage_in_fresh_processes(codecs, tmp_path):
    from PIL import Image
    src, mid, dst = tmp_path / 'in', tmp_path / 'icf', tmp_path / 'out'
    src.mkdir()
    imgs = {'a': _image(128, 192, seed=41), 'b': _image(61, 93, seed=42)}
    for stem, img in imgs.items():
        Image.fromarray(img).save(str(src / (stem + '.png')))
    r = _cli(['compress-dir', str(src), str(mid), '--tile', '64', '--checked'], 600)
    assert r.returncode == 0, r.stderr
    for stem, img in imgs.items():
        assert (mid / (stem + '.icf')).read_bytes() == codecs['v4'].compress(img), stem
    good = (mid / 'a.icf').read_bytes()
    bad = _flipped(good, [1, 4])
    (mid / 'a.icf').write_bytes(bad)
    r = _cli(['verify', str(mid)], 120)
    assert r.returncode == 1 and 'a.icf: 2 of 6 tiles damaged: tile 1 (crc), tile 4 (crc)' in r.stdout and 'b.icf: ok' in r.stdout
    r = _cli(['decompress-dir', str(mid), str(dst)], 600)
    assert r.returncode == 2 and 'a.icf' in r.stderr and 'CRC mismatch' in r.stderr
    r = _cli(['decompress-dir', str(mid), str(dst), '--salvage'], 600)
    assert r.returncode == 0, r.stderr
    print(r.stdout.strip())
    assert 'a.icf: salvaged, 2 of 6 tiles damaged: tile 1 (crc) pixels y 0..64 x 64..128, tile 4 (crc) pixels y 64..128 x 64..128' in r.stdout
    assert sorted(os.listdir(str(dst))) == ['a.png', 'b.png']
    assert np.array_equal(np.asarray(Image.open(str(dst / 'a.png'))), codecs['v2'].salvage(bad)[0])
    assert np.array_equal(np.asarray(Image.open(str(dst / 'b.png'))), codecs['v2'].decompress((mid / 'b.icf').read_bytes()))
    r = _cli(['decompress', str(mid / 'a.icf'), str(tmp_path / 'one.png'), '--salvage'], 600)
    assert r.returncode == 0 and 'salvaged, 2 of 6 tiles damaged' in r.stdout, r.stderr
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / 'one.png'))), codecs['v2'].salvage(bad)[0])
    head = bytearray(good)
    head[20] ^= 1
    (mid / 'a.icf').write_bytes(bytes(head))
    r = _cli(['decompress', str(mid / 'a.icf'), str(tmp_path / 'none.png'), '--salvage'], 600)
    assert r.returncode == 2 and 'header damaged: nothing can be recovered' in r.stderr and not (tmp_path / 'none.png').exists()
