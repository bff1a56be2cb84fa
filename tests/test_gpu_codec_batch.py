"""-m gpu: the batch codec.  compress_many / decompress_many, encode_tiles_batch / decode_tiles_batch and ic_pc_decode_tiles_batch_f32
run the kernels of the single-image calls on the same inputs, so every comparison is an equality: the same bytes, the same pixels,
the same symbols, q = centers[symbols] bit for bit."""
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5
SHAPES = [(61, 93), (64, 96), (64, 96), (128, 72), (512, 768)]
TILES = [(3, 5), (16, 16), None]


def _image(H, W_, seed=9):
    from imgcomp_cvpr_amd import weights as W
    return np.ascontiguousarray(W.synthetic_image((1, 3, H, W_), 'natural', seed=seed)[0].transpose(1, 2, 0))


@pytest.fixture(scope='module')
def images():
    return [_image(H, W_, seed=20 + i) for i, (H, W_) in enumerate(SHAPES)]


@pytest.fixture(scope='module')
def codecs(cuda, configs, syn_weights):
    from imgcomp_cvpr_amd import codec
    return {tile: codec.Codec(configs[0], configs[1], syn_weights, cuda, tile=tile) for tile in TILES}


@pytest.fixture(scope='module')
def files(codecs, images):
    """the single-image path, file by file: what the batch calls are compared with"""
    return {tile: [codecs[tile].compress(img) for img in images] for tile in TILES}


@pytest.fixture(scope='module')
def pixels(codecs, files):
    return {tile: [codecs[None].decompress(f) for f in files[tile]] for tile in TILES}


# ---- 1, 2: the same bytes, the same pixels ------------------------------------------------------------------------------------

@pytest.mark.parametrize('tile', TILES)
def test_compress_many_writes_the_bytes_of_compress(codecs, images, files, tile):
    from imgcomp_cvpr_amd import codec
    got = codecs[tile].compress_many(images)
    assert len(got) == len(images)
    for i, (a, b) in enumerate(zip(got, files[tile])):
        assert codec.parse_container(a).version == (1 if tile is None else 2)
        assert a == b, 'image {} {}: compress_many wrote other bytes than compress'.format(i, SHAPES[i])
    assert codecs[tile].compress_many([]) == []
    assert codecs[tile].compress_many(images[:1]) == files[tile][:1]
    with pytest.raises(ValueError, match='image 1: expected an HWC uint8 image'):
        codecs[tile].compress_many([images[0], images[1].astype(np.float32)])


@pytest.mark.parametrize('tile', TILES)
def test_decompress_many_gives_the_pixels_of_decompress(codecs, files, pixels, tile):
    for c in (codecs[tile], codecs[None]):                # the file says how it is tiled, not the object
        got = c.decompress_many(files[tile])
        assert len(got) == len(SHAPES)
        for i, (a, b) in enumerate(zip(got, pixels[tile])):
            assert a.dtype == np.uint8 and a.shape == SHAPES[i] + (3,)
            assert np.array_equal(a, b), 'file {} {}: decompress_many gave other pixels than decompress'.format(i, SHAPES[i])
    assert codecs[tile].decompress_many([]) == []


def test_decompress_many_of_mixed_formats_and_tile_extents(codecs, files, pixels):
    """format 1 and format 2, two tile extents (16 x 16 the majority), in one call, results in input order"""
    order = [((16, 16), 4), (None, 0), ((3, 5), 3), ((16, 16), 1), (None, 4), ((16, 16), 3), ((3, 5), 0)]
    got = codecs[None].decompress_many([files[t][i] for t, i in order])
    for n, (t, i) in enumerate(order):
        assert np.array_equal(got[n], pixels[t][i]), (n, t, i)
    # the tiled and the untiled file of an image decode to the same pixels (test_gpu_codec_tiled.py): so do their batch results
    assert np.array_equal(got[0], got[4])


# ---- 3: the ABI ---------------------------------------------------------------------------------------------------------------

def _guarded(nbytes, cuda):
    return torch.full((nbytes,), GUARD, dtype=torch.uint8, device=cuda)


def _raw_batch(cuda, pred, vols, tile, outputs='both', flags=0, gap=512):
    """ic_pc_decode_tiles_batch_f32 through the ABI.  vols: [(streams, first_syms, (C,h,w))].  The volumes lie `gap` elements apart
    in `symbols` and `q`, with `gap` elements before the first and behind the last; every byte outside the volumes, behind status
    and behind the workspace's stated size must keep its guard value.  -> ([symbols per volume], [q per volume], status)"""
    from imgcomp_cvpr_amd import _lib, codec
    tiles, blobs, pos, shapes, offs, total = [], [], 0, [], [], gap
    for n, (streams, firsts, (C, h, w)) in enumerate(vols):
        for t, (y0, x0, a, b) in enumerate(codec.tile_grid(h, w, *tile)):
            tiles.append((y0, x0, a, b, pos, len(streams[t]), firsts[t], n))
            blobs.append(streams[t])
            pos += len(streams[t])
        shapes.append((C, h, w))
        offs.append(total)
        total += C * h * w + gap
    C = shapes[0][0]
    table = _lib.tile_table(tiles)
    vtable = _lib.volume_table([(h, w, o, o) for (_, h, w), o in zip(shapes, offs)])
    data = torch.frombuffer(bytearray(b''.join(blobs)), dtype=torch.uint8).to(cuda)
    sym_raw, q_raw = _guarded(8 * total, cuda), _guarded(4 * total, cuda)
    status = torch.full((len(tiles) + 64,), -7, dtype=torch.int32, device=cuda)
    need = _lib.lib.ic_pc_decode_tiles_batch_workspace_bytes(C, max(t[2] for t in tiles), max(t[3] for t in tiles), len(tiles),
                                                             len(shapes), pred.pc._k)
    ws = _guarded(need + 4096, cuda)
    centers = pred.centers.contiguous().float()
    _lib.check(_lib.lib.ic_pc_decode_tiles_batch_f32(
        _lib.ptr(data), pos, table, len(tiles), vtable, len(shapes), pred.pc._tab, _lib.ptr(centers), pred.pc._k, pred.pc.L,
        pred.freqs_resolution, _lib.ptr(sym_raw) if outputs in ('both', 'symbols') else None,
        _lib.ptr(q_raw) if outputs in ('both', 'q') else None, _lib.ptr(status), C, _lib.ptr(ws), need, flags,
        _lib.current_stream(cuda)), 'ic_pc_decode_tiles_batch_f32')
    torch.cuda.synchronize()
    assert bool((status[len(tiles):] == -7).all()), 'status: written behind the table'
    assert bool((ws[need:] == GUARD).all()), 'workspace: written behind its stated size'
    syms, qs = [], []
    for raw, size, dtype, used, outs in ((sym_raw, 8, torch.int64, outputs in ('both', 'symbols'), syms),
                                         (q_raw, 4, torch.float32, outputs in ('both', 'q'), qs)):
        keep = torch.ones(total, dtype=torch.bool, device=cuda)
        for (c, h, w), o in zip(shapes, offs):
            if used:
                keep[o:o + c * h * w] = False
                outs.append(raw.view(dtype)[o:o + c * h * w].reshape(c, h, w).clone())
        assert bool((raw.view(total, size)[keep] == GUARD).all()), 'written outside the volumes ({})'.format(dtype)
    return syms, qs, status[:len(tiles)].tolist()


def _coded_volumes(c, imgs, tile):
    vols, want = [], []
    for img in imgs:
        sym = c.encode_symbols(img)[0].symbols[0]
        coded = c.pred.encode_tiles(sym, *tile)
        vols.append(([b for b, _ in coded], [f for _, f in coded], tuple(int(v) for v in sym.shape)))
        want.append(sym)
    return vols, want


@pytest.mark.parametrize('flag', [None, 'PC_DECODE_PER_LAYER', 'PC_DECODE_RECOMPUTE'])
def test_abi_two_volumes_of_different_extent(cuda, codecs, images, flag):
    from imgcomp_cvpr_amd import _lib
    c, tile = codecs[None], (3, 5)
    pred = c.pred
    vols, want = _coded_volumes(c, [images[0], images[3]], tile)           # latent planes 8 x 12 and 16 x 9
    assert [v[2] for v in vols] == [(32, 8, 12), (32, 16, 9)]
    flags = 0 if flag is None else getattr(_lib, flag)
    centers = pred.centers.contiguous().float()
    # the existing call, volume by volume
    single = [pred.decode_tiles(s, f, shape, *tile) for s, f, shape in vols]
    for n in range(2):
        assert np.array_equal(single[n], want[n].cpu().numpy())
    syms, qs, status = _raw_batch(cuda, pred, vols, tile, 'both', flags)
    assert status == [0] * (9 + 12)
    for n in range(2):
        assert np.array_equal(syms[n].cpu().numpy(), single[n]), n
        assert torch.equal(qs[n], centers[syms[n]]), 'volume {}: q is not centers[symbols] bit for bit'.format(n)
    s_only, none, status = _raw_batch(cuda, pred, vols, tile, 'symbols', flags)
    assert none == [] and status == [0] * 21 and all(torch.equal(a, b) for a, b in zip(s_only, syms))
    none, q_only, status = _raw_batch(cuda, pred, vols, tile, 'q', flags)
    assert none == [] and status == [0] * 21 and all(torch.equal(a, b) for a, b in zip(q_only, qs))
    # one volume, every descriptor's volume field 0: the existing call
    for n in range(2):
        s1, q1, status = _raw_batch(cuda, pred, vols[n:n + 1], tile, 'both', flags)
        assert status == [0] * len(vols[n][0]) and np.array_equal(s1[0].cpu().numpy(), single[n]) and torch.equal(q1[0], qs[n])


# ---- 4: refused calls launch nothing ------------------------------------------------------------------------------------------

def test_refused_calls_write_nothing(cuda, codecs, images):
    """the host checks on real device buffers: the return code, and every output byte keeps its guard value"""
    from imgcomp_cvpr_amd import _lib
    c, tile = codecs[None], (3, 5)
    pred = c.pred
    vols, _ = _coded_volumes(c, [images[0], images[3]], tile)
    blob = b''.join(vols[0][0] + vols[1][0])
    data = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(cuda)
    n0, n1 = 32 * 8 * 12, 32 * 16 * 9
    vtable = [(8, 12, 0, 0), (16, 9, n0, n0)]
    ok0 = (3, 5, 3, 5, 0, len(vols[0][0][0]), vols[0][1][0], 0)
    ok1 = (12, 5, 3, 4, 0, len(vols[0][0][0]), vols[0][1][0], 1)         # rows 12..14 exist in volume 1 only
    need = _lib.lib.ic_pc_decode_tiles_batch_workspace_bytes(32, 3, 5, 2, 2, pred.pc._k)
    centers = pred.centers.contiguous().float()

    def call(tiles, outputs='both', nvolumes=2, workspace_bytes=need):
        sym, q, ws = _guarded(8 * (n0 + n1), cuda), _guarded(4 * (n0 + n1), cuda), _guarded(need, cuda)
        status = torch.full((8,), -7, dtype=torch.int32, device=cuda)
        rc = _lib.lib.ic_pc_decode_tiles_batch_f32(
            _lib.ptr(data), len(blob), _lib.tile_table(tiles), len(tiles), _lib.volume_table(vtable), nvolumes, pred.pc._tab,
            _lib.ptr(centers), pred.pc._k, pred.pc.L, pred.freqs_resolution, _lib.ptr(sym) if outputs in ('both', 'symbols') else None,
            _lib.ptr(q) if outputs in ('both', 'q') else None, _lib.ptr(status), 32, _lib.ptr(ws), workspace_bytes, 0,
            _lib.current_stream(cuda))
        torch.cuda.synchronize()
        untouched = bool((sym == GUARD).all()) and bool((q == GUARD).all()) and bool((ws == GUARD).all()) and bool((status == -7).all())
        return rc, untouched

    assert call([ok0, ok1])[0] == 0                                       # the table the bad ones are variations of
    assert call([ok0, ok1[:7] + (2,)]) == (-1, True)                       # volume index out of range
    assert call([ok0, ok1[:7] + (-1,)]) == (-1, True)
    assert call([ok0, ok1], nvolumes=1) == (-1, True)
    assert call([ok0, ok1[:7] + (0,)]) == (-1, True)                       # outside its own volume though inside another
    assert call([ok0, ok1], outputs='none') == (-1, True)                  # both outputs NULL
    for short in (0, need // 2, need - 1):
        assert call([ok0, ok1], workspace_bytes=short) == (-3, True)       # short workspace


# ---- 5: chunks ----------------------------------------------------------------------------------------------------------------

def test_chunked_decode_equals_one_chunk(cuda, codecs, images, monkeypatch):
    from imgcomp_cvpr_amd import _lib, codec, probclass
    c, tile = codecs[None], (16, 16)
    pred = c.pred
    vols, want = _coded_volumes(c, images, tile)
    assert sum(len(v[0]) for v in vols) == 28                              # 1 + 1 + 1 + 1 + 24 tiles
    calls = []
    real = _lib.lib.ic_pc_decode_tiles_batch_f32
    monkeypatch.setattr(probclass.lib, 'ic_pc_decode_tiles_batch_f32', lambda *a: calls.append(a[3]) or real(*a))
    whole = pred.decode_tiles_batch(vols, *tile, want='both')
    assert calls == [28]
    for n, (q, s) in enumerate(whole):
        assert s.is_cuda and q.is_cuda and s.dtype == torch.int64 and q.dtype == torch.float32
        assert torch.equal(s, want[n]) and torch.equal(q, pred.centers.float()[s]), n
    budget = int(_lib.lib.ic_pc_decode_tiles_batch_workspace_bytes(32, 16, 16, 8, len(vols), pred.pc._k))
    del calls[:]
    parts = pred.decode_tiles_batch(vols, *tile, want='both', max_workspace_bytes=budget)
    assert len(calls) >= 3 and sum(calls) == 28 and max(calls) <= 8, calls
    for n in range(len(vols)):
        assert torch.equal(parts[n][0], whole[n][0]) and torch.equal(parts[n][1], whole[n][1]), n
    for kind, pick in (('q', 0), ('symbols', 1)):
        one = pred.decode_tiles_batch(vols, *tile, want=kind, max_workspace_bytes=budget)
        assert all(torch.equal(one[n], whole[n][pick]) for n in range(len(vols))), kind
    one_slot = int(_lib.lib.ic_pc_decode_tiles_batch_workspace_bytes(32, 8, 12, 1, len(vols), pred.pc._k))
    del calls[:]
    with pytest.raises(ValueError, match='budget'):
        pred.decode_tiles_batch(vols, *tile, max_workspace_bytes=one_slot - 1)
    assert calls == []
    # the encoder side: the streams of encode_tiles, volume by volume
    coded = pred.encode_tiles_batch(want, *tile)
    assert [([b for b, _ in v], [f for _, f in v]) for v in coded] == [(v[0], v[1]) for v in vols]


# ---- 6: damage stays put ------------------------------------------------------------------------------------------------------

def _rebuild(head, **changes):
    from imgcomp_cvpr_amd import codec
    d = head._asdict()
    d.update(changes)
    return codec.build_tiled_container(d['ae_name'], d['pc_name'], d['H'], d['W'], d['C'], d['h'], d['w'], d['L'], d['resolution'],
                                       d['fingerprint'], d['th'], d['tw'], d['first_syms'], d['streams'])


def test_a_damaged_tile_stays_in_its_file(cuda, codecs, files, pixels):
    """one tile's stream of one file replaced by other bytes of equal length, the container rebuilt with a valid CRC: the decoder is
    specified for such a stream (test_a_damaged_tile_stays_alone).  Either that tile's status raises with the file named, or only
    that tile's symbols differ; every other file decodes as before."""
    from imgcomp_cvpr_amd import codec
    c, tile = codecs[None], (16, 16)
    good = [files[tile][i] for i in (1, 4, 3)]
    head = codec.parse_container(good[1])
    victim = 9
    streams = list(head.streams)
    assert len(streams[victim]) >= 8
    streams[victim] = bytes(b ^ 0x5A for b in reversed(streams[victim]))
    bad = [good[0], _rebuild(head, streams=streams), good[2]]
    assert codec.parse_container(bad[1]).streams[victim] != head.streams[victim] and len(bad[1]) == len(good[1])
    heads = [codec.parse_container(f) for f in bad]
    vols = [(h.streams, h.first_syms, (h.C, h.h, h.w)) for h in heads]
    ref = c.pred.decode_tiles_batch([(h.streams, h.first_syms, (h.C, h.h, h.w)) for h in map(codec.parse_container, good)], *tile,
                                    want='symbols')
    try:
        got = c.pred.decode_tiles_batch(vols, *tile, want='symbols')
    except ValueError as e:
        assert 'volume 1, tile {} '.format(victim) in str(e), e
        with pytest.raises(ValueError, match='file 1: decoder status is not 0'):
            c.decompress_many(bad)
    else:
        y0, x0, a, b = codec.tile_grid(head.h, head.w, *tile)[victim]
        same = got[1] == ref[1]
        assert not bool(same[:, y0:y0 + a, x0:x0 + b].all()), 'the damaged tile decoded as if nothing had happened'
        same[:, y0:y0 + a, x0:x0 + b] = True
        assert bool(same.all()), 'symbols outside the damaged tile changed'
        assert torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2])
        out = c.decompress_many(bad)
        assert np.array_equal(out[0], pixels[tile][1]) and np.array_equal(out[2], pixels[tile][3])
        assert out[1].shape == pixels[tile][4].shape and not np.array_equal(out[1], pixels[tile][4])
    # the undamaged neighbours alone, in the same object, still decode
    assert all(np.array_equal(a, b) for a, b in zip(c.decompress_many([good[0], good[2]]), [pixels[tile][1], pixels[tile][3]]))


def test_a_refused_file_stops_the_batch_before_the_device(codecs, files, monkeypatch):
    from imgcomp_cvpr_amd import codec
    c, tile = codecs[None], (16, 16)
    calls = []
    for name in ('decode_tiles_batch', 'decode_tiles', 'decode_stream'):
        monkeypatch.setattr(c.pred, name, lambda *a, _n=name, **k: calls.append(_n))
    head = codec.parse_container(files[tile][3])
    foreign = _rebuild(head, fingerprint=head.fingerprint ^ 1)
    with pytest.raises(ValueError, match='file 1: model fingerprint mismatch'):
        c.decompress_many([files[tile][0], foreign, files[tile][4]])
    flipped = bytearray(files[None][2])
    flipped[len(flipped) // 2] ^= 1
    with pytest.raises(ValueError, match='file 2: CRC mismatch'):
        c.decompress_many([files[tile][0], files[None][1], bytes(flipped)])
    with pytest.raises(ValueError, match='file 0: truncated file'):
        c.decompress_many([b'ICVF', files[tile][0]])
    assert calls == []


# ---- 7: the command line ------------------------------------------------------------------------------------------------------

def _cli(args, timeout):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    return subprocess.run([sys.executable, '-m', 'imgcomp_cvpr_amd.codec'] + args, cwd=ROOT, env=env, timeout=timeout,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


def test_cli_directories_in_fresh_processes(codecs, tmp_path):
    from PIL import Image
    src, mid, dst = tmp_path / 'in', tmp_path / 'icf', tmp_path / 'out'
    src.mkdir()
    imgs = {'b': _image(200, 328, seed=12), 'a': _image(61, 93, seed=13), 'c': _image(64, 96, seed=14)}
    for stem, img in imgs.items():
        Image.fromarray(img).save(str(src / (stem + '.png')))
    r = _cli(['compress-dir', str(src), str(mid), '--tile', '128', '--batch', '2'], 600)      # two calls: 2 files, then 1
    assert r.returncode == 0, r.stderr
    print(r.stdout.strip())
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 4 and [os.path.basename(l.split(':')[0]) for l in lines[:3]] == ['a.icf', 'b.icf', 'c.icf']
    assert '6 tiles' in lines[1] and 'bpp' in lines[0] and lines[3].startswith('total: 3 files')
    r = _cli(['decompress-dir', str(mid), str(dst)], 600)
    assert r.returncode == 0, r.stderr
    print(r.stdout.strip())
    assert len(r.stdout.strip().splitlines()) == 4 and 'total: 3 files' in r.stdout
    tiled, plain = codecs[(16, 16)], codecs[None]
    for stem, img in imgs.items():
        data = open(str(mid / (stem + '.icf')), 'rb').read()
        assert data == tiled.compress(img), stem
        assert np.array_equal(np.asarray(Image.open(str(dst / (stem + '.png')))), plain.decompress(data)), stem
    assert sorted(os.listdir(str(mid))) == ['a.icf', 'b.icf', 'c.icf'] and sorted(os.listdir(str(dst))) == ['a.png', 'b.png', 'c.png']


# ---- 8: one launch, not N -----------------------------------------------------------------------------------------------------

def test_one_launch_for_four_files_beats_four_launches(cuda, codecs):
    """4 images of 256 x 384 at 16 x 16 tiles: 6 tiles each, 24 work-groups in all -- under a tenth of the device's compute units,
    so one launch over all of them should take about as long as one file's.  Asserted: median of 5 batch calls < median of 5 loops
    of 4 decode_tiles calls, nothing more; the ratios are in profiles/codec_batch_timing.json."""
    c, tile = codecs[None], (16, 16)
    pred = c.pred
    vols, want = _coded_volumes(c, [_image(256, 384, seed=40 + i) for i in range(4)], tile)
    assert [len(v[0]) for v in vols] == [6] * 4

    def loop():
        return [pred.decode_tiles(s, f, shape, *tile) for s, f, shape in vols]

    def batch():
        return pred.decode_tiles_batch(vols, *tile, want='symbols')

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for fn in (loop, batch):                                               # warm-up: allocator, code objects
        _, out = timed(fn)
        for n in range(4):
            assert np.array_equal(out[n] if isinstance(out[n], np.ndarray) else out[n].cpu().numpy(), want[n].cpu().numpy())
    t_loop = [timed(loop)[0] for _ in range(5)]
    t_batch = [timed(batch)[0] for _ in range(5)]
    m_loop, m_batch = statistics.median(t_loop), statistics.median(t_batch)
    print('decode 4 x (32, 32, 48) at 16 x 16 tiles: loop of decode_tiles {:.2f} ms (min {:.2f}, max {:.2f}), one decode_tiles_batch '
          '{:.2f} ms (min {:.2f}, max {:.2f}), ratio {:.3f}'.format(1e3 * m_loop, 1e3 * min(t_loop), 1e3 * max(t_loop), 1e3 * m_batch,
                                                                    1e3 * min(t_batch), 1e3 * max(t_batch), m_batch / m_loop))
    assert m_batch < m_loop
