"""-m gpu: the tiled codec (container format 2).  Every tile is coded as a volume of its own, so every comparison is an equality
with what the single-volume coders give for that sub-volume: encode_tiles against encode_stream (and through it the host coder and
the reference coder's golden streams), decode_tiles -- all tiles in one launch, ic_pc_decode_tiles_f32 -- against the encoder's
symbols and against decode_stream tile by tile."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.util import dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5


def _image(H, W_, seed=9):
    from imgcomp_cvpr_amd import weights as W
    return np.ascontiguousarray(W.synthetic_image((1, 3, H, W_), 'natural', seed=seed)[0].transpose(1, 2, 0))


@pytest.fixture(scope='module')
def plain(cuda, configs, syn_weights):
    from imgcomp_cvpr_amd import codec
    return codec.Codec(configs[0], configs[1], syn_weights, cuda)


def _symbols(c, img):
    return c.encode_symbols(img)[0].symbols[0].cpu().numpy()


def _sub(sym, tile):
    y0, x0, a, b = tile
    return np.ascontiguousarray(sym[:, y0:y0 + a, x0:x0 + b])


CASES = [((61, 93), (3, 5)), ((512, 768), (16, 16))]


@pytest.mark.parametrize('shape,tile', CASES)
def test_tile_streams_equal_single_volume_streams(plain, shape, tile):
    from imgcomp_cvpr_amd import codec
    sym = _symbols(plain, _image(*shape))
    grid = codec.tile_grid(sym.shape[1], sym.shape[2], *tile)
    assert len(grid) == {(3, 5): 9, (16, 16): 24}[tile]
    coded = plain.pred.encode_tiles(sym, *tile)
    assert len(coded) == len(grid)
    for t, g in enumerate(grid):
        sub = _sub(sym, g)
        assert coded[t] == plain.pred.encode_stream(sub), 'tile {} {}: not the stream of its sub-volume'.format(t, g)
        assert coded[t][1] == int(sub.reshape(-1)[0])
        if shape == (61, 93):
            assert coded[t] == plain._host_encode_stream(sub), 'tile {} {}: not the host coder\'s stream'.format(t, g)
    assert len(set(b for b, _ in coded)) > 1


def _raw_decode_tiles(cuda, pred, streams, first_syms, shape, grid, flags=0, slack=4096):
    """ic_pc_decode_tiles_f32 through the ABI: symbols, status and workspace each lie inside a larger allocation whose tail is
    pre-filled with a guard value that must survive -> (symbols, status list)"""
    from imgcomp_cvpr_amd import _lib
    C, h, w = shape
    offs = np.concatenate([[0], np.cumsum([len(b) for b in streams])]).astype(np.int64)
    table = _lib.tile_table([(g[0], g[1], g[2], g[3], offs[t], len(streams[t]), first_syms[t]) for t, g in enumerate(grid)])
    data = torch.frombuffer(bytearray(b''.join(streams)) or bytearray(1), dtype=torch.uint8).to(cuda)
    n = C * h * w
    out = torch.full((n + slack,), -7, dtype=torch.int64, device=cuda)
    status = torch.full((len(grid) + slack,), -7, dtype=torch.int32, device=cuda)
    need = _lib.lib.ic_pc_decode_tiles_workspace_bytes(C, max(g[2] for g in grid), max(g[3] for g in grid), len(grid), pred.pc._k)
    ws = torch.full((need + slack,), GUARD, dtype=torch.uint8, device=cuda)
    centers = pred.centers.contiguous().float()
    _lib.check(_lib.lib.ic_pc_decode_tiles_f32(_lib.ptr(data), int(offs[-1]), table, len(grid), pred.pc._tab, _lib.ptr(centers),
                                               pred.pc._k, pred.pc.L, pred.freqs_resolution, _lib.ptr(out), _lib.ptr(status), C, h, w,
                                               _lib.ptr(ws), need, flags, _lib.current_stream(cuda)), 'ic_pc_decode_tiles_f32')
    torch.cuda.synchronize()
    assert bool((out[n:] == -7).all()), 'symbols: written behind the volume'
    assert bool((status[len(grid):] == -7).all()), 'status: written behind the table'
    assert bool((ws[need:] == GUARD).all()), 'workspace: written behind its stated size'
    return out[:n].reshape(C, h, w).cpu().numpy(), status[:len(grid)].tolist()


@pytest.mark.parametrize('shape,tile', CASES)
def test_decode_tiles_returns_the_symbols(cuda, plain, shape, tile):
    from imgcomp_cvpr_amd import codec
    pred = plain.pred
    sym = _symbols(plain, _image(*shape))
    grid = codec.tile_grid(sym.shape[1], sym.shape[2], *tile)
    coded = pred.encode_tiles(sym, *tile)
    streams, firsts = [b for b, _ in coded], [f for _, f in coded]
    out = pred.decode_tiles(streams, firsts, sym.shape, *tile)
    assert out.dtype == np.int64 and out.shape == sym.shape
    assert np.array_equal(out, sym), 'decode_tiles lost the encoder\'s symbols'
    for t, g in enumerate(grid):                         # the parent's decoder, tile by tile
        assert np.array_equal(pred.decode_stream(streams[t], (sym.shape[0], g[2], g[3]), firsts[t]), _sub(out, g)), (t, g)
    raw, status = _raw_decode_tiles(cuda, pred, streams, firsts, sym.shape, grid)
    assert status == [0] * len(grid) and np.array_equal(raw, sym)
    # the ABI decodes any set of rectangles: the tiles in another order, their streams staying where they are
    if shape == (61, 93):
        from imgcomp_cvpr_amd import _lib
        offs = np.concatenate([[0], np.cumsum([len(b) for b in streams])])
        order = list(reversed(range(len(grid))))
        table = _lib.tile_table([(grid[t][0], grid[t][1], grid[t][2], grid[t][3], offs[t], len(streams[t]), firsts[t]) for t in order])
        data = torch.frombuffer(bytearray(b''.join(streams)), dtype=torch.uint8).to(cuda)
        o2 = torch.full(sym.shape, -1, dtype=torch.int64, device=cuda)
        st = torch.full((len(grid),), -1, dtype=torch.int32, device=cuda)
        need = _lib.lib.ic_pc_decode_tiles_workspace_bytes(sym.shape[0], 3, 5, len(grid), pred.pc._k)
        ws = torch.empty(need, dtype=torch.uint8, device=cuda)
        centers = pred.centers.contiguous().float()
        _lib.check(_lib.lib.ic_pc_decode_tiles_f32(_lib.ptr(data), int(offs[-1]), table, len(grid), pred.pc._tab, _lib.ptr(centers),
                                                   pred.pc._k, pred.pc.L, pred.freqs_resolution, _lib.ptr(o2), _lib.ptr(st),
                                                   sym.shape[0], sym.shape[1], sym.shape[2], _lib.ptr(ws), need, 0,
                                                   _lib.current_stream(cuda)))
        assert st.tolist() == [0] * len(grid) and np.array_equal(o2.cpu().numpy(), sym)


@pytest.mark.parametrize('shape,tile,victim', [((61, 93), (3, 5), 4), ((512, 768), (16, 16), 9)])
def test_a_damaged_tile_stays_alone(plain, shape, tile, victim, tmp_path):
    """the truncated-stream case of test_device_decoder_stream on one tile: its stream cut to the first half (zeros past the end,
    never the next tile's bytes) still decodes to symbols in [0, L); every other tile is exact."""
    from imgcomp_cvpr_amd import codec
    pred = plain.pred
    sym = _symbols(plain, _image(*shape))
    grid = codec.tile_grid(sym.shape[1], sym.shape[2], *tile)
    coded = pred.encode_tiles(sym, *tile)
    streams, firsts = [b for b, _ in coded], [f for _, f in coded]
    assert len(streams[victim]) >= 8
    streams[victim] = streams[victim][:len(streams[victim]) // 2]
    out = pred.decode_tiles(streams, firsts, sym.shape, *tile)
    assert out.min() >= 0 and out.max() < plain.L
    for t, g in enumerate(grid):
        if t != victim:
            assert np.array_equal(_sub(out, g), _sub(sym, g)), 'tile {} changed with the stream of tile {}'.format(t, victim)
    # what the cut tile decodes to is what the single-volume decoder makes of the same cut stream
    g = grid[victim]
    assert np.array_equal(_sub(out, g), pred.decode_stream(streams[victim], (sym.shape[0], g[2], g[3]), firsts[victim]))
    assert not np.array_equal(_sub(out, g), _sub(sym, g))
    if shape == (61, 93):                                # ... and what the host loop makes of it (480 symbols: cheap on the host)
        from imgcomp_cvpr_amd import bit_counter
        path = str(tmp_path / 'cut.bin')
        open(path, 'wb').write(streams[victim])
        ref = bit_counter._decode(path, (sym.shape[0] + 4, g[2] + 8, g[3] + 8), pred.input_ctx_shape, firsts[victim], pred.get_freqs)
        assert np.array_equal(_sub(out, g), pred.undo_pad_symbols_volume(ref))


def test_one_tile_is_the_format_1_payload(cuda, configs, syn_weights, plain):
    from imgcomp_cvpr_amd import codec
    img = _image(61, 93)
    v1 = codec.parse_container(plain.compress(img))
    for tile in ((8, 12), (16, 16), (8, 4096)):
        c = codec.Codec(configs[0], configs[1], syn_weights, cuda, tile=tile)
        v2 = codec.parse_container(c.compress(img))
        assert isinstance(v2, codec.TiledContainer) and v2.version == 2 and (v2.th, v2.tw) == tile
        assert v2.payload == v1.payload and v2.streams == [v1.payload] and v2.first_syms == [v1.first_sym]


@pytest.mark.parametrize('shape,tile', CASES)
def test_tiled_codec_gives_the_untiled_pixels(cuda, configs, syn_weights, plain, shape, tile):
    from imgcomp_cvpr_amd import codec
    img = _image(*shape)
    tiled = codec.Codec(configs[0], configs[1], syn_weights, cuda, tile=tile)
    f1, f2 = plain.compress(img), tiled.compress(img)
    assert codec.parse_container(f1).version == 1 and codec.parse_container(f2).version == 2 and f1 != f2
    want = plain.decompress(f1)
    assert want.shape == img.shape
    # both formats through the same Codec, either one: the file's version decides, not the object's tile option
    for c in (plain, tiled):
        assert np.array_equal(c.decompress(f1), want) and np.array_equal(c.decompress(f2), want)
    s1, _ = plain.decode_symbols(f1)
    s2, head = plain.decode_symbols(f2)
    assert np.array_equal(s1, s2) and len(head.streams) == len(codec.tile_grid(head.h, head.w, *tile))
    # a damaged or foreign tiled file is refused before anything is decoded
    bad = bytearray(f2)
    bad[len(bad) // 2] ^= 1
    with pytest.raises(ValueError, match='CRC'):
        plain.decompress(bytes(bad))
    print('{} x {}: untiled payload {} bytes, file {}; tiles {} x {}: payload {} bytes, file {}'.format(
        shape[0], shape[1], len(codec.parse_container(f1).payload), len(f1), tile[0], tile[1], len(head.payload), len(f2)))


def _pred_for(cuda, L, pc_name):
    from imgcomp_cvpr_amd import autoencoder, probclass, config_parser as cp, weights as W
    ae_cfg, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc_cfg, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', pc_name))
    ae_cfg.num_centers = L
    wts = W.synthetic_weights(ae_cfg, pc_cfg)
    ae = autoencoder.get_network_cls(ae_cfg)(ae_cfg).load_weights(wts, cuda)
    pc = probclass.get_network_cls(pc_cfg)(pc_cfg, num_centers=L).load_weights(wts, cuda)
    return ae, probclass.PredictionNetwork(pc, pc_cfg, ae.get_centers_variable())


def test_other_number_of_centres(cuda):
    """L = 8: the generic lane loops of pc_dec_symbol_wave<0>, on the 3 x 9 plane of a 24 x 72 image cut into 2 x 4 tiles"""
    from imgcomp_cvpr_amd import codec, weights as W
    ae, pred = _pred_for(cuda, 8, 'res_shallow')
    sym = ae.encode(dev(W.synthetic_image((1, 3, 24, 72), 'natural', seed=8), cuda), False).symbols[0].cpu().numpy()
    assert sym.shape == (32, 3, 9) and sym.max() < 8
    grid = codec.tile_grid(3, 9, 2, 4)
    coded = pred.encode_tiles(sym, 2, 4)
    assert len(coded) == len(grid) == 6
    for t, g in enumerate(grid):
        assert coded[t] == pred.encode_stream(_sub(sym, g))
    out = pred.decode_tiles([b for b, _ in coded], [f for _, f in coded], sym.shape, 2, 4)
    assert np.array_equal(out, sym)


@pytest.mark.parametrize('flag', ['PC_DECODE_PER_LAYER', 'PC_DECODE_RECOMPUTE'])
def test_slow_path_flags(cuda, plain, flag):
    """the two test flags of ic_pc_decode_f32 take the tile-after-tile loop (small image on purpose: the per-layer path costs tens
    of microseconds per symbol)"""
    from imgcomp_cvpr_amd import _lib, codec
    pred = plain.pred
    sym = _symbols(plain, _image(61, 93))
    coded = pred.encode_tiles(sym, 3, 5)
    streams, firsts = [b for b, _ in coded], [f for _, f in coded]
    out = pred.decode_tiles(streams, firsts, sym.shape, 3, 5, flags=getattr(_lib, flag))
    assert np.array_equal(out, sym)
    raw, status = _raw_decode_tiles(cuda, pred, streams, firsts, sym.shape, codec.tile_grid(8, 12, 3, 5), flags=getattr(_lib, flag))
    assert status == [0] * 9 and np.array_equal(raw, sym)


def test_k64_takes_the_slow_path(cuda):
    """cvpr/res_shallow_64 has no activation-cache decoder: tile after tile through the launch-per-layer loop.  The single-volume
    decoder round-trips this 16 x 24 image (checked first: the suite had no decode test for k = 64 before this one), then 1 x 2
    tiles of its 2 x 3 plane."""
    from imgcomp_cvpr_amd import codec, weights as W
    ae, pred = _pred_for(cuda, 6, 'res_shallow_64')
    assert pred.pc._k == 64
    sym = ae.encode(dev(W.synthetic_image((1, 3, 16, 24), 'natural', seed=5), cuda), False).symbols[0].cpu().numpy()
    assert sym.shape == (32, 2, 3)
    stream, first = pred.encode_stream(sym)
    assert np.array_equal(pred.decode_stream(stream, sym.shape, first), sym), 'single-volume decoder, k = 64'
    grid = codec.tile_grid(2, 3, 1, 2)
    coded = pred.encode_tiles(sym, 1, 2)
    assert len(coded) == len(grid) == 4
    for t, g in enumerate(grid):
        assert coded[t] == pred.encode_stream(_sub(sym, g))
    out = pred.decode_tiles([b for b, _ in coded], [f for _, f in coded], sym.shape, 1, 2)
    assert np.array_equal(out, sym)


def _cli(args, timeout):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    return subprocess.run([sys.executable, '-m', 'imgcomp_cvpr_amd.codec'] + args, cwd=ROOT, env=env, timeout=timeout,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


def test_cli_tile_in_fresh_processes(cuda, configs, syn_weights, plain, tmp_path):
    from PIL import Image
    from imgcomp_cvpr_amd import codec
    img = _image(200, 328, seed=12)                       # latent 25 x 41: 2 x 3 tiles of 16 x 16, edge tiles 9 high and 9 wide
    src, icf, png = str(tmp_path / 'in.png'), str(tmp_path / 'out.icf'), str(tmp_path / 'back.png')
    Image.fromarray(img).save(src)
    r = _cli(['compress', src, icf, '--tile', '128'], 600)
    assert r.returncode == 0, r.stderr
    print(r.stdout.strip())
    assert 'bpp' in r.stdout and '6 tiles' in r.stdout
    r = _cli(['decompress', icf, png], 600)                # no option: the file says that it is tiled
    assert r.returncode == 0, r.stderr
    data = open(icf, 'rb').read()
    assert data == codec.Codec(configs[0], configs[1], syn_weights, cuda, tile=(16, 16)).compress(img)
    assert np.array_equal(np.asarray(Image.open(png)), plain.decompress(plain.compress(img)))
    for bad in ('100', '0', '-128'):
        r = _cli(['compress', src, str(tmp_path / 'no.icf'), '--tile', bad], 600)
        assert r.returncode != 0 and 'multiple of the subsampling factor 8' in r.stderr, (bad, r.returncode, r.stderr)
        assert not os.path.exists(str(tmp_path / 'no.icf'))
