"""-m gpu: wavefront tiles (container format 5) on the device.  The encoder's streams against the Python coder over the parallel
pass's tables permuted by wavefront_order; the wavefront decoder (IC_PC_DECODE_WAVEFRONT) against the symbols that were coded,
against the format-4 file of the same image, and -- with tables under the test's control -- against the host decoder in the hard
coder states and on bytes that no encoder wrote; the flag's refusals; batching; salvage."""
import numpy as np
import pytest
import torch

from tests import codec_cases as cc
from tests.test_cpu_codec_wavefront import LENGTH_MARGIN_PER_STREAM
from tests.test_gpu_codec_decoder import GARBAGE_TABLES, PENDING_PREFIXES, _draw, _floor_volume, _model

pytestmark = pytest.mark.gpu
GUARD = 0xA5


def _image(H, W_, seed=9):
    from imgcomp_cvpr_amd import weights as W
    return np.ascontiguousarray(W.synthetic_image((1, 3, H, W_), 'natural', seed=seed)[0].transpose(1, 2, 0))


@pytest.fixture(scope='module')
def wf(cuda, configs, syn_weights):
    from imgcomp_cvpr_amd import codec
    return codec.Codec(configs[0], configs[1], syn_weights, cuda, tile=(16, 16), order='wavefront')


def _as(c, tile, order='wavefront', checked=False):
    """the module's one codec with other writer settings (they are read when compress runs; reading needs none)"""
    c.tile, c.order, c.checked = tile, order, checked
    return c


# ---- round trips --------------------------------------------------------------------------------------------------------------

SIZES = [(512, 768), (768, 512), (200, 312), (8, 8), (64, 512)]        # (64, 512): one row of 16 x 16 tiles
EXTENTS = [16, 8, 32, 200]                                              # 200: larger than every volume here, one tile


@pytest.mark.parametrize('size', SIZES)
@pytest.mark.parametrize('extent', EXTENTS)
def test_round_trip_symbols_pixels_and_length(wf, size, extent):
    from imgcomp_cvpr_amd import codec
    img = _image(*size)
    tile = (extent, extent)
    sym = wf.encode_symbols(img)[0].symbols[0].cpu().numpy()
    data5 = _as(wf, tile).compress(img)
    data4 = _as(wf, tile, 'raster', True).compress(img)
    _as(wf, tile)
    c5, c4 = codec.parse_container(data5), codec.parse_container(data4)
    assert isinstance(c5, codec.WavefrontContainer) and c5.version == 5 and isinstance(c4, codec.CheckedContainer) and c4.version == 4
    assert c5.first_syms == c4.first_syms and len(c5.streams) == len(c4.streams) == len(codec.tile_grid(c5.h, c5.w, *tile))
    got, head = wf.decode_symbols(data5)
    assert got.dtype == np.int64 and np.array_equal(got, sym) and head == c5
    assert np.array_equal(wf.decode_symbols(data4)[0], sym)
    out5, out4 = wf.decompress(data5), wf.decompress(data4)
    assert out5.shape == img.shape and out5.dtype == np.uint8 and np.array_equal(out5, out4)
    diff = len(c5.payload) - len(c4.payload)
    print('{} x {} tile {}: {} tiles, format 4 payload {} bytes, format 5 {} bytes ({:+d})'.format(
        size[0], size[1], extent, len(c5.streams), len(c4.payload), len(c5.payload), diff))
    assert abs(diff) <= LENGTH_MARGIN_PER_STREAM * len(c5.streams)
    if len(sym.reshape(-1)) > 64 and len(c5.streams) > 0 and max(len(b) for b in c5.streams) > 8:
        assert c5.payload != c4.payload                                   # another order, other bytes


def test_streams_equal_the_python_coder_over_permuted_tables(wf):
    from imgcomp_cvpr_amd import codec
    img = _image(96, 136)                                                 # latent 12 x 17: tiles 8x8, 8x8, 8x1, 4x8, 4x8, 4x1
    sym = wf.encode_symbols(img)[0].symbols[0].cpu().numpy()
    grid = codec.tile_grid(sym.shape[1], sym.shape[2], 8, 8)
    assert [g[2:] for g in grid] == [(8, 8), (8, 8), (8, 1), (4, 8), (4, 8), (4, 1)]
    coded = wf.pred.encode_tiles(sym, 8, 8, order='wavefront')
    raster = wf.pred.encode_tiles(sym, 8, 8)
    c = codec.parse_container(_as(wf, (8, 8)).compress(img))
    _as(wf, (16, 16))
    assert c.streams == [b for b, _ in coded] and c.first_syms == [f for _, f in coded]
    for t, (y0, x0, a, b) in enumerate(grid):
        sub = np.ascontiguousarray(sym[:, y0:y0 + a, x0:x0 + b])
        freqs = wf.pred.get_all(wf.pred.pad_symbols_volume(sub))[1]      # the parallel pass's tables of the tile as its own volume
        order = codec.wavefront_order(*sub.shape)
        flat = sub.reshape(-1)
        host, _ = cc.host_encode(flat[order][1:], freqs[order][1:])
        assert coded[t] == (host, int(flat[0])), 'tile {} {}: not the Python coder over the permuted tables'.format(t, grid[t])
        assert raster[t][1] == coded[t][1]
        back = np.empty(flat.size, np.int64)
        back[order] = [int(flat[0])] + cc.host_decode(host, freqs[order][1:])
        assert np.array_equal(back, flat)
    assert [b for b, _ in coded] != [b for b, _ in raster]


def test_compress_many_agrees_file_by_file(wf):
    imgs = [_image(200, 312, seed=3), _image(64, 96, seed=4), _image(200, 312, seed=5)]
    _as(wf, (16, 16))
    assert wf.compress_many(imgs) == [wf.compress(i) for i in imgs]


# ---- the decoder against the host decoder, tables under the test's control ----------------------------------------------------

def _raw_batch(cuda, pred, volumes, th, tw, flags, want_q=True, slack=4096, check=True):
    """ic_pc_decode_tiles_batch_f32 through the ABI.  volumes: [(streams, first_syms, (C,h,w))].  symbols, q, status and the
    workspace lie in larger allocations whose other cells hold guard values that must survive; the volumes lie `slack` cells
    apart.  -> (return code, [symbols per volume], [q per volume], status list)"""
    from imgcomp_cvpr_amd import _lib, codec
    tiles, blobs, pos, offs, total = [], [], 0, [], slack
    for n, (streams, firsts, (C, h, w)) in enumerate(volumes):
        for t, (y0, x0, a, b) in enumerate(codec.tile_grid(h, w, th, tw)):
            tiles.append((y0, x0, a, b, pos, len(streams[t]), firsts[t], n))
            blobs.append(bytes(streams[t]))
            pos += len(streams[t])
        offs.append(total)
        total += C * h * w + slack
    C = volumes[0][2][0]
    table = _lib.tile_table(tiles)
    vtable = _lib.volume_table([(h, w, o, o) for (_, _, (_, h, w)), o in zip(volumes, offs)])
    data = torch.frombuffer(bytearray(b''.join(blobs)) or bytearray(1), dtype=torch.uint8).to(cuda)
    sym = torch.full((total,), -7, dtype=torch.int64, device=cuda)
    q = torch.full((total,), -12345.625, dtype=torch.float32, device=cuda) if want_q else None
    status = torch.full((len(tiles) + slack,), -7, dtype=torch.int32, device=cuda)
    need = int(_lib.lib.ic_pc_decode_tiles_batch_workspace_bytes(C, max(t[2] for t in tiles), max(t[3] for t in tiles), len(tiles),
                                                                 len(volumes), pred.pc._k))
    ws = torch.full((need + slack,), GUARD, dtype=torch.uint8, device=cuda)
    centers = pred.centers.contiguous().float()
    rc = _lib.lib.ic_pc_decode_tiles_batch_f32(_lib.ptr(data), pos, table, len(tiles), vtable, len(volumes), pred.pc._tab,
                                               _lib.ptr(centers), pred.pc._k, pred.pc.L, pred.freqs_resolution, _lib.ptr(sym), _lib.ptr(q),
                                               _lib.ptr(status), C, _lib.ptr(ws), need, int(flags), _lib.current_stream(cuda))
    torch.cuda.synchronize()
    assert bool((ws[need:] == GUARD).all()), 'workspace: written behind its stated size'
    assert bool((status[len(tiles):] == -7).all()), 'status: written behind the table'
    keep = torch.ones(total, dtype=torch.bool, device=cuda)
    for (_, _, (c, h, w)), o in zip(volumes, offs):
        keep[o:o + c * h * w] = False
    assert bool((sym[keep] == -7).all()), 'symbols: written outside the volumes'
    if want_q:
        assert bool((q[keep] == -12345.625).all()), 'q: written outside the volumes'
    if rc != 0:
        assert bool((sym == -7).all()) and bool((status == -7).all()), 'a refused call wrote something'
        return rc, None, None, None
    cut = lambda buf: [buf[o:o + c * h * w].view(c, h, w) for (_, _, (c, h, w)), o in zip(volumes, offs)]
    syms = cut(sym)
    if want_q:
        for s, qq in zip(syms, cut(q)):
            assert torch.equal(qq, centers[s]), 'q is not centers[symbols]'
    return rc, [s.cpu().numpy() for s in syms], q, status[:len(tiles)].tolist()


def _wave_ref(table):
    """a constant table: the uncoded first symbol, then the host decoder over the bytes, each symbol at its wavefront position"""
    from imgcomp_cvpr_amd import codec

    def ref(data, first, shape):
        n = int(np.prod(shape))
        out = np.empty(n, np.int64)
        out[codec.wavefront_order(*shape)] = [first] + cc.host_decode(data, [table] * (n - 1))
        return out.reshape(shape)
    return ref


def _raster_ref(table):
    def ref(data, first, shape):
        n = int(np.prod(shape))
        return np.array([first] + cc.host_decode(data, [table] * (n - 1)), np.int64).reshape(shape)
    return ref


def _check_wave(cuda, pred, volumes, th, tw, table, what):
    """every tile of every volume against the host decoder on that tile's own bytes: the Python surface and the raw entry, all
    status words 0"""
    from imgcomp_cvpr_amd import _lib, codec
    ref = _wave_ref(table)
    wants = []
    for streams, firsts, shape in volumes:
        want = np.full(shape, -1, np.int64)
        for t, (y0, x0, a, b) in enumerate(codec.tile_grid(shape[1], shape[2], th, tw)):
            want[:, y0:y0 + a, x0:x0 + b] = ref(streams[t], firsts[t], (shape[0], a, b))
        wants.append(want)
    rc, syms, _, status = _raw_batch(cuda, pred, volumes, th, tw, _lib.PC_DECODE_WAVEFRONT)
    assert rc == 0 and status == [0] * len(status), (what, rc, status)
    for n, (s, want) in enumerate(zip(syms, wants)):
        assert np.array_equal(s, want), '{}: volume {} differs from the host decoder in wavefront positions'.format(what, n)
    both = pred.decode_tiles_batch(volumes, th, tw, want='both', order='wavefront')
    centers = pred.centers.contiguous().float()
    for (q, s), want in zip(both, wants):
        assert np.array_equal(s.cpu().numpy(), want) and torch.equal(q, centers[s]), what
    return wants


def _wave_round_trip(cuda, pred, table, syms, tile, what):
    """volumes the encoder wrote in wavefront order: its streams are the host coder's on the permuted sequence, the decoder
    returns the volumes, which is also what the host decoder makes of the bytes"""
    from imgcomp_cvpr_amd import codec
    vols = []
    for sym in syms:
        coded = pred.encode_tiles(sym, tile[0], tile[1], order='wavefront')
        for (data, first), (y0, x0, a, b) in zip(coded, codec.tile_grid(sym.shape[1], sym.shape[2], *tile)):
            flat = sym[:, y0:y0 + a, x0:x0 + b].reshape(-1)
            order = codec.wavefront_order(sym.shape[0], a, b)
            host, _ = cc.host_encode(flat[order][1:], [table] * (flat.size - 1))
            assert first == int(flat[0]) and data == host, '{}: the encoder differs from the host coder'.format(what)
        vols.append(([b for b, _ in coded], [f for _, f in coded], sym.shape))
    wants = _check_wave(cuda, pred, vols, tile[0], tile[1], table, what)
    for want, sym in zip(wants, syms):
        assert np.array_equal(want, sym), what
    return vols


@pytest.mark.parametrize('bias,run_sym', [((0, 40, 40, 40, 40, 40), 0), ((40, 40, 40, 40, 40, 0), 5)])
def test_floor_frequency_symbols(cuda, bias, run_sym):
    """runs of the symbol of frequency 1, about 30 bits each: the worst a table can cost (codec_cases.worst_case_logits)"""
    pred, table = _model(cuda, list(bias))
    assert table[run_sym] == 1
    rs = np.random.RandomState(17)
    sym = _floor_volume(rs, table, run_sym, (6, 5, 8), 3)
    other = _floor_volume(rs, table, run_sym, (6, 4, 9), 1)
    _wave_round_trip(cuda, pred, table, [sym, other, sym], (3, 5), 'floor frequency, bias {}'.format(bias))


@pytest.mark.parametrize('bias', [(0, 0, 0), (0, 1, 2, 3, 2, 1)])
def test_pending_run_longer_than_64(cuda, bias):
    """codec_cases.straddle_symbols in CODING order: the volume holds the run at its wavefront positions"""
    from imgcomp_cvpr_amd import codec
    pred, table = _model(cuda, list(bias))
    shape, steps = (4, 4, 6), 60
    order = codec.wavefront_order(*shape)
    for lead in (0, 1, 3, 6):
        prefix = PENDING_PREFIXES[lead]
        run, reached = cc.straddle_symbols(table, steps, prefix)
        rs = np.random.RandomState(40 + lead)
        n = int(np.prod(shape))
        seq = np.array([int(rs.randint(len(table)))] + list(prefix) + run + rs.randint(len(table), size=n - 1 - lead - steps).tolist(), np.int64)
        sym = np.empty(n, np.int64)
        sym[order] = seq
        sym = sym.reshape(shape)
        _, pending = cc.host_encode(seq[1:], [table] * (n - 1))
        assert pending >= reached > 64, (pending, reached)
        # one tile covering the volume carries the run whole; the ragged grid beside it is a plain round trip
        _wave_round_trip(cuda, pred, table, [sym], (4, 6), 'pending run, bias {}, {} leading symbols'.format(bias, lead))
        _wave_round_trip(cuda, pred, table, [sym, _draw(rs, table, (4, 3, 7))], (3, 4), 'pending run, tiles, bias {}'.format(bias))


@pytest.mark.parametrize('bias', GARBAGE_TABLES, ids=['floor L=6', 'exact L=3', 'skewed L=16'])
def test_arbitrary_bytes_constant_tables(cuda, bias):
    """bytes that no encoder wrote: the wavefront decoder returns exactly what the host decoder returns, in wavefront positions,
    every tile on its own string, packed back to back as the container packs them"""
    pred, table = _model(cuda, bias)
    L = len(table)
    rs = np.random.RandomState(60 + L)
    shape, tile, other_shape = (6, 6, 8), (4, 5), (6, 3, 7)
    valid, _ = pred.encode_stream(_draw(rs, table, shape), order='wavefront')
    strings = cc.garbage_strings(valid, seed=70 + L)
    for r in range(0, len(strings), 4):
        picks = [strings[(r + j) % len(strings)] for j in range(4)]
        vol = ([d for _, d in picks], [int(v) for v in rs.randint(L, size=4)], shape)
        other = ([strings[(r + 5) % len(strings)][1], strings[(r + 11) % len(strings)][1]], [int(v) for v in rs.randint(L, size=2)], other_shape)
        _check_wave(cuda, pred, [vol, other, vol], tile[0], tile[1], table, 'bias {}, tiles of {}'.format(bias, [n for n, _ in picks]))
    for name, data in strings:                           # and every string as one tile covering the volume
        _check_wave(cuda, pred, [([data], [int(rs.randint(L))], shape)], shape[1], shape[2], table, 'bias {}, {}'.format(bias, name))


def test_total_over_the_limit_is_status_1(cuda):
    """one over the coder's limit: every tile that codes a symbol reports status 1 -- the host decoder's refusal -- a tile of one
    symbol beside it reports 0 and holds its first symbol, and nothing is written outside the volumes"""
    from imgcomp_cvpr_amd import _lib, arithmetic_coding as ac
    pred, table = _model(cuda, [40, 0, 0, 0], resolution=2.0 ** 30)
    assert sum(table) == ac.MAX_TOTAL + 1
    data = np.random.RandomState(9).randint(0, 256, size=40).astype(np.uint8).tobytes()
    with pytest.raises(ValueError, match='total is too large'):
        cc.host_decode(data, [table] * 23)
    streams, firsts = [data[10 * t:10 * t + 10] for t in range(4)], [0, 1, 2, 3]
    rc, syms, _, status = _raw_batch(cuda, pred, [(streams, firsts, (2, 3, 4))], 2, 3, _lib.PC_DECODE_WAVEFRONT)
    assert rc == 0 and status == [1] * 4 and syms[0].min() >= 0 and syms[0].max() < 4
    rc, syms, _, status = _raw_batch(cuda, pred, [([data[:9], b''], [2, 3], (1, 1, 3))], 1, 2, _lib.PC_DECODE_WAVEFRONT)
    assert rc == 0 and status == [1, 0] and syms[0][0, 0, 0] == 2 and syms[0][0, 0, 2] == 3
    with pytest.raises(ValueError, match=r'total is too large \(volume 0, tile 0 '):
        pred.decode_tiles_batch([([data[:9], b''], [2, 3], (1, 1, 3))], 1, 2, want='symbols', order='wavefront')
    # at the limit the same call is accepted and is the host decoder's
    ok, ok_table = _model(cuda, [40, 0, 0], resolution=2.0 ** 30)
    _check_wave(cuda, ok, [([data[:9], b''], [2, 1], (1, 1, 3))], 1, 2, ok_table, 'total == MAX_TOTAL')


# ---- the flag -----------------------------------------------------------------------------------------------------------------

def test_flag_absent_is_the_raster_decoder_and_refusals(cuda, configs, syn_weights):
    from imgcomp_cvpr_amd import _lib, codec
    pred, table = _model(cuda, [0, 1, 2, 3, 2, 1])
    rs = np.random.RandomState(3)
    sym = _draw(rs, table, (5, 6, 7))
    vols = _wave_round_trip(cuda, pred, table, [sym], (4, 5), 'flag')
    # the same bytes without the flag: the existing entry decodes them in raster order, as before
    ref = _raster_ref(table)
    want = np.full(sym.shape, -1, np.int64)
    for t, (y0, x0, a, b) in enumerate(codec.tile_grid(6, 7, 4, 5)):
        want[:, y0:y0 + a, x0:x0 + b] = ref(vols[0][0][t], vols[0][1][t], (5, a, b))
    rc, syms, _, status = _raw_batch(cuda, pred, vols, 4, 5, 0)
    assert rc == 0 and status == [0] * 4 and np.array_equal(syms[0], want) and not np.array_equal(want, sym)
    assert np.array_equal(pred.decode_tiles_batch(vols, 4, 5, want='symbols', order='raster')[0].cpu().numpy(), want)
    assert np.array_equal(pred.decode_tiles(vols[0][0], vols[0][1], sym.shape, 4, 5), want)
    with pytest.raises(ValueError, match="order is 'raster' or 'wavefront'"):
        pred.decode_tiles_batch(vols, 4, 5, order='diagonal')
    # together with a slow-path flag, or for another width: refused, nothing written
    for extra in (_lib.PC_DECODE_RECOMPUTE, _lib.PC_DECODE_PER_LAYER):
        assert _raw_batch(cuda, pred, vols, 4, 5, _lib.PC_DECODE_WAVEFRONT | extra)[0] == -2
    wide, _ = _model(cuda, [0, 1, 2, 3, 2, 1], 'res_shallow_64')
    assert wide.pc._k == 64
    assert _raw_batch(cuda, wide, vols, 4, 5, _lib.PC_DECODE_WAVEFRONT)[0] == -2
    assert _raw_batch(cuda, wide, vols, 4, 5, 0)[0] == 0
    with pytest.raises(_lib.HipLibraryError):
        wide.decode_tiles_batch(vols, 4, 5, order='wavefront')
    # the codec refuses that model at construction, before anything is written
    from imgcomp_cvpr_amd import config_parser as cp, weights as W
    pc64, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow_64'))
    w64 = W.synthetic_weights(configs[0], pc64)
    with pytest.raises(ValueError, match='k = 24, this one has k = 64'):
        codec.Codec(configs[0], pc64, w64, cuda, tile=(16, 16), order='wavefront')
    with pytest.raises(ValueError, match="order='wavefront' needs a tile extent"):
        codec.Codec(configs[0], configs[1], syn_weights, cuda, order='wavefront')


# ---- batching -----------------------------------------------------------------------------------------------------------------

def test_many_over_a_mix_of_formats(wf):
    from imgcomp_cvpr_amd import _lib, codec
    imgs = [_image(200, 312, seed=11), _image(96, 136, seed=12)]
    settings = [(None, 'raster', False), ((16, 16), 'raster', False), ((16, 16), 'raster', True), ((8, 8), 'raster', True),
                ((16, 16), 'wavefront', False), ((8, 8), 'wavefront', False), ((8, 8), 'wavefront', True)]
    datas = []
    for tile, order, checked in settings:
        _as(wf, tile, order, checked)
        singles = [wf.compress(i) for i in imgs]
        assert wf.compress_many(imgs) == singles, (tile, order, checked)
        datas += singles
    _as(wf, (16, 16))
    assert sorted(set(codec.parse_container(d).version for d in datas)) == [1, 2, 4, 5]
    assert datas[-1] == datas[-3] and datas[-2] == datas[-4]              # checked=True is redundant for format 5
    datas = datas[:-2]
    singles = [wf.decompress(d) for d in datas]
    many = wf.decompress_many(datas)
    assert len(many) == len(singles) and all(np.array_equal(a, b) for a, b in zip(many, singles))
    # a small budget: several chunks per group, the same pixels
    need = int(_lib.lib.ic_pc_decode_tiles_batch_workspace_bytes(wf.C, 16, 16, 3, len(datas), wf.pred.pc._k))
    small = wf.decompress_many(datas, max_workspace_bytes=need)
    assert all(np.array_equal(a, b) for a, b in zip(small, singles))
    for a, img in zip(singles, imgs * (len(datas) // 2)):
        assert a.shape == img.shape


# ---- salvage ------------------------------------------------------------------------------------------------------------------

def test_salvage_of_a_damaged_format_5_file(wf):
    from imgcomp_cvpr_amd import codec
    img = _image(200, 312, seed=21)                                       # latent 25 x 39: 2 x 3 tiles of 16 x 16
    tile = (16, 16)
    good5 = _as(wf, tile).compress(img)
    good4 = _as(wf, tile, 'raster', True).compress(img)
    _as(wf, tile)
    strict, _ = wf.decode_symbols(good5)

    def damaged(data):
        c = codec.parse_container(data)
        start = len(data) - 4 - len(c.payload)
        bad = bytearray(data[:len(data) - 4 - 3])                          # the last stream loses its last three bytes
        bad[start + len(c.streams[0]) + len(c.streams[1]) // 2] ^= 0x10    # a byte of tile 1
        return bytes(bad)

    bad5, bad4 = damaged(good5), damaged(good4)
    for bad in (bad5, bad4):
        with pytest.raises(ValueError):
            wf.decompress(bad)
    assert codec.verify_file(bad5) == (False, '2 of 6 tiles damaged: tile 1 (crc), tile 5 (truncated)')
    img5, rep5 = wf.salvage(bad5)
    img4, rep4 = wf.salvage(bad4)
    assert rep5 == rep4 and [d.index for d in rep5.damaged] == [1, 5] and [d.reason for d in rep5.damaged] == ['crc', 'truncated']
    assert rep5.ntiles == 6 and rep5.file_crc_ok is False
    assert np.array_equal(img5, img4) and img5.shape == img.shape
    # intact tiles: the strict decode's symbols, bit for bit
    c, dmg, _ = codec.parse_salvage(bad5)
    syms, report = wf.pred.decode_tiles_batch([(c.streams, c.first_syms, (c.C, c.h, c.w))], c.th, c.tw, want='symbols', conceal=True,
                                              order='wavefront')
    assert report == [[(1, 'missing'), (5, 'missing')]]
    got = syms[0].cpu().numpy()
    for t, (y0, x0, a, b) in enumerate(codec.tile_grid(c.h, c.w, c.th, c.tw)):
        same = np.array_equal(got[:, y0:y0 + a, x0:x0 + b], strict[:, y0:y0 + a, x0:x0 + b])
        assert same == (t not in (1, 5)), t
    # the batch call, a raster file beside it, and an intact file
    many = wf.salvage_many([bad5, bad4, good5])
    assert np.array_equal(many[0][0], img5) and many[0][1] == rep5 and np.array_equal(many[1][0], img4) and many[1][1] == rep4
    assert np.array_equal(many[2][0], wf.decompress(good5)) and many[2][1].damaged == [] and many[2][1].file_crc_ok is True
