"""-m gpu: every device decoder against the host decoder (arithmetic_coding.ArithmeticDecoder) in the coder states that the
near-uniform tables of the synthetic weights never reach -- symbols at the frequency floor of 1, underflow runs longer than 64
bits, totals at and one over the coder's limit, 2 to 16 centres -- and on byte strings that no encoder wrote.

The decoders compute their own logits, so the tables are put under the test's control through the weights:
codec_cases.constant_table_weights zeroes the last layer's filter, the logits of every position are then exactly its bias, and the
frequency table is one chosen row for the parallel pass, the encoder and every decoder alike.  Every comparison is an equality
(symbols, bytes, status words).

"All decoders" are: decode_stream with flags 0 (activation caches, pc_dec_symbol_wave), PC_DECODE_RECOMPUTE and
PC_DECODE_PER_LAYER (pc_dec_symbol); decode_tiles with one tile covering the volume; decode_tiles on a ragged grid, every tile
against the host decoder on that tile's own bytes; decode_tiles_batch(want='both') with the volume in twice beside another one,
q == centers[symbols] exactly."""
import numpy as np
import pytest
import torch

from imgcomp_cvpr_amd import arithmetic_coding as ac
from tests import codec_cases as cc
from tests.test_gpu_codec import _device_tables
from tests.test_gpu_codec_tiled import _raw_decode_tiles
from tests.util import dev

pytestmark = pytest.mark.gpu
GUARD = 0xA5
COMPARED = {'strings': 0, 'decodes': 0}      # byte strings no encoder wrote, and decoder results compared with the host decoder's
_MODELS = {}


def _flags():
    from imgcomp_cvpr_amd import _lib
    return (0, _lib.PC_DECODE_RECOMPUTE, _lib.PC_DECODE_PER_LAYER)


def _configs(L, pc_name):
    from imgcomp_cvpr_amd import config_parser as cp
    ae_cfg, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc_cfg, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', pc_name))
    ae_cfg.num_centers = L
    return ae_cfg, pc_cfg


def _load(cuda, ae_cfg, pc_cfg, wts, resolution):
    from imgcomp_cvpr_amd import autoencoder, probclass
    ae = autoencoder.get_network_cls(ae_cfg)(ae_cfg).load_weights(wts, cuda)                 # supplies the centres only
    pc = probclass.get_network_cls(pc_cfg)(pc_cfg, num_centers=ae_cfg.num_centers).load_weights(wts, cuda)
    return probclass.PredictionNetwork(pc, pc_cfg, ae.get_centers_variable(), freqs_resolution=resolution)


def _model(cuda, bias, pc_name='res_shallow', resolution=1e9):
    """-> (pred, table): a prediction network whose table is `table` (taken from the device: ic_pc_logits_to_freqs_f32 on the bias
    row) at every position -- asserted here on a random volume, for the parallel pass that the encoder's tables come from"""
    key = (tuple(bias), pc_name, resolution)
    if key not in _MODELS:
        L = len(bias)
        ae_cfg, pc_cfg = _configs(L, pc_name)
        pred = _load(cuda, ae_cfg, pc_cfg, cc.constant_table_weights(ae_cfg, pc_cfg, bias), resolution)
        table = _device_tables(dev(np.asarray(bias, np.float32)[None], cuda), resolution)[0]
        sym = np.random.RandomState(5).randint(0, L, size=(3, 4, 5))
        freqs = pred.get_all(pred.pad_symbols_volume(sym))[1]
        assert freqs.shape == (sym.size, L) and (freqs == table[None]).all(), 'the table is not the bias row at every position'
        _MODELS[key] = (pred, [int(v) for v in table])
        print('bias {} ({}, resolution {:g}): table {}'.format(list(bias), pc_name, resolution, _MODELS[key][1]))
    return _MODELS[key]


def _const_ref(table):
    """the reference for a constant table: the uncoded first symbol, then the host decoder over the bytes -> (C,h,w)"""
    def ref(data, first, shape):
        n = int(np.prod(shape))
        return np.array([first] + cc.host_decode(data, [table] * (n - 1)), np.int64).reshape(shape)
    return ref


def _host_loop_ref(pred, tmp_path):
    """the reference for tables that depend on the context: bit_counter._decode asking pred.get_freqs one context at a time
    (device tables, host ArithmeticDecoder), as the reference project decodes"""
    from imgcomp_cvpr_amd import bit_counter
    memo = {}

    def ref(data, first, shape):
        key = (bytes(data), int(first), tuple(shape))
        if key not in memo:
            path = str(tmp_path / 'stream{}.bin'.format(len(memo)))
            with open(path, 'wb') as f:
                f.write(data)
            padded = (shape[0] + 4, shape[1] + 8, shape[2] + 8)
            out = bit_counter._decode(path, padded, pred.input_ctx_shape, int(first), pred.get_freqs)
            memo[key] = pred.undo_pad_symbols_volume(out).astype(np.int64)
        return memo[key]
    return ref


def _check_volume(pred, data, first, shape, ref, what):
    """the entry points that take one stream for the whole volume -> the reference's symbols"""
    want = ref(data, first, shape)
    for flags in _flags():
        got = pred.decode_stream(data, shape, first, flags=flags)
        assert got.dtype == np.int64 and np.array_equal(got, want), '{}: decode_stream(flags={}) differs from the host decoder'.format(what, flags)
    got = pred.decode_tiles([data], [first], shape, shape[1], shape[2])
    assert np.array_equal(got, want), '{}: decode_tiles with one tile differs from the host decoder'.format(what)
    COMPARED['decodes'] += 4
    return want


def _check_tiled(pred, volumes, th, tw, ref, what):
    """volumes: [(streams, first_syms, (C,h,w))] on the grid of (th, tw) tiles.  Every tile against the reference on that
    tile's own bytes: decode_tiles volume by volume, decode_tiles_batch for all of them at once -> the reference's volumes"""
    from imgcomp_cvpr_amd import codec
    wants = []
    for streams, firsts, shape in volumes:
        want = np.full(shape, -1, np.int64)
        for t, (y0, x0, a, b) in enumerate(codec.tile_grid(shape[1], shape[2], th, tw)):
            want[:, y0:y0 + a, x0:x0 + b] = ref(streams[t], firsts[t], (shape[0], a, b))
        wants.append(want)
        got = pred.decode_tiles(streams, firsts, shape, th, tw)
        assert np.array_equal(got, want), '{}: decode_tiles differs from the host decoder in tiles {}'.format(what, _tiles_that_differ(got, want, th, tw))
    both = pred.decode_tiles_batch(volumes, th, tw, want='both')
    centers = pred.centers.contiguous().float()
    assert len(both) == len(volumes)
    for (q, s), want in zip(both, wants):
        s_host = s.cpu().numpy()
        assert np.array_equal(s_host, want), '{}: decode_tiles_batch differs from the host decoder in tiles {}'.format(what, _tiles_that_differ(s_host, want, th, tw))
        assert q.dtype == torch.float32 and torch.equal(q, centers[s]), '{}: q is not centers[symbols]'.format(what)
    COMPARED['decodes'] += 2 * len(volumes)
    return wants


def _tiles_that_differ(got, want, th, tw):
    from imgcomp_cvpr_amd import codec
    return [t for t, (y0, x0, a, b) in enumerate(codec.tile_grid(want.shape[1], want.shape[2], th, tw))
            if not np.array_equal(got[:, y0:y0 + a, x0:x0 + b], want[:, y0:y0 + a, x0:x0 + b])]


def _round_trip(pred, sym, table, tile, other, what):
    """a volume the encoder wrote: the device stream is the host coder's on the device's table, and all decoders return the
    volume -- which is also what the host decoder makes of the bytes"""
    ref = _const_ref(table)
    flat = sym.reshape(-1)
    stream, first = pred.encode_stream(sym)
    host, pending = cc.host_encode(flat[1:], [table] * (flat.size - 1))
    assert first == int(flat[0]) and stream == host, '{}: encode_stream differs from the host coder'.format(what)
    assert np.array_equal(_check_volume(pred, stream, first, sym.shape, ref, what), sym)
    vols = []
    for v in (sym, other, sym):
        coded = pred.encode_tiles(v, *tile)
        vols.append(([b for b, _ in coded], [f for _, f in coded], v.shape))
    wants = _check_tiled(pred, vols, tile[0], tile[1], ref, what)
    assert np.array_equal(wants[0], sym) and np.array_equal(wants[1], other) and np.array_equal(wants[2], sym)
    return stream, pending


def _draw(rs, table, shape, likely=0.7):
    """symbols of `shape`: drawn from the table's own distribution, with improbable symbols mixed in"""
    p = np.array(table, np.float64) / sum(table)
    n = int(np.prod(shape))
    return np.where(rs.rand(n) < likely, rs.choice(len(table), size=n, p=p), rs.randint(len(table), size=n)).reshape(shape).astype(np.int64)


def _floor_volume(rs, table, run_sym, shape, run_channels):
    """the first `run_channels` channels are one run of the frequency-1 symbol, the rest mixes shorter runs with random symbols"""
    sym = rs.randint(0, len(table), size=shape).astype(np.int64)
    sym[:run_channels] = run_sym
    tail = sym[run_channels:].reshape(-1)
    for start in range(5, tail.size - 12, 31):
        tail[start:start + 12] = run_sym
    sym[run_channels:] = tail.reshape(sym[run_channels:].shape)
    return sym


def _floor_case(cuda, bias, run_sym, pc_name, shape, run_channels, tile):
    pred, table = _model(cuda, bias, pc_name)
    assert table[run_sym] == 1 and min(t for j, t in enumerate(table) if j != run_sym) > 10 ** 8
    rs = np.random.RandomState(17)
    sym = _floor_volume(rs, table, run_sym, shape, run_channels)
    other = _floor_volume(rs, table, run_sym, (shape[0], shape[1] - 1, shape[2] + 1), 1)
    what = 'floor frequency, bias {} ({})'.format(bias, pc_name)
    _round_trip(pred, sym, table, tile, other, what)
    # the run part is a volume of its own (raster order C, H, W and one table): what it costs
    run = sym[:run_channels]
    stream, _ = pred.encode_stream(run)
    bits = 8.0 * len(stream) / (run.size - 1)
    print('{}: {} symbols of frequency 1 cost {:.3f} bits per symbol'.format(what, run.size - 1, bits))
    assert 29.0 <= bits <= 32.0, bits


@pytest.mark.parametrize('bias,run_sym', [((0, 40, 40, 40, 40, 40), 0), ((40, 40, 40, 40, 40, 0), 5)])
def test_floor_frequency_symbols(cuda, bias, run_sym):
    _floor_case(cuda, list(bias), run_sym, 'res_shallow', (6, 5, 8), 3, (3, 5))


PENDING_PREFIXES = {0: (), 1: (0,), 3: (0, 1, 0), 6: (1, 0, 2, 0, 1, 1)}      # leading symbols: the run is released at other bit phases


def _pending_case(cuda, bias, pc_name, leads):
    pred, table = _model(cuda, bias, pc_name)
    shape, steps = (4, 4, 6), 60
    for lead in leads:
        prefix = PENDING_PREFIXES[lead]
        run, reached = cc.straddle_symbols(table, steps, prefix)
        rs = np.random.RandomState(40 + lead)
        n = int(np.prod(shape))
        flat = np.array([int(rs.randint(len(table)))] + list(prefix) + run + rs.randint(len(table), size=n - 1 - lead - steps).tolist(), np.int64)
        assert flat.size == n
        sym = flat.reshape(shape)
        what = 'pending run, bias {} ({}), {} leading symbols'.format(bias, pc_name, lead)
        _, pending = _round_trip(pred, sym, table, (3, 4), _draw(rs, table, (4, 3, 7)), what)
        print('{}: straddle_symbols reached {}, the host coder\'s _pending {} on this sequence'.format(what, reached, pending))
        assert pending >= reached > 64, (pending, reached)


@pytest.mark.parametrize('bias', [(0, 0, 0), (0, 1, 2, 3, 2, 1)])
def test_pending_run_longer_than_64(cuda, bias):
    _pending_case(cuda, list(bias), 'res_shallow', (0, 1, 3, 6))


OTHER_L = {2: [0, 2.5], 3: [3, 0, 1], 8: [4, 0, 1, 2, 0.5, 3, 0, 1.5],
           11: [0.6 * (7 * j % 11) for j in range(11)], 16: [0.45 * (5 * j % 16) for j in range(16)]}


@pytest.mark.parametrize('L', sorted(OTHER_L))
def test_other_numbers_of_centres(cuda, L):
    """pc_dec_symbol_wave<0> and the generic lane loops, up to the 16-lane limit; skewed tables, none with a cumulative boundary
    at half the total"""
    pred, table = _model(cuda, OTHER_L[L])
    assert len(table) == L and len(set(table)) > 1
    rs = np.random.RandomState(L)
    _round_trip(pred, _draw(rs, table, (5, 5, 8)), table, (3, 5), _draw(rs, table, (5, 4, 9)), 'L = {}'.format(L))


def test_k64_floor_and_pending(cuda):
    """cvpr/res_shallow_64 has one decode path, the launch-per-layer loop with pc_dec_symbol: every entry point ends there"""
    assert _model(cuda, [0, 40, 40, 40, 40, 40], 'res_shallow_64')[0].pc._k == 64
    _floor_case(cuda, [0, 40, 40, 40, 40, 40], 0, 'res_shallow_64', (4, 4, 5), 2, (3, 3))
    _pending_case(cuda, [0, 1, 2, 3, 2, 1], 'res_shallow_64', (0, 3))


def test_total_at_the_limit(cuda):
    pred, table = _model(cuda, [40, 0, 0], resolution=2.0 ** 30)
    assert table == [1 << 30, 1, 1] and sum(table) == ac.MAX_TOTAL
    rs = np.random.RandomState(8)

    def draw(shape):                                     # mostly the symbol of frequency 2^30, the 30-bit symbols now and then
        return np.where(rs.rand(*shape) < 0.1, rs.randint(1, 3, size=shape), 0).astype(np.int64)
    sym = draw((6, 5, 8))
    assert (sym > 0).sum() > 10
    _round_trip(pred, sym, table, (3, 5), draw((6, 4, 9)), 'total == MAX_TOTAL')


def _raw_decode(cuda, pred, data, first, shape, flags=0, slack=4096):
    """ic_pc_decode_f32 through the ABI: symbols, status and workspace each lie inside a larger allocation whose tail is
    pre-filled with a guard value that must survive -> (symbols, status)"""
    from imgcomp_cvpr_amd import _lib
    C, h, w = shape
    n = C * h * w
    d = torch.frombuffer(bytearray(data) or bytearray(1), dtype=torch.uint8).to(cuda)
    out = torch.full((n + slack,), -7, dtype=torch.int64, device=cuda)
    status = torch.full((1 + slack,), -7, dtype=torch.int32, device=cuda)
    need = _lib.lib.ic_pc_decode_workspace_bytes(C, h, w, pred.pc._k)
    ws = torch.full((need + slack,), GUARD, dtype=torch.uint8, device=cuda)
    centers = pred.centers.contiguous().float()
    _lib.check(_lib.lib.ic_pc_decode_f32(_lib.ptr(d), len(data), int(first), pred.pc._tab, _lib.ptr(centers), pred.pc._k, pred.pc.L,
                                         pred.freqs_resolution, _lib.ptr(out), _lib.ptr(status), C, h, w, _lib.ptr(ws), need,
                                         int(flags), _lib.current_stream(cuda)), 'ic_pc_decode_f32')
    torch.cuda.synchronize()
    assert bool((out[n:] == -7).all()), 'symbols: written behind the volume'
    assert bool((status[1:] == -7).all()), 'status: written behind the word'
    assert bool((ws[need:] == GUARD).all()), 'workspace: written behind its stated size'
    return out[:n].reshape(C, h, w).cpu().numpy(), int(status[0])


def test_total_over_the_limit_is_status_1(cuda):
    """one over the limit: the encoder refuses, every decoder refuses, the raw status words are 1, and nothing is written outside
    the output buffers.  A status belongs to its volume / tile alone.  With one table for every position every tile that codes a
    symbol is refused, so the neighbour that must stay untouched is a tile of ONE symbol (C = 1, 1 x 1): its only symbol is the
    uncoded first symbol, no table is consulted for it, and its status must be 0 and its symbol its first_sym -- next to a
    refused tile, in the one-launch path and in both tile-after-tile paths."""
    from imgcomp_cvpr_amd import codec
    pred, table = _model(cuda, [40, 0, 0, 0], resolution=2.0 ** 30)
    assert table == [1 << 30, 1, 1, 1] and sum(table) == ac.MAX_TOTAL + 1
    rs = np.random.RandomState(9)
    shape = (2, 3, 4)
    with pytest.raises(ValueError, match='total is too large'):
        pred.encode_stream(rs.randint(0, 4, size=shape))
    data = rs.randint(0, 256, size=40).astype(np.uint8).tobytes()
    with pytest.raises(ValueError, match='total is too large'):
        cc.host_decode(data, [table] * 23)
    assert cc.model_decode(data, [table] * 23) == ([], 1)
    for flags in _flags():
        with pytest.raises(ValueError, match='total is too large'):
            pred.decode_stream(data, shape, 1, flags=flags)
        out, status = _raw_decode(cuda, pred, data, 1, shape, flags)
        assert status == 1 and out.min() >= 0 and out.max() < 4
    with pytest.raises(ValueError, match='total is too large'):
        pred.decode_tiles([data], [1], shape, 3, 4)
    grid = codec.tile_grid(3, 4, 2, 3)
    streams, firsts = [data[10 * t:10 * t + 10] for t in range(4)], [0, 1, 2, 3]
    with pytest.raises(ValueError, match='total is too large'):
        pred.decode_tiles(streams, firsts, shape, 2, 3)
    with pytest.raises(ValueError, match='total is too large'):
        pred.decode_tiles_batch([(streams, firsts, shape), ([data], [2], (2, 2, 3)), (streams, firsts, shape)], 2, 3, want='both')
    for flags in _flags():
        out, status = _raw_decode_tiles(cuda, pred, streams, firsts, shape, grid, flags=flags)
        assert status == [1] * 4 and out.min() >= 0 and out.max() < 4
    # the tile of one symbol beside a refused one
    line, pair = (1, 1, 3), codec.tile_grid(1, 3, 1, 2)
    assert pair == [(0, 0, 1, 2), (0, 2, 1, 1)]
    for flags in _flags():
        out, status = _raw_decode_tiles(cuda, pred, [data[:9], b''], [2, 3], line, pair, flags=flags)
        assert status == [1, 0], (flags, status)
        assert out[0, 0, 0] == 2 and out[0, 0, 2] == 3 and 0 <= out[0, 0, 1] < 4
    with pytest.raises(ValueError, match=r'total is too large \(tile 0 '):
        pred.decode_tiles([data[:9], b''], [2, 3], line, 1, 2)
    # the same call is accepted at the limit, and is the host decoder's
    ok, ok_table = _model(cuda, [40, 0, 0], resolution=2.0 ** 30)
    for flags in _flags():
        out, status = _raw_decode_tiles(cuda, ok, [data[:9], b''], [2, 1], line, pair, flags=flags)
        assert status == [0, 0] and out.reshape(-1).tolist() == [2] + cc.host_decode(data[:9], [ok_table]) + [1]
        out, status = _raw_decode(cuda, ok, data, 1, shape, flags)
        assert status == 0 and np.array_equal(out, _const_ref(ok_table)(data, 1, shape))


GARBAGE_TABLES = [[0, 40, 40, 40, 40, 40], [0, 0, 0], OTHER_L[16]]


@pytest.mark.parametrize('bias', GARBAGE_TABLES, ids=['floor L=6', 'exact L=3', 'skewed L=16'])
def test_arbitrary_bytes_constant_tables(cuda, bias):
    """bytes that no encoder wrote (codec_cases.garbage_strings, the strings of the CPU test): every decoder returns exactly what
    the host decoder returns.  For the tiles every tile gets a string of its own, packed back to back as the container packs
    them: a reader that ran into the next tile's bytes instead of zeros would differ."""
    pred, table = _model(cuda, bias)
    L, ref = len(table), _const_ref(table)
    rs = np.random.RandomState(60 + L)
    shape, tile = (6, 6, 8), (4, 5)
    valid, _ = pred.encode_stream(_draw(rs, table, shape))
    strings = cc.garbage_strings(valid, seed=70 + L)
    for name, data in strings:
        _check_volume(pred, data, int(rs.randint(L)), shape, ref, 'bias {}, {}'.format(bias, name))
    # four tiles (4x5, 4x3, 2x5, 2x3), every string in some tile; the batch has the volume twice beside another one
    other_shape = (6, 3, 7)
    for r in range(0, len(strings), 4):
        picks = [strings[(r + j) % len(strings)] for j in range(4)]
        vol = ([d for _, d in picks], [int(v) for v in rs.randint(L, size=4)], shape)
        other = ([strings[(r + 5) % len(strings)][1], strings[(r + 11) % len(strings)][1]], [int(v) for v in rs.randint(L, size=2)], other_shape)
        _check_tiled(pred, [vol, other, vol], tile[0], tile[1], ref, 'bias {}, tiles of {}'.format(bias, [n for n, _ in picks]))
    COMPARED['strings'] += len(strings)
    print('bias {}: {} byte strings, running totals: {} strings, {} decoder results equal to the host decoder\'s'.format(
        bias, len(strings), COMPARED['strings'], COMPARED['decodes']))


# Chosen on the CPU with the float64 oracle's bitcost logits (oracle.bitcost on this very volume, tables by
# codec_cases.softmax_tables): gain 1 -> no row with a frequency of 1; gain 50 -> 64 % of the rows have one (8 % have five);
# gain 100 -> 97 %.  50 keeps both kinds of rows in one volume.
PEAKY_GAIN = 50.0


@pytest.mark.parametrize('model', ['plain', 'peaky'])
def test_arbitrary_bytes_real_tables(cuda, configs, syn_weights, tmp_path, model):
    """tables that depend on the context, as a trained model's do: the synthetic weights of the fixtures, and the same with the
    last layer scaled until entries at the frequency floor appear.  All decoders against the reference-style host loop that asks
    the device for one table at a time and steps the host ArithmeticDecoder (bit_counter._decode with pred.get_freqs)."""
    ae_cfg, pc_cfg = configs
    wts = dict(syn_weights)
    if model == 'peaky':
        for part in ('/weights', '/biases'):
            wts[cc.LAST_LAYER + part] = syn_weights[cc.LAST_LAYER + part] * np.float32(PEAKY_GAIN)
    pred = _load(cuda, ae_cfg, pc_cfg, wts, 1e9)
    ref = _host_loop_ref(pred, tmp_path)
    rs = np.random.RandomState(31)
    sym = rs.randint(0, 6, size=(3, 8, 12)).astype(np.int64)
    other = rs.randint(0, 6, size=(3, 4, 6)).astype(np.int64)
    freqs = pred.get_all(pred.pad_symbols_volume(sym))[1]
    share = float((freqs == 1).any(axis=1).mean())
    print('{} model: {:.1%} of the {} rows of this volume contain a frequency of 1'.format(model, share, len(freqs)))
    if model == 'peaky':
        assert share >= 0.1, share                       # 64 % expected (see PEAKY_GAIN): never silently the mild case
    tile = (5, 7)
    stream, first = pred.encode_stream(sym)
    coded, coded_other = pred.encode_tiles(sym, *tile), pred.encode_tiles(other, *tile)
    assert len(coded) == 4 and len(coded_other) == 1
    other_vol = ([b for b, _ in coded_other], [f for _, f in coded_other], other.shape)
    noise = lambda n: rs.randint(0, 256, size=n).astype(np.uint8).tobytes()
    cases = [('valid', stream, [b for b, _ in coded]), ('first half', stream[:len(stream) // 2], [b[:len(b) // 2] for b, _ in coded]),
             ('random 40', noise(40), [noise(10) for _ in coded]), ('random 300', noise(300), [noise(80) for _ in coded])]
    for name, data, tiles in cases:
        what = '{} model, {}'.format(model, name)
        want = _check_volume(pred, data, first, sym.shape, ref, what)
        vol = (tiles, [f for _, f in coded], sym.shape)
        wants = _check_tiled(pred, [vol, other_vol, vol], tile[0], tile[1], ref, what)
        assert np.array_equal(wants[1], other)
        if name == 'valid':
            assert np.array_equal(want, sym) and np.array_equal(wants[0], sym)
        else:
            assert not np.array_equal(want, sym)
            COMPARED['strings'] += 1 + len(tiles)
    print('{} model: running totals: {} strings, {} decoder results equal to the host decoder\'s'.format(
        model, COMPARED['strings'], COMPARED['decodes']))
