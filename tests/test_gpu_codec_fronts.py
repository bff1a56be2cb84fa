"""-m gpu: front-layered tiles (container format 8) -- the encoder (the wavefront gather in front of ic_pc_encode_segments_f32) against the
host coder over the permuted tables cut at front_layer_cuts, the wavefront tile decoder that restarts at front cuts
(ic_pc_decode_tiles_batch_fronts_f32, ic_pc_decode_tiles_batch_fronts_pertile_f32) against the coded symbols, the preview rule, the
format-5 preview decoder and, with tables under the test's control, the word-level model of the decoder restarted at the cuts; then
whole files against formats 5 and 6.  Every comparison is an equality."""
import ctypes

import numpy as np
import pytest
import torch

from tests import codec_cases as cc
from tests import recover_rule as RR
from tests.test_gpu_codec_decoder import GARBAGE_TABLES, PENDING_PREFIXES, _draw, _load, _model
from tests.test_gpu_codec_layered import GUARD, Q_GUARD, SHAPES, SYM_GUARD, _ends_variants, _image

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pred(cuda, configs, syn_weights):
    return _load(cuda, configs[0], configs[1], syn_weights, 1e9)


# ---- the encoder --------------------------------------------------------------------------------------------------------------

def _host_front_segments(pred, tile_chw, ends):
    """the host coder over get_all's tables of the tile as a volume of its own, permuted through wavefront_order and cut at the cuts"""
    from imgcomp_cvpr_amd import codec
    C, a, b = tile_chw.shape
    order = codec.wavefront_order(C, a, b)
    freqs = np.asarray(pred.get_all(pred.pad_symbols_volume(tile_chw))[1])[order]
    flat = tile_chw.reshape(-1).astype(np.int64)[order]
    cuts = codec.front_layer_cuts(C, a, b, ends)
    return [cc.host_encode(flat[max(1, lo):hi], freqs[max(1, lo):hi])[0] for lo, hi in zip([0] + cuts, cuts)]


def _coded(pred, syms, th, tw, ends):
    vols = []
    for sym in syms:
        coded = pred.encode_tiles(sym, th, tw, front_ends=ends)
        vols.append(([s for s, _ in coded], [f for _, f in coded], tuple(sym.shape)))
    return vols


def _coded5(pred, syms, th, tw):
    vols = []
    for sym in syms:
        coded = pred.encode_tiles(sym, th, tw, order='wavefront')
        vols.append(([s for s, _ in coded], [f for _, f in coded], tuple(sym.shape)))
    return vols


@pytest.mark.parametrize('shape', SHAPES + [(6, 5, 7)])
def test_encoder_segments_are_the_host_coders(pred, shape):
    from imgcomp_cvpr_amd import codec
    C = shape[0]
    th, tw = (4, 4) if shape == (6, 5, 7) else shape[1:]                      # (6, 5, 7): four tiles of three extents, the others one tile
    rs = np.random.RandomState(sum(shape))
    syms = [rs.randint(0, pred.pc.L, size=shape).astype(np.int64) for _ in range(2)]
    grid = codec.tile_grid(shape[1], shape[2], th, tw)
    fives = _coded5(pred, syms, th, tw)
    for ends in _ends_variants(C):
        vols = _coded(pred, syms, th, tw, ends)
        batch = pred.encode_tiles_batch(syms, th, tw, front_ends=ends)
        for n, sym in enumerate(syms):
            assert [s for s, _ in batch[n]] == vols[n][0] and [f for _, f in batch[n]] == vols[n][1]
            for t, (y0, x0, a, b) in enumerate(grid):
                assert vols[n][0][t] == _host_front_segments(pred, sym[:, y0:y0 + a, x0:x0 + b], ends), (shape, ends, n, t)
                assert vols[n][1][t] == int(sym[0, y0, x0])
                if len(ends) == 1:
                    assert vols[n][0][t][0] == fives[n][0][t]                 # G = 1: the format-5 stream, byte for byte
                if ends[0] == 1 and a == 1 and b == 1:
                    assert vols[n][0][t][0] == b'\x80'                        # the empty segment
    for kw in (dict(layer_ends=[C]), dict(order='wavefront')):
        with pytest.raises(ValueError, match='front_ends cuts the wavefront order at fronts by itself'):
            pred.encode_tiles(syms[0], th, tw, front_ends=[C], **kw)


# ---- the decoder through the ABI ----------------------------------------------------------------------------------------------

def _raw_fronts(cuda, pred, volumes, th, tw, ends, K, fill, limits=None, want_syms=True, want_q=True, flags=0, unneeded='real', nlayers=None,
                ws_short=0, break_seg=None, slack=4096):
    """ic_pc_decode_tiles_batch_fronts_f32 (limits None: the limit K for all tiles) or ic_pc_decode_tiles_batch_fronts_pertile_f32 (limits:
    one per tile, all volumes in order) through the ABI.  volumes: [(streams, first_syms, (C,h,w))], streams[t] the tile's list of
    segments.  unneeded: what stands for a tile's segments of layers that begin at or above its limit -- 'real' (their bytes), 'zero'
    ({0, 0}), 'other' (other bytes at another place).  symbols, q, status and the workspace carry guard values; the volumes lie
    `slack` cells apart.  The tile descriptors' stream fields hold nonsense: they are not read.
    -> (return code, [symbols per volume] or None, [q per volume, device] or None, status list)"""
    from imgcomp_cvpr_amd import _lib, codec
    G = len(ends)
    junk = bytes(np.random.RandomState(97).randint(0, 256, size=43).astype(np.uint8))
    tiles, segs, blobs, pos, offs, total = [], [], [junk], len(junk), [], slack
    for n, (streams, firsts, (C, h, w)) in enumerate(volumes):
        for t, (y0, x0, a, b) in enumerate(codec.tile_grid(h, w, th, tw)):
            k_t = K if limits is None else limits[len(tiles)]
            tiles.append((y0, x0, a, b, -5, 1 << 40, firsts[t], n))
            for g in range(len(streams[t])):
                needed = g == 0 or (g - 1 < len(ends) and ends[g - 1] < k_t)
                if needed or unneeded == 'real':
                    segs.append((pos, len(streams[t][g])))
                    blobs.append(bytes(streams[t][g]))
                    pos += len(streams[t][g])
                else:
                    segs.append((0, 0) if unneeded == 'zero' else (4, len(junk) - 4))
        offs.append(total)
        total += C * h * w + slack
    assert limits is None or len(limits) == len(tiles)
    if break_seg is not None:
        i, seg = break_seg
        segs[i] = seg(pos)
    C = volumes[0][2][0]
    table, seg_table = _lib.tile_table(tiles), _lib.seg_table(segs)
    vtable = _lib.volume_table([(h, w, o, o) for (_, _, (_, h, w)), o in zip(volumes, offs)])
    data = torch.frombuffer(bytearray(b''.join(blobs)), dtype=torch.uint8).to(cuda)
    sym = torch.full((total,), SYM_GUARD, dtype=torch.int64, device=cuda) if want_syms else None
    q = torch.full((total,), Q_GUARD, dtype=torch.float32, device=cuda) if want_q else None
    status = torch.full((len(tiles) + slack,), SYM_GUARD, dtype=torch.int32, device=cuda)
    nl = G if nlayers is None else nlayers
    shape_args = (C, max(t[2] for t in tiles), max(t[3] for t in tiles), len(tiles), len(volumes), 24, min(max(nl, 1), 16))
    per = limits is not None
    name = 'ic_pc_decode_tiles_batch_fronts_pertile' if per else 'ic_pc_decode_tiles_batch_fronts'
    need = int(getattr(_lib.lib, name + '_workspace_bytes')(*shape_args))
    assert need == int(getattr(_lib.lib, name.replace('fronts', 'layers') + '_workspace_bytes')(*shape_args)) > 0
    ws = torch.full((need + slack,), GUARD, dtype=torch.uint8, device=cuda)
    centers = pred.centers.contiguous().float()
    host_ends = (ctypes.c_int * max(G, 1))(*ends)
    host_limits = (ctypes.c_int * len(tiles))(*limits) if per else None
    rc = getattr(_lib.lib, name + '_f32')(
        _lib.ptr(data), pos, table, len(tiles), vtable, len(volumes), pred.pc._tab, _lib.ptr(centers), pred.pc._k, pred.pc.L,
        pred.freqs_resolution, _lib.ptr(sym), _lib.ptr(q), _lib.ptr(status), C, _lib.ptr(ws), need - ws_short, int(flags),
        _lib.current_stream(cuda), host_limits if per else int(K), int(fill), host_ends, nl, seg_table)
    torch.cuda.synchronize()
    assert bool((ws[need:] == GUARD).all()), 'workspace: written behind its stated size'
    assert bool((status[len(tiles):] == SYM_GUARD).all()), 'status: written behind the table'
    keep = torch.ones(total, dtype=torch.bool, device=cuda)
    for (_, _, (c, h, w)), o in zip(volumes, offs):
        keep[o:o + c * h * w] = False
    for buf, guard, what in ((sym, SYM_GUARD, 'symbols'), (q, Q_GUARD, 'q')):
        if buf is not None:
            assert bool((buf[keep] == guard).all()), '{}: written outside the volumes'.format(what)
            if rc != 0:
                assert bool((buf == guard).all()), 'a refused call wrote {}'.format(what)
            else:
                assert not bool((buf[~keep] == guard).any()), '{}: a cell of a listed tile was not written'.format(what)
    if rc != 0:
        assert bool((status == SYM_GUARD).all()) and bool((ws == GUARD).all()), 'a refused call wrote something'
        return rc, None, None, None
    cut = lambda buf: [buf[o:o + c * h * w].view(c, h, w) for (_, _, (c, h, w)), o in zip(volumes, offs)]
    if want_syms and want_q:
        for s, qq in zip(cut(sym), cut(q)):
            assert torch.equal(qq, centers[s]), 'q is not centers[symbols]'
    return (rc, [s.cpu().numpy() for s in cut(sym)] if want_syms else None, cut(q) if want_q else None, status[:len(tiles)].tolist())


def _check_all_k(cuda, pred, vols, syms, th, tw, ends, what, fives=None):
    """the whole decode, then every K in 1 .. C: the preview rule on what was coded, the channels=K decode of the format-5 streams of
    the same symbols, and the same with the segments that K does not reach given as {0, 0} and as other bytes"""
    from imgcomp_cvpr_amd import codec
    fill, C = pred.conceal_fallback(), syms[0].shape[0]
    centers = pred.centers.contiguous().float()
    rc, full, _, status = _raw_fronts(cuda, pred, vols, th, tw, ends, C, fill)
    assert rc == 0 and status == [0] * len(status), (what, rc, status)
    assert all(np.array_equal(a, b) for a, b in zip(full, syms)), '{}: the full decode is not what was coded'.format(what)
    for K in range(1, C + 1):
        wants = [codec.preview_symbols(s, K, fill) for s in syms]
        if fives is not None:
            five = pred.decode_tiles_batch(fives, th, tw, want='symbols', order='wavefront', channels=K)
            assert all(np.array_equal(f.cpu().numpy(), want) for f, want in zip(five, wants)), (what, K)
        for unneeded in ('real', 'zero', 'other'):
            rc, got, q, status = _raw_fronts(cuda, pred, vols, th, tw, ends, K, fill, unneeded=unneeded)
            assert rc == 0 and status == [0] * len(status), (what, K, unneeded, rc, status)
            assert all(np.array_equal(g, want) for g, want in zip(got, wants)), '{} K = {} ({}): not the rule on what was coded'.format(what, K, unneeded)
            assert all(torch.equal(qq, centers[torch.as_tensor(want).to(cuda)]) for qq, want in zip(q, wants))
    return full


@pytest.mark.parametrize('shape', SHAPES)
def test_decoder_fronts_single_tile(cuda, pred, shape):
    C = shape[0]
    sym = np.random.RandomState(10 + sum(shape)).randint(0, pred.pc.L, size=shape).astype(np.int64)
    fives = _coded5(pred, [sym], shape[1], shape[2])
    for ends in _ends_variants(C):
        vols = _coded(pred, [sym], shape[1], shape[2], ends)
        _check_all_k(cuda, pred, vols, [sym], shape[1], shape[2], ends, '{} ends {}'.format(shape, ends), fives)


def test_decoder_fronts_two_volumes_edge_tiles(cuda, pred):
    """(6, 5, 7) cut into 4 x 4 tiles: four tiles of three different extents, every one with its own cuts; beside a second volume"""
    from imgcomp_cvpr_amd import codec
    rs = np.random.RandomState(21)
    syms = [rs.randint(0, pred.pc.L, size=s).astype(np.int64) for s in ((6, 5, 7), (6, 3, 2))]
    assert sorted(set(g[2:] for g in codec.tile_grid(5, 7, 4, 4))) == [(1, 3), (1, 4), (4, 3), (4, 4)]
    assert len(set(tuple(codec.front_layer_cuts(6, a, b, [1, 2, 6])) for _, _, a, b in codec.tile_grid(5, 7, 4, 4))) == 4
    fill = pred.conceal_fallback()
    centers = pred.centers.contiguous().float()
    fives = _coded5(pred, syms, 4, 4)
    for ends in ([6], [1, 2, 6], [1, 2, 3, 4, 5, 6]):
        vols = _coded(pred, syms, 4, 4, ends)
        full = _check_all_k(cuda, pred, vols, syms, 4, 4, ends, 'two volumes, ends {}'.format(ends), fives)
        for K in (2, 6):
            wants = [codec.preview_symbols(f, K, fill) for f in full]
            rc, none, q_only, status = _raw_fronts(cuda, pred, vols, 4, 4, ends, K, fill, want_syms=False)
            assert rc == 0 and none is None and status == [0] * len(status)
            rc, s_only, none, status = _raw_fronts(cuda, pred, vols, 4, 4, ends, K, fill, want_q=False)
            assert rc == 0 and none is None and status == [0] * len(status) and all(np.array_equal(a, b) for a, b in zip(s_only, wants))
            assert all(torch.equal(qq, centers[torch.as_tensor(w).to(cuda)]) for qq, w in zip(q_only, wants))
            # the Python surface; entries of layers that are not needed may be None
            thin = [([[b if (g == 0 or ends[g - 1] < K) else None for g, b in enumerate(segs)] for segs in streams], firsts, shape)
                    for streams, firsts, shape in vols]
            both = pred.decode_tiles_batch(thin, 4, 4, want='both', channels=K, front_ends=ends)
            for (qq, s), want in zip(both, wants):
                assert np.array_equal(s.cpu().numpy(), want) and torch.equal(qq, centers[s])
        assert all(np.array_equal(s.cpu().numpy(), f) for s, f in zip(pred.decode_tiles_batch(vols, 4, 4, want='symbols', front_ends=ends), full))
    with pytest.raises(ValueError, match='conceal'):
        pred.decode_tiles_batch(vols, 4, 4, conceal=True, front_ends=[1, 2, 3, 4, 5, 6])
    with pytest.raises(ValueError, match='need the segments'):
        pred.decode_tiles_batch([([[None] * 6] * 4, vols[0][1], (6, 5, 7))], 4, 4, front_ends=[1, 2, 3, 4, 5, 6])
    with pytest.raises(ValueError, match='front_ends cuts the wavefront order at fronts by itself'):
        pred.decode_tiles_batch(vols, 4, 4, front_ends=[6], order='wavefront')


def _split(limits, volumes, th, tw):
    from imgcomp_cvpr_amd import codec
    out, i = [], 0
    for _, _, (_, h, w) in volumes:
        n = len(codec.tile_grid(h, w, th, tw))
        out.append(limits[i:i + n])
        i += n
    return out


@pytest.mark.parametrize('ends', [[6], [1, 2, 6], [1, 2, 3, 4, 5, 6]], ids=['one layer', '1,2,6', 'a layer per channel'])
def test_decoder_limit_per_tile(cuda, pred, ends):
    C = 6
    rs = np.random.RandomState(31 + len(ends))
    syms = [rs.randint(0, pred.pc.L, size=s).astype(np.int64) for s in ((6, 5, 7), (6, 9, 3))]
    vols = _coded(pred, syms, 4, 4, ends)
    ntiles = sum(len(v[0]) for v in vols)
    fill = pred.conceal_fallback()
    centers = pred.centers.contiguous().float()
    mixed = [int(v) for v in rs.randint(1, C + 1, size=ntiles)]               # random limits, layer ends or not
    for limits in ([C] * ntiles, [1] * ntiles, mixed, mixed[::-1], [[3, 1, 6, 2, 5, 4, 6, 1][i % 8] for i in range(ntiles)]):
        wants = [RR.preview_per_tile(s, k, 4, 4, fill) for s, k in zip(syms, _split(limits, vols, 4, 4))]
        for unneeded in ('real', 'zero', 'other'):
            rc, got, q, status = _raw_fronts(cuda, pred, vols, 4, 4, ends, None, fill, limits=limits, unneeded=unneeded)
            assert rc == 0 and status == [0] * ntiles, (limits, unneeded, rc, status)
            assert all(np.array_equal(g, w) for g, w in zip(got, wants)), 'limits {} ({}): not the per-tile preview of what was coded'.format(limits, unneeded)
            assert all(torch.equal(qq, centers[torch.as_tensor(w).to(cuda)]) for qq, w in zip(q, wants))
        rc, none, q_only, status = _raw_fronts(cuda, pred, vols, 4, 4, ends, None, fill, limits=limits, want_syms=False, unneeded='zero')
        assert rc == 0 and none is None and status == [0] * ntiles
        assert all(torch.equal(qq, centers[torch.as_tensor(w).to(cuda)]) for qq, w in zip(q_only, wants))
        rc, s_only, none, status = _raw_fronts(cuda, pred, vols, 4, 4, ends, None, fill, limits=limits, want_q=False, unneeded='zero')
        assert rc == 0 and none is None and all(np.array_equal(g, w) for g, w in zip(s_only, wants))
    for K in (1, 2, 3, 6):                                                    # one limit for all: the scalar entry, bit for bit
        rc, a, qa, sa = _raw_fronts(cuda, pred, vols, 4, 4, ends, None, fill, limits=[K] * ntiles)
        rc2, b, qb, sb = _raw_fronts(cuda, pred, vols, 4, 4, ends, K, fill)
        assert rc == 0 and rc2 == 0 and sa == sb
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(qa, qb))
    # the Python surface: decode, then the concealment per (tile, channel)
    layers = [[len(ends), 0, 1, len(ends)], [1, len(ends), 0]]
    thin = [([None if g_t == 0 else [b if g < g_t else None for g, b in enumerate(segs)] for segs, g_t in zip(streams, gl)], firsts, shape)
            for (streams, firsts, shape), gl in zip(vols, layers)]
    got, held = pred.decode_tiles_batch(thin, 4, 4, want='both', front_ends=ends, tile_layers=layers)
    have = [[([0] + ends)[g] for g in gl] for gl in layers]
    for (q, s), sym, hv in zip(got, syms, have):
        assert np.array_equal(s.cpu().numpy(), RR.recover(sym, hv, 4, 4, pred.pc.L, fill)) and torch.equal(q, centers[s])
    assert held == [[(t, g, hv[t], None) for t, g in enumerate(gl) if hv[t] < C] for gl, hv in zip(layers, have)]


def test_decoder_refusals_write_nothing(cuda, pred):
    from imgcomp_cvpr_amd import _lib
    sym = np.random.RandomState(2).randint(0, pred.pc.L, size=(6, 5, 7)).astype(np.int64)
    fill, ends = pred.conceal_fallback(), [1, 2, 6]
    vols = _coded(pred, [sym], 4, 4, ends)
    ok = [6, 2, 1, 3]
    for limits in (None, ok):                                                 # the scalar entry, the per-tile entry
        call = lambda e=ends, K=6, f=fill, lim=limits, **kw: _raw_fronts(cuda, pred, vols, 4, 4, e, K, f, limits=lim, **kw)[0]
        assert call() == 0
        for flags in (_lib.PC_DECODE_WAVEFRONT, _lib.PC_DECODE_RECOMPUTE, _lib.PC_DECODE_PER_LAYER):
            assert call(flags=flags) == -2, flags                             # IC_ERR_UNSUPPORTED: the order is the entry's own
        for bad in ([2, 2, 6], [0, 2, 6], [1, 2, 5], [1, 2, 7], [2, 1, 6]):
            assert call(e=bad) == -1, bad                                     # IC_ERR_ARG
        for nl in (0, 17, -1):
            assert call(nlayers=nl) == -1, nl
        assert call(f=pred.pc.L) == -1
        assert call(ws_short=1) == -3                                         # IC_ERR_WORKSPACE
        outside = [lambda total: (total - 1, 2), lambda total: (-1, 1), lambda total: (0, -1), lambda total: (total + 1, 0)]
        for seg in outside:                                                   # a needed segment outside [0, total_bytes); one no limit reaches
            assert call(break_seg=(3 * 0 + 2, seg)) == -1                     # tile 0 reads all layers either way
            assert call(break_seg=(3 * 2 + 0, seg)) == -1                     # layer 0 is always read
            if limits is None:
                assert call(K=2, break_seg=(3 * 1 + 2, seg)) == 0
            else:
                assert call(break_seg=(3 * 3 + 2, seg)) == -1                 # tile 3, limit 3: layer 2 begins at 2
                assert call(break_seg=(3 * 1 + 2, seg)) == 0                  # tile 1, limit 2
                assert call(break_seg=(3 * 2 + 1, seg)) == 0                  # tile 2, limit 1
    for K in (0, 7):
        assert _raw_fronts(cuda, pred, vols, 4, 4, ends, K, fill)[0] == -1
    for t in range(4):
        for bad in (0, 7, -1):
            assert _raw_fronts(cuda, pred, vols, 4, 4, ends, None, fill, limits=ok[:t] + [bad] + ok[t + 1:])[0] == -1, (t, bad)
    wide, _ = _model(cuda, [0, 1, 2, 3, 2, 1], 'res_shallow_64')
    assert wide.pc._k == 64
    wvols = _coded(wide, [sym], 4, 4, ends)                                   # the encoder knows no width
    assert _raw_fronts(cuda, wide, wvols, 4, 4, ends, 6, 0)[0] == -2 and _raw_fronts(cuda, wide, wvols, 4, 4, ends, None, 0, limits=ok)[0] == -2
    with pytest.raises(ValueError, match='k = 24, this one has k = 64'):
        wide.decode_tiles_batch(wvols, 4, 4, front_ends=ends)


# ---- hard coder states on the device ------------------------------------------------------------------------------------------

def _const_front_segments(table, sym_chw, ends):
    """the host coder over one constant table: the tile's symbols in wavefront order, cut at the cuts"""
    from imgcomp_cvpr_amd import codec
    order = codec.wavefront_order(*sym_chw.shape)
    flat = sym_chw.reshape(-1)[order]
    cuts = codec.front_layer_cuts(*(sym_chw.shape + (ends,)))
    return [cc.host_encode(flat[max(1, a):b], [table] * (b - max(1, a)))[0] for a, b in zip([0] + cuts, cuts)]


def test_pending_run_across_a_cut(cuda):
    """a run of pending bits longer than 64, built in the ORDER OF THE STREAM, is open at the first cut (48 symbols into the stream of
    a (4, 4, 6) tile with ends 1, 2, 4; the run covers the stream's positions 1 + lead .. 60 + lead)"""
    from imgcomp_cvpr_amd import codec
    model, table = _model(cuda, [0, 1, 2, 3, 2, 1])
    shape, steps = (4, 4, 6), 60
    order = codec.wavefront_order(*shape)
    assert codec.front_layer_cuts(4, 4, 6, [1, 2, 4]) == [48, 72, 96] and codec.front_layer_cuts(4, 4, 6, [1, 2, 3, 4])[:2] == [48, 72]
    for lead in (0, 3):
        prefix = PENDING_PREFIXES[lead]
        run, reached = cc.straddle_symbols(table, steps, prefix)
        assert reached > 64
        rs = np.random.RandomState(40 + lead)
        stream = np.array([int(rs.randint(6))] + list(prefix) + run + rs.randint(6, size=96 - 1 - lead - steps).tolist(), np.int64)
        sym = np.empty(96, np.int64)
        sym[order] = stream
        sym = sym.reshape(shape)
        for ends in ([1, 2, 4], [1, 2, 3, 4], [4]):
            vols = _coded(model, [sym], 4, 6, ends)
            assert vols[0][0][0] == _const_front_segments(table, sym, ends), 'the device segments are not the host coder\'s'
            _check_all_k(cuda, model, vols, [sym], 4, 6, ends, 'pending run, lead {}, ends {}'.format(lead, ends))


def test_floor_frequency_symbols_across_the_cuts(cuda):
    model, table = _model(cuda, [0, 40, 40, 40, 40, 40])
    assert table[0] == 1
    rs = np.random.RandomState(17)
    sym = rs.randint(0, 6, size=(5, 3, 4)).astype(np.int64)
    sym[:3] = 0                                                               # the frequency-1 symbol on both sides of two cuts
    for ends in ([1, 2, 5], [1, 2, 3, 4, 5]):
        vols = _coded(model, [sym], 3, 4, ends)
        assert vols[0][0][0] == _const_front_segments(table, sym, ends)
        _check_all_k(cuda, model, vols, [sym], 3, 4, ends, 'floor frequency, ends {}'.format(ends))


@pytest.mark.parametrize('bias', GARBAGE_TABLES, ids=['floor L=6', 'exact L=3', 'skewed L=16'])
def test_arbitrary_bytes_as_segments(cuda, bias):
    """bytes that no encoder wrote, every segment a string of its own: the symbols and the status are those of the word-level model
    of the decoder (codec_cases.model_decode, equal to the host decoder) restarted at every front cut, every tile by its own cuts"""
    from imgcomp_cvpr_amd import codec
    model, table = _model(cuda, bias)
    L = len(table)
    rs = np.random.RandomState(80 + L)
    shape, ends = (6, 5, 7), [1, 2, 6]
    valid = model.encode_stream(_draw(rs, table, (6, 4, 4)))[0]
    strings = [d for _, d in cc.garbage_strings(valid, seed=90 + L)]
    grid = codec.tile_grid(5, 7, 4, 4)
    fill = model.conceal_fallback()
    for r in range(0, len(strings), 6):
        streams = [[strings[(r + 3 * t + g) % len(strings)] for g in range(3)] for t in range(4)]
        firsts = [int(v) for v in rs.randint(L, size=4)]
        want = np.full(shape, -1, np.int64)
        for t, (y0, x0, a, b) in enumerate(grid):
            order, cuts = codec.wavefront_order(6, a, b), codec.front_layer_cuts(6, a, b, ends)
            flat = np.full(6 * a * b, -1, np.int64)
            flat[0] = firsts[t]
            for g, (lo, hi) in enumerate(zip([0] + cuts, cuts)):
                lo = max(1, lo)
                got, status = cc.model_decode(streams[t][g], [table] * (hi - lo))
                assert status == 0 and got == cc.host_decode(streams[t][g], [table] * (hi - lo))
                flat[order[lo:hi]] = got
            want[:, y0:y0 + a, x0:x0 + b] = flat.reshape(6, a, b)
        assert want.min() >= 0 and want.max() < L
        for K in (1, 2, 6):
            rc, got, _, status = _raw_fronts(cuda, model, [(streams, firsts, shape)], 4, 4, ends, K, fill, unneeded='zero')
            assert rc == 0 and status == [0] * 4, (r, K, status)
            assert np.array_equal(got[0], codec.preview_symbols(want, K, fill)), 'strings {}.., K = {}'.format(r, K)
        limits = [3, 1, 6, 2]
        rc, got, _, status = _raw_fronts(cuda, model, [(streams, firsts, shape)], 4, 4, ends, None, fill, limits=limits, unneeded='other')
        assert rc == 0 and status == [0] * 4 and np.array_equal(got[0], RR.preview_per_tile(want, limits, 4, 4, fill)), r


def test_total_over_the_limit_with_cuts(cuda):
    """one over the coder's limit at every position: the status of a tile is 1 as soon as one coded symbol lies inside what is stepped
    through -- in the middle segment as in any other -- and stays 1 over the cuts behind it; a prefix that is the uncoded first symbol
    alone has consulted no table: status 0.  As with the raster cuts, a model's table is one row at every position, so every segment
    that codes a symbol fails and the one clean segment is the empty segment 0: the fold of an early error over a clean LAST segment
    cannot be shown with these tables (a sweep that opens a segment decodes at least one symbol from it)."""
    from imgcomp_cvpr_amd import arithmetic_coding as ac
    model, table = _model(cuda, [40, 0, 0, 0], resolution=2.0 ** 30)
    assert sum(table) == ac.MAX_TOTAL + 1
    data = np.random.RandomState(9).randint(0, 256, size=40).astype(np.uint8).tobytes()
    fill = model.conceal_fallback()
    vol = ([[data[:9], data[9:20], data[20:]]], [2], (3, 1, 2))
    for K in (1, 2, 3):
        rc, syms, _, status = _raw_fronts(cuda, model, [vol], 1, 2, [1, 2, 3], K, fill)
        assert rc == 0 and status == [1] and syms[0].min() >= 0 and syms[0].max() < 4 and syms[0][0, 0, 0] == 2
    one = ([[b'\x80', data[9:20], data[20:]]], [2], (3, 1, 1))                # segment 0 empty and clean, the middle segment fails
    for K, want in ((1, 0), (2, 1), (3, 1)):
        rc, syms, _, status = _raw_fronts(cuda, model, [one], 1, 1, [1, 2, 3], K, fill, unneeded='zero')
        assert rc == 0 and status == [want] and syms[0][0, 0, 0] == 2 and (syms[0].reshape(-1)[K:] == fill).all()
    two = ([[data[:9], data[9:20]], [data[20:30], data[30:]]], [2, 3], (2, 1, 2))      # two 1 x 1 tiles, a limit each
    for limits, want in (([1, 1], [0, 0]), ([1, 2], [0, 1]), ([2, 1], [1, 0]), ([2, 2], [1, 1])):
        rc, syms, _, status = _raw_fronts(cuda, model, [two], 1, 1, [1, 2], None, fill, limits=limits, unneeded='zero')
        assert rc == 0 and status == want, (limits, status)


# ---- files ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def cdc(cuda, configs, syn_weights):
    from imgcomp_cvpr_amd import codec
    return codec.Codec(configs[0], configs[1], syn_weights, cuda)


def _write(c, version, img, tile=(4, 4), many=False, ends='default'):
    c.tile = tile
    c.order = 'wavefront' if version == 5 else 'raster'
    c.layers = ends if version == 6 else None
    c.front_layers = ends if version == 8 else None
    try:
        return c.compress_many(img) if many else c.compress(img)
    finally:
        c.tile, c.order, c.checked, c.layers, c.front_layers = None, 'raster', False, None, None


ENDS32 = [4, 8, 16, 32]
IMAGES = [((40, 56), (4, 4)), ((200, 312), (8, 8)), ((8, 8), (4, 4))]


@pytest.mark.parametrize('size,tile', IMAGES, ids=['40x56', '200x312 tile 8', '8x8'])
def test_file_equals_formats_5_and_6(cdc, size, tile):
    from imgcomp_cvpr_amd import codec
    img = _image(*size)
    data, five, six = (_write(cdc, v, img, tile) for v in (8, 5, 6))
    head, head5, head6 = (codec.parse_container(d) for d in (data, five, six))
    assert head.version == 8 and head.layer_ends == ENDS32 and head.first_syms == head5.first_syms == head6.first_syms
    assert (head.h, head.w) == ((size[0] + 7) // 8, (size[1] + 7) // 8) and len(data) - len(six) == len(head.payload) - len(head6.payload)
    full = cdc.decode_symbols(data)[0]
    assert np.array_equal(full, cdc.decode_symbols(five)[0]) and np.array_equal(full, cdc.decode_symbols(six)[0])
    pixels = cdc.decompress(data)
    assert np.array_equal(pixels, cdc.decompress(five)) and np.array_equal(pixels, cdc.decompress(six))
    for K in ENDS32 + [5]:                                                    # (5 is no layer end)
        a = cdc.decode_symbols(data, channels=K)[0]
        assert np.array_equal(a, codec.preview_symbols(full, K, cdc.pred.conceal_fallback())) and np.array_equal(a, cdc.decode_symbols(five, channels=K)[0])
    # every prefix of the file is the preview of its layers
    for g in range(1, 5):
        n = codec.layer_prefix_bytes(data, g)
        out, report = cdc.decompress_partial(data[:n])
        assert report == codec.PartialReport(4, g, ENDS32[g - 1], False), (g, report)
        assert np.array_equal(out, cdc.decompress(data, channels=ENDS32[g - 1])), g
        if g > 1:
            out, report = cdc.decompress_partial(data[:n - 1])                # one byte less: the layer before
            assert report.layers_decoded == g - 1 and np.array_equal(out, cdc.decompress(data, channels=ENDS32[g - 2]))
        else:
            with pytest.raises(ValueError, match='no complete layer'):
                cdc.decompress_partial(data[:n - 1])
    out, report = cdc.decompress_partial(data)
    assert report == codec.PartialReport(4, 4, 32, True) and np.array_equal(out, pixels)
    ok, text = codec.verify_file(data)
    assert ok and 'format 8' in text and 'G = 4' in text
    flipped = bytearray(data)
    flipped[codec.layer_prefix_bytes(data, 0) + 3] ^= 0x04
    assert not codec.verify_file(bytes(flipped))[0]
    with pytest.raises(ValueError, match='CRC'):
        cdc.decompress(bytes(flipped))
    with pytest.raises(ValueError, match='out of scope'):
        cdc.salvage(data)
    with pytest.raises(ValueError, match=r'is not streamed.*--recover'):
        cdc.open_stream().feed(data)


def test_file_one_layer_is_format_5(cdc):
    from imgcomp_cvpr_amd import codec
    img = _image(40, 56)
    head, head5 = codec.parse_container(_write(cdc, 8, img, ends=[32])), codec.parse_container(_write(cdc, 5, img))
    assert [s[0] for s in head.streams] == head5.streams                      # G = 1: the format-5 streams, byte for byte
    data = _write(cdc, 8, img, ends=[1, 2, 32])
    assert codec.parse_container(data).layer_ends == [1, 2, 32] and np.array_equal(cdc.decompress(data), cdc.decompress(_write(cdc, 5, img)))


def _seg_start(data, c, g, t):
    from imgcomp_cvpr_amd import codec
    return codec.layer_prefix_bytes(data, g) + sum(len(b) for b in c.segments[g][:t])


def _flip(data, c, g, t):
    bad = bytearray(data)
    bad[_seg_start(data, c, g, t) + len(c.segments[g][t]) // 2] ^= 0x20
    return bytes(bad)


def test_file_recover(cdc):
    from imgcomp_cvpr_amd import codec
    data = _write(cdc, 8, _image(40, 56, seed=3))
    c = codec.parse_container(data)
    full = cdc.decode_symbols(data)[0]
    fill, L, grid = cdc.pred.conceal_fallback(), cdc.L, codec.tile_grid(5, 7, 4, 4)
    img, report = cdc.recover(data)
    assert np.array_equal(img, cdc.decompress(data)) and report == codec.RecoverReport(4, 4, True, [])

    def check(damaged, have, reasons):
        sym, head, report = cdc.recover_symbols(damaged)
        want = RR.recover(full, have, 4, 4, L, fill)
        assert head.version == 8 and np.array_equal(sym, want)
        img, report2 = cdc.recover(damaged)
        assert report2 == report and np.array_equal(img, cdc._image(want, c))
        assert [(d.index, d.channels, d.reason, d.latent) for d in report.tiles] == [(t, have[t], reasons[t], grid[t]) for t in sorted(reasons)]
        assert [d.layers for d in report.tiles] == [([0] + ENDS32).index(have[t]) for t in sorted(reasons)]
        assert (report.ntiles, report.layers_total, report.file_crc_ok) == (4, 4, False)
    assert len(c.segments[2][2]) > 1
    check(data[:_seg_start(data, c, 2, 2) + 1], [16, 16, 8, 8], {t: 'truncated' for t in range(4)})        # cut inside layer 2, one byte into tile 2's segment
    check(data[:_seg_start(data, c, 3, 2)], [32, 32, 16, 16], {2: 'truncated', 3: 'truncated'})
    check(_flip(data, c, 1, 2), [32, 32, 4, 32], {2: 'crc'})                  # layers 2 and 3 of tile 2 are intact, and lost
    check(_flip(data, c, 0, 0), [0, 32, 32, 32], {0: 'crc'})
    check(_flip(_flip(data, c, 3, 1), c, 2, 3)[:-2], [32, 16, 32, 8], {1: 'crc', 3: 'crc'})
    for g in range(1, 5):                                                     # a file cut at a layer end: --partial's image
        cut = data[:codec.layer_prefix_bytes(data, g)]
        assert np.array_equal(cdc.recover(cut)[0], cdc.decompress_partial(cut)[0]), g
    with pytest.raises(ValueError, match='header damaged'):
        cdc.recover(data[:codec.layer_prefix_bytes(data, 0) - 1])


def test_many_equals_single(cdc):
    from imgcomp_cvpr_amd import codec
    imgs = [_image(40, 56, seed=3), _image(8, 8, seed=4), _image(64, 96, seed=5)]
    eights = [_write(cdc, 8, im) for im in imgs]
    assert _write(cdc, 8, imgs, many=True) == eights                         # compress_many: the same bytes, file by file
    datas = eights + [_write(cdc, 6, im) for im in imgs] + [_write(cdc, 5, im) for im in imgs] + [_write(cdc, 8, imgs[0], ends=[2, 32])]
    for K in (None, 8):
        singles = [cdc.decompress(d, channels=K) for d in datas]
        many = cdc.decompress_many(datas, channels=K)
        assert len(many) == len(singles) and all(np.array_equal(a, b) for a, b in zip(many, singles)), K
    c8, c6 = codec.parse_container(datas[0]), codec.parse_container(datas[3])
    damaged = [datas[0], datas[0][:_seg_start(datas[0], c8, 2, 2)], _flip(datas[0], c8, 1, 2), datas[3][:_seg_start(datas[3], c6, 2, 2)],
               _flip(datas[3], c6, 1, 2), datas[2][:codec.layer_prefix_bytes(datas[2], 1) + 3], datas[9], datas[5]]
    singles = [cdc.recover(d) for d in damaged]
    many = cdc.recover_many(damaged)
    assert len(many) == len(singles)
    for i, ((a, ra), (b, rb)) in enumerate(zip(many, singles)):
        assert np.array_equal(a, b) and ra == rb, i
    assert [len(r.tiles) for _, r in singles] == [0, 4, 1, 4, 1, 6, 0, 0]
    with pytest.raises(ValueError, match='file 1: .*--salvage'):
        cdc.recover_many([datas[0], datas[6]])                                # a format-5 file is not recovered


def test_options_and_cli(cdc, cuda, configs, syn_weights, tmp_path, capsys):
    from PIL import Image
    from imgcomp_cvpr_amd import codec, config_parser as cp, weights as W
    for kw, why in ((dict(front_layers='default'), 'needs a tile extent'), (dict(tile=(4, 4), front_layers=[4, 31]), 'not C = 32'),
                    (dict(tile=(4, 4), front_layers='default', order='wavefront'), "does not go with order='wavefront'"),
                    (dict(tile=(4, 4), front_layers='default', layers='default'), 'does not go with layers'),
                    (dict(tile=(4, 4), front_layers='other'), "'default'")):
        with pytest.raises(ValueError, match=why):
            codec.Codec(configs[0], configs[1], syn_weights, cuda, **kw)
    pc64, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow_64'))
    w64 = W.synthetic_weights(configs[0], pc64)
    with pytest.raises(ValueError, match='k = 24, this one has k = 64'):
        codec.Codec(configs[0], pc64, w64, cuda, tile=(4, 4), front_layers='default')
    img = _image(40, 56, seed=6)
    src = str(tmp_path / 'in.png')
    Image.fromarray(img).save(src)
    icf, png = str(tmp_path / 'a.icf'), str(tmp_path / 'a.png')
    assert codec.main(['compress', src, icf, '--tile', '32', '--front-progressive', '--device', str(cuda)]) == 0
    capsys.readouterr()
    data = open(icf, 'rb').read()
    assert data == _write(cdc, 8, img)
    assert codec.main(['compress', src, icf, '--tile', '32', '--front-layers', '2,32', '--device', str(cuda)]) == 0
    capsys.readouterr()
    assert open(icf, 'rb').read() == _write(cdc, 8, img, ends=[2, 32])
    cut = str(tmp_path / 'cut.icf')
    with open(cut, 'wb') as f:
        f.write(data[:codec.layer_prefix_bytes(data, 2) + 5])
    assert codec.main(['decompress', cut, png, '--partial', '--device', str(cuda)]) == 0
    assert 'layers decoded 2 of 4' in capsys.readouterr().out
    assert np.array_equal(np.asarray(Image.open(png)), cdc.decompress(data, channels=8))
    assert codec.main(['decompress', cut, png, '--recover', '--device', str(cuda)]) == 0
    assert 'tiles incomplete' in capsys.readouterr().out
    assert np.array_equal(np.asarray(Image.open(png)), cdc.recover(data[:codec.layer_prefix_bytes(data, 2) + 5])[0])
    assert codec.main(['decompress', cut, png, '--device', str(cuda)]) == 2                    # the strict reader refuses the cut file
    assert 'CRC' in capsys.readouterr().err
    whole = str(tmp_path / 'whole.icf')
    with open(whole, 'wb') as f:
        f.write(data)
    assert codec.main(['decompress', whole, png, '--channels', '4', '--device', str(cuda)]) == 0
    capsys.readouterr()
    assert np.array_equal(np.asarray(Image.open(png)), cdc.decompress(data, channels=4))
    assert codec.main(['stream', whole, str(tmp_path / 'frames'), '--device', str(cuda)]) == 2
    assert '--recover' in capsys.readouterr().err
    assert codec.main(['verify', cut]) == 1 and '2 of 4 layers complete' in capsys.readouterr().out
    src_dir, out_dir, back = tmp_path / 'pngs', tmp_path / 'icfs', tmp_path / 'back'
    src_dir.mkdir()
    Image.fromarray(img).save(str(src_dir / 'a.png'))
    Image.fromarray(_image(8, 8, seed=4)).save(str(src_dir / 'b.png'))
    assert codec.main(['compress-dir', str(src_dir), str(out_dir), '--tile', '32', '--front-progressive', '--device', str(cuda)]) == 0
    assert open(str(out_dir / 'a.icf'), 'rb').read() == data
    assert codec.main(['decompress-dir', str(out_dir), str(back), '--device', str(cuda)]) == 0
    capsys.readouterr()
    assert np.array_equal(np.asarray(Image.open(str(back / 'a.png'))), cdc.decompress(data))
