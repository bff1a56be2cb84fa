"""-m gpu: recovery of layered files (container format 6) -- the layered tile decoder with a channel limit per tile
(ic_pc_decode_tiles_batch_layers_pertile_f32) against the per-tile preview rule on the full decode and against its scalar sibling, the
concealment per (tile, channel) (ic_pc_conceal_tiles_channels) against the NumPy statement of its rule (tests/recover_rule.py), then
whole files, cut and damaged.  Every comparison is an equality."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import conceal_rule as R
from tests import recover_rule as RR
from tests.test_gpu_codec_decoder import _load, _model
from tests.test_gpu_codec_layered import GUARD, Q_GUARD, SYM_GUARD, _coded, _image, _raw_layers, _write

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pred(cuda, configs, syn_weights):
    return _load(cuda, configs[0], configs[1], syn_weights, 1e9)


@pytest.fixture(scope='module')
def cdc(cuda, configs, syn_weights):
    from imgcomp_cvpr_amd import codec
    return codec.Codec(configs[0], configs[1], syn_weights, cuda)


# ---- the decoder through the ABI ----------------------------------------------------------------------------------------------

def _raw_pertile(cuda, pred, volumes, th, tw, ends, limits, fill, want_syms=True, want_q=True, flags=0, above='real', nlayers=None,
                 ws_short=0, break_seg=None, slack=4096):
    """ic_pc_decode_tiles_batch_layers_pertile_f32 through the ABI, as _raw_layers calls its sibling.  limits: one per tile, all volumes
    in order.  above: what stands for a tile's segments of layers that begin at or above ITS limit -- 'real' (their bytes), 'zero'
    ({0, 0}), 'other' (other bytes at another place).  symbols, q, status and the workspace carry guard values.
    -> (return code, [symbols per volume] or None, [q per volume, device] or None, status list)"""
    from imgcomp_cvpr_amd import _lib, codec
    G = len(ends)
    junk = bytes(np.random.RandomState(98).randint(0, 256, size=41).astype(np.uint8))
    tiles, segs, blobs, pos, offs, total = [], [], [junk], len(junk), [], slack
    for n, (streams, firsts, (C, h, w)) in enumerate(volumes):
        for t, (y0, x0, a, b) in enumerate(codec.tile_grid(h, w, th, tw)):
            K = limits[len(tiles)]
            tiles.append((y0, x0, a, b, -5, 1 << 40, firsts[t], n))
            for g in range(len(streams[t])):
                needed = g == 0 or (g - 1 < len(ends) and ends[g - 1] < K)
                if needed or above == 'real':
                    segs.append((pos, len(streams[t][g])))
                    blobs.append(bytes(streams[t][g]))
                    pos += len(streams[t][g])
                else:
                    segs.append((0, 0) if above == 'zero' else (5, len(junk) - 5))
        offs.append(total)
        total += C * h * w + slack
    assert len(limits) == len(tiles)
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
    need = int(_lib.lib.ic_pc_decode_tiles_batch_layers_pertile_workspace_bytes(*shape_args))
    assert need > int(_lib.lib.ic_pc_decode_tiles_batch_layers_workspace_bytes(*shape_args))
    ws = torch.full((need + slack,), GUARD, dtype=torch.uint8, device=cuda)
    centers = pred.centers.contiguous().float()
    host_ends, host_limits = (ctypes.c_int * max(G, 1))(*ends), (ctypes.c_int * len(limits))(*limits)
    rc = _lib.lib.ic_pc_decode_tiles_batch_layers_pertile_f32(
        _lib.ptr(data), pos, table, len(tiles), vtable, len(volumes), pred.pc._tab, _lib.ptr(centers), pred.pc._k, pred.pc.L,
        pred.freqs_resolution, _lib.ptr(sym), _lib.ptr(q), _lib.ptr(status), C, _lib.ptr(ws), need - ws_short, int(flags),
        _lib.current_stream(cuda), host_limits, int(fill), host_ends, nl, seg_table)
    torch.cuda.synchronize()
    assert bool((ws[need:] == GUARD).all()), 'workspace: written behind its stated size'
    assert bool((status[len(tiles):] == SYM_GUARD).all()), 'status: written behind the table'
    keep = torch.ones(total, dtype=torch.bool, device=cuda)
    for (_, _, (c, h, w)), o in zip(volumes, offs):
        keep[o:o + c * h * w] = False
    for buf, guard, name in ((sym, SYM_GUARD, 'symbols'), (q, Q_GUARD, 'q')):
        if buf is not None:
            assert bool((buf[keep] == guard).all()), '{}: written outside the volumes'.format(name)
            if rc != 0:
                assert bool((buf == guard).all()), 'a refused call wrote {}'.format(name)
            else:
                assert not bool((buf[~keep] == guard).any()), '{}: a cell of a listed tile was not written'.format(name)
    if rc != 0:
        assert bool((status == SYM_GUARD).all()) and bool((ws == GUARD).all()), 'a refused call wrote something'
        return rc, None, None, None
    cut = lambda buf: [buf[o:o + c * h * w].view(c, h, w) for (_, _, (c, h, w)), o in zip(volumes, offs)]
    if want_syms and want_q:
        for s, qq in zip(cut(sym), cut(q)):
            assert torch.equal(qq, centers[s]), 'q is not centers[symbols]'
    return (rc, [s.cpu().numpy() for s in cut(sym)] if want_syms else None, cut(q) if want_q else None, status[:len(tiles)].tolist())


def _split(limits, volumes, th, tw):
    """the flat list of limits -> one list per volume"""
    from imgcomp_cvpr_amd import codec
    out, i = [], 0
    for _, _, (_, h, w) in volumes:
        n = len(codec.tile_grid(h, w, th, tw))
        out.append(limits[i:i + n])
        i += n
    return out


VOLUME_SETS = [[(6, 5, 7)], [(6, 4, 4), (6, 9, 3)]]
ENDS = [[6], [1, 2, 6], [1, 2, 3, 4, 5, 6]]


@pytest.mark.parametrize('shapes', VOLUME_SETS, ids=['one volume', 'two volumes'])
@pytest.mark.parametrize('ends', ENDS, ids=['one layer', '1,2,6', 'a layer per channel'])
def test_decoder_limit_per_tile(cuda, pred, shapes, ends):
    C = 6
    rs = np.random.RandomState(31 + len(shapes) + len(ends))
    syms = [rs.randint(0, pred.pc.L, size=s).astype(np.int64) for s in shapes]
    vols = _coded(pred, syms, 4, 4, ends)
    ntiles = sum(len(v[0]) for v in vols)
    fill = pred.conceal_fallback()
    centers = pred.centers.contiguous().float()
    mixed = [[3, 1, 6, 2, 5, 4, 6, 1][i % 8] for i in range(ntiles)]         # 3, 4, 5 are no layer ends of [1, 2, 6]
    for limits in ([C] * ntiles, [1] * ntiles, mixed, mixed[::-1]):
        wants = [RR.preview_per_tile(s, k, 4, 4, fill) for s, k in zip(syms, _split(limits, vols, 4, 4))]
        for above in ('real', 'zero', 'other'):
            rc, got, q, status = _raw_pertile(cuda, pred, vols, 4, 4, ends, limits, fill, above=above)
            assert rc == 0 and status == [0] * ntiles, (limits, above, rc, status)
            assert all(np.array_equal(g, w) for g, w in zip(got, wants)), 'limits {} ({}): not the per-tile preview of what was coded'.format(limits, above)
            assert all(torch.equal(qq, centers[torch.as_tensor(w).to(cuda)]) for qq, w in zip(q, wants))
        rc, none, q_only, status = _raw_pertile(cuda, pred, vols, 4, 4, ends, limits, fill, want_syms=False, above='zero')
        assert rc == 0 and none is None and status == [0] * ntiles
        assert all(torch.equal(qq, centers[torch.as_tensor(w).to(cuda)]) for qq, w in zip(q_only, wants))
        rc, s_only, none, status = _raw_pertile(cuda, pred, vols, 4, 4, ends, limits, fill, want_q=False, above='zero')
        assert rc == 0 and none is None and all(np.array_equal(g, w) for g, w in zip(s_only, wants))
    for K in (1, 2, 3, 6):                                                    # one limit for all: the scalar entry, bit for bit
        rc, a, qa, sa = _raw_pertile(cuda, pred, vols, 4, 4, ends, [K] * ntiles, fill)
        rc2, b, qb, sb = _raw_layers(cuda, pred, vols, 4, 4, ends, K, fill)
        assert rc == 0 and rc2 == 0 and sa == sb
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(qa, qb))


def test_decoder_surface_tile_layers(cuda, pred):
    """PredictionNetwork.decode_tiles_batch(tile_layers=...): decode, then the concealment per channel"""
    from imgcomp_cvpr_amd import _lib
    rs = np.random.RandomState(77)
    syms = [rs.randint(0, 3, size=s).astype(np.int64) for s in VOLUME_SETS[1]]       # three symbols: the votes have majorities
    ends, fill, L = [1, 2, 6], pred.conceal_fallback(), pred.pc.L
    vols = _coded(pred, syms, 4, 4, ends)
    layers = [[3], [2, 0, 3]]
    thin = [([None if g_t == 0 else [b if g < g_t else None for g, b in enumerate(segs)] for segs, g_t in zip(streams, gl)], firsts, shape)
            for (streams, firsts, shape), gl in zip(vols, layers)]
    both, held = pred.decode_tiles_batch(thin, 4, 4, want='both', layer_ends=ends, tile_layers=layers)
    assert held == [[], [(0, 2, 2, None), (1, 0, 0, None)]]
    have = [[6], [2, 0, 6]]
    centers = pred.centers.contiguous().float()
    for (q, s), sym, hv in zip(both, syms, have):
        assert np.array_equal(s.cpu().numpy(), RR.recover(sym, hv, 4, 4, L, fill)) and torch.equal(q, centers[s])
    whole, held = pred.decode_tiles_batch(vols, 4, 4, want='symbols', layer_ends=ends, tile_layers=[[3], [3, 3, 3]])
    assert held == [[], []] and all(np.array_equal(s.cpu().numpy(), sym) for s, sym in zip(whole, syms))
    none, held = pred.decode_tiles_batch(thin, 4, 4, want='symbols', layer_ends=ends, tile_layers=[[0], [0, 0, 0]])
    assert all(bool((s == fill).all()) for s in none) and held == [[(0, 0, 0, None)], [(t, 0, 0, None) for t in range(3)]]
    one_tile = int(_lib.lib.ic_pc_decode_tiles_batch_layers_pertile_workspace_bytes(6, 4, 4, 1, 2, pred.pc._k, 3))
    chunked, _ = pred.decode_tiles_batch(thin, 4, 4, want='symbols', layer_ends=ends, tile_layers=layers, max_workspace_bytes=one_tile * 3 // 2)
    assert all(np.array_equal(a.cpu().numpy(), b[1].cpu().numpy()) for a, b in zip(chunked, both))
    for given, kw, why in ((thin, dict(tile_layers=layers), 'needs layer_ends'), (thin, dict(tile_layers=layers, layer_ends=ends, conceal=True), 'conceal'),
                           (thin, dict(tile_layers=layers, layer_ends=ends, channels=2), 'does not go with'),
                           (vols, dict(tile_layers=[[3], [3, 3]], layer_ends=ends), 'entries for a grid of 3'),
                           (vols, dict(tile_layers=[[3], [3, 4, 3]], layer_ends=ends), 'layers to read of 3'),
                           (thin, dict(tile_layers=[[3], [3, 3, 3]], layer_ends=ends), 'need the segments')):
        with pytest.raises(ValueError, match=why):
            pred.decode_tiles_batch(given, 4, 4, **kw)


def test_decoder_status_per_tile(cuda):
    """one over the coder's limit at every position (the model of the layered status test): a tile's status is 1 as soon as its own
    limit reaches a coded symbol, and 0 where the tile stops at the uncoded first symbol"""
    from imgcomp_cvpr_amd import arithmetic_coding as ac
    model, table = _model(cuda, [40, 0, 0, 0], resolution=2.0 ** 30)
    assert sum(table) == ac.MAX_TOTAL + 1
    data = np.random.RandomState(9).randint(0, 256, size=40).astype(np.uint8).tobytes()
    fill = model.conceal_fallback()
    vol = ([[data[:9], data[9:20], data[20:]]], [2], (3, 1, 2))               # the case of the layered status test
    for K in (1, 2, 3):
        rc, syms, _, status = _raw_pertile(cuda, model, [vol], 1, 2, [1, 2, 3], [K], fill)
        assert rc == 0 and status == [1] and syms[0].min() >= 0 and syms[0].max() < 4 and syms[0][0, 0, 0] == 2
    two = ([[data[:9], data[9:20]], [data[20:30], data[30:]]], [2, 3], (2, 1, 2))      # two 1 x 1 tiles: channel 0 is the first symbol alone
    for limits, want in (([1, 1], [0, 0]), ([1, 2], [0, 1]), ([2, 1], [1, 0]), ([2, 2], [1, 1])):
        rc, syms, _, status = _raw_pertile(cuda, model, [two], 1, 1, [1, 2], limits, fill, above='zero')
        assert rc == 0 and status == want, (limits, status)
        assert syms[0][0, 0].tolist() == [2, 3] and [syms[0][1, 0, t] == fill for t in range(2) if limits[t] == 1] == [True] * limits.count(1)


def test_decoder_refusals_write_nothing(cuda, pred):
    from imgcomp_cvpr_amd import _lib
    sym = np.random.RandomState(2).randint(0, pred.pc.L, size=(6, 5, 7)).astype(np.int64)
    fill, ends = pred.conceal_fallback(), [1, 2, 6]
    vols = _coded(pred, [sym], 4, 4, ends)
    ok = [6, 2, 1, 3]
    assert _raw_pertile(cuda, pred, vols, 4, 4, ends, ok, fill)[0] == 0
    for t in range(4):
        for bad in (0, 7, -1):
            assert _raw_pertile(cuda, pred, vols, 4, 4, ends, ok[:t] + [bad] + ok[t + 1:], fill)[0] == -1, (t, bad)      # IC_ERR_ARG
    assert _raw_pertile(cuda, pred, vols, 4, 4, ends, ok, pred.pc.L)[0] == -1
    # a segment outside [0, total_bytes): refused where the tile's own limit reaches its layer, not looked at where it does not
    outside = [lambda total: (total - 1, 2), lambda total: (-1, 1), lambda total: (0, -1), lambda total: (total + 1, 0)]
    for seg in outside:
        assert _raw_pertile(cuda, pred, vols, 4, 4, ends, ok, fill, break_seg=(3 * 0 + 2, seg))[0] == -1      # tile 0 reads all layers
        assert _raw_pertile(cuda, pred, vols, 4, 4, ends, ok, fill, break_seg=(3 * 3 + 2, seg))[0] == -1      # tile 3, limit 3: layer 2 begins at 2
        assert _raw_pertile(cuda, pred, vols, 4, 4, ends, ok, fill, break_seg=(3 * 2 + 0, seg))[0] == -1      # layer 0 is always read
        assert _raw_pertile(cuda, pred, vols, 4, 4, ends, ok, fill, break_seg=(3 * 1 + 2, seg))[0] == 0       # tile 1, limit 2
        assert _raw_pertile(cuda, pred, vols, 4, 4, ends, ok, fill, break_seg=(3 * 2 + 1, seg))[0] == 0       # tile 2, limit 1
    assert _raw_pertile(cuda, pred, vols, 4, 4, ends, ok, fill, ws_short=1)[0] == -3                           # IC_ERR_WORKSPACE
    for flags in (_lib.PC_DECODE_WAVEFRONT, _lib.PC_DECODE_RECOMPUTE, _lib.PC_DECODE_PER_LAYER):
        assert _raw_pertile(cuda, pred, vols, 4, 4, ends, ok, fill, flags=flags)[0] == -2, flags               # IC_ERR_UNSUPPORTED
    for nl in (0, 17):
        assert _raw_pertile(cuda, pred, vols, 4, 4, ends, ok, fill, nlayers=nl)[0] == -1, nl
        assert _lib.lib.ic_pc_decode_tiles_batch_layers_pertile_workspace_bytes(6, 4, 4, 4, 1, 24, nl) == 0
    for bad in ([2, 2, 6], [1, 2, 5]):
        assert _raw_pertile(cuda, pred, vols, 4, 4, bad, ok, fill)[0] == -1, bad
    wide, _ = _model(cuda, [0, 1, 2, 3, 2, 1], 'res_shallow_64')
    assert _raw_pertile(cuda, wide, _coded(wide, [sym], 4, 4, ends), 4, 4, ends, ok, 0)[0] == -2              # k = 64


# ---- the concealment through the ABI ------------------------------------------------------------------------------------------

def _raw_conceal_channels(cuda, vols, th, tw, L, centers, fallback, with_q=True, gap=384):
    """ic_pc_conceal_tiles_channels through the ABI.  vols: [((C,h,w) int64 numpy, [have per tile])].  The volumes lie `gap` elements
    apart; symbols outside the volumes hold -7, q holds a sentinel everywhere (the kernel is its only writer here), the workspace has
    a guarded tail.  -> (return code, [symbols per volume], [q per volume] or None)"""
    from imgcomp_cvpr_amd import _lib
    shapes, offs, total, tiles, have = [], [], gap, [], []
    for n, (sym, hv) in enumerate(vols):
        C, h, w = sym.shape
        grid = R.grid(h, w, th, tw)
        assert len(hv) == len(grid)
        tiles += [grid[t] + (0, 0, 0, n) for t in range(len(grid)) if hv[t] < C]
        have += [int(v) for v in hv]
        shapes.append((C, h, w))
        offs.append(total)
        total += C * h * w + gap
    host = np.full(total, -7, np.int64)
    for (sym, _), o in zip(vols, offs):
        host[o:o + sym.size] = sym.reshape(-1)
    sym_dev = torch.as_tensor(host).to(cuda)
    q_dev = torch.full((total,), Q_GUARD, dtype=torch.float32, device=cuda) if with_q else None
    table = _lib.tile_table(tiles)
    vtable = _lib.volume_table([(h, w, o, o) for (_, h, w), o in zip(shapes, offs)])
    need = int(_lib.lib.ic_pc_conceal_tiles_channels_workspace_bytes(len(tiles), len(shapes), len(have)))
    ws = torch.full((need + 4096,), GUARD, dtype=torch.uint8, device=cuda)
    cen = torch.as_tensor(np.asarray(centers, np.float32)).to(cuda)
    host_have = (ctypes.c_uint16 * len(have))(*have)
    rc = _lib.lib.ic_pc_conceal_tiles_channels(_lib.ptr(sym_dev), _lib.ptr(q_dev), table, len(tiles), vtable, len(shapes), host_have,
                                               _lib.ptr(cen), L, fallback, shapes[0][0], th, tw, _lib.ptr(ws), need, _lib.current_stream(cuda))
    torch.cuda.synchronize()
    assert bool((ws[need:] == GUARD).all()), 'workspace: written behind its stated size'
    got = sym_dev.cpu().numpy()
    keep = np.ones(total, bool)
    for (c, h, w), o in zip(shapes, offs):
        keep[o:o + c * h * w] = False
    assert (got[keep] == -7).all(), 'symbols: written outside the volumes'
    syms = [got[o:o + c * h * w].reshape(c, h, w) for (c, h, w), o in zip(shapes, offs)]
    if not with_q:
        return rc, syms, None
    qall = q_dev.cpu().numpy()
    assert (qall[keep] == np.float32(Q_GUARD)).all(), 'q: written outside the volumes'
    return rc, syms, [qall[o:o + c * h * w].reshape(c, h, w) for (c, h, w), o in zip(shapes, offs)]


def _missing(shape, have, th, tw):
    """(C, h, w) bool: the cells of the (tile, channel) pairs at or above the tile's `have`"""
    m = np.zeros(shape, bool)
    for (y0, x0, a, b), k in zip(R.grid(shape[1], shape[2], th, tw), have):
        m[k:, y0:y0 + a, x0:x0 + b] = True
    return m


def _check_channels_rule(cuda, vols, th, tw, L, centers, fallback, with_q=True):
    rc, syms, qs = _raw_conceal_channels(cuda, vols, th, tw, L, centers, fallback, with_q)
    assert rc == 0
    cen = np.asarray(centers, np.float32)
    for n, (sym, have) in enumerate(vols):
        want = RR.conceal_channels(sym, have, th, tw, L, fallback)
        assert np.array_equal(syms[n], want), 'volume {}: symbols differ from the rule'.format(n)
        m = _missing(sym.shape, have, th, tw)
        assert np.array_equal(syms[n][~m], sym[~m]), 'volume {}: a channel that its tile holds changed'.format(n)
        if with_q:
            assert np.array_equal(qs[n][m].view(np.uint32), cen[want][m].view(np.uint32)), 'q is not centers[symbols] bit for bit'
            assert (qs[n][~m] == np.float32(Q_GUARD)).all(), 'volume {}: q of a channel that its tile holds was written'.format(n)
    return syms


def _few_symbols(rs, shape, L):
    """few distinct symbols per ring, so that the most frequent one is a real decision and ties happen"""
    sym = rs.randint(0, L, size=shape).astype(np.int64)
    sym[1] = rs.randint(0, 2, size=shape[1:]) * (L - 1)
    sym[2] = 3
    return sym


@pytest.mark.parametrize('shape,th,tw', [((6, 5, 7), 4, 4), ((3, 9, 9), 3, 3)])
def test_conceal_channels_equals_the_rule(cuda, shape, th, tw):
    from tests.test_gpu_codec_checked import _raw_conceal
    L, C = 6, shape[0]
    rs = np.random.RandomState(sum(shape))
    centers = np.sort(rs.uniform(-2, 2, L).astype(np.float32))
    fallback = R.fallback_symbol(centers)
    nt = len(R.grid(shape[1], shape[2], th, tw))
    centre = nt // 2                                                          # (3,9,9)/3x3: tile 4, with four neighbours
    for t in sorted(set([0, centre, nt - 1])):                                # one tile holds nothing, the rest everything: the whole-tile kernel
        sym = _few_symbols(rs, shape, L)
        got = _check_channels_rule(cuda, [(sym, [0 if u == t else C for u in range(nt)])], th, tw, L, centers, fallback)[0]
        old = _raw_conceal(cuda, [(sym, [t])], th, tw, L, centers, fallback)[0][0]
        assert np.array_equal(got, old) and np.array_equal(got, R.conceal(sym, [t], th, tw, L, fallback))
    maps = {'staircase': [t % (C + 1) for t in range(nt)], 'staircase down': [C - t % (C + 1) for t in range(nt)],
            'random': rs.randint(0, C + 1, size=nt).tolist(), 'all nothing': [0] * nt, 'all one': [1] * nt, 'nothing missing but one channel': [C - 1] * nt}
    if nt == 9:                                                               # the centre's neighbours hold 0, 1, 2, 3 channels: some sides only
        maps['partial neighbours'] = [3, 1, 3, 0, 0, 3, 3, 2, 3]
    for name, have in maps.items():
        sym = _few_symbols(rs, shape, L)
        got = _check_channels_rule(cuda, [(sym, have)], th, tw, L, centers, fallback)[0]
        if name == 'all nothing':
            assert (got == fallback).all()
        if name == 'all one':
            assert (got[1:] == fallback).all() and np.array_equal(got[:1], sym[:1])
        # a (tile, channel) that is written is never read: other contents there change nothing
        other = sym.copy()
        m = _missing(shape, have, th, tw)
        other[m] = rs.randint(0, L, size=int(m.sum()))
        assert np.array_equal(_check_channels_rule(cuda, [(other, have)], th, tw, L, centers, fallback, with_q=False)[0], got), name


def test_conceal_channels_tie_two_volumes_and_refusals(cuda):
    from imgcomp_cvpr_amd import _lib
    L = 6
    centers = np.array([-1.5, -0.5, 0.25, 0.75, 1.0, 2.0], np.float32)
    fallback = R.fallback_symbol(centers)
    assert fallback == 2
    # the centre tile of a 3 x 3 grid lacks channels 1 and 2; above: three 5s, below: three 1s, left: lacks channel 1, right: lacks both
    sym = np.zeros((3, 9, 9), np.int64)
    sym[:, 2, 3:6], sym[:, 6, 3:6], sym[:, 3:6, 2], sym[:, 3:6, 6] = 5, 1, 4, 4
    have = [3, 3, 3, 1, 1, 0, 3, 3, 3]
    got = _check_channels_rule(cuda, [(sym, have)], 3, 3, L, centers, fallback)[0]
    assert (got[1, 3:6, 3:6] == 1).all(), 'a 3 : 3 tie must pick the smaller symbol'
    sym[2, 3:6, 2] = 1                                                        # channel 2: the left neighbour still lacks it: 3 : 3 stays
    sym[2, 2, 3] = 1                                                          # ... until one of the 5s turns: 4 : 2
    got = _check_channels_rule(cuda, [(sym, have)], 3, 3, L, centers, fallback)[0]
    assert (got[2, 3:6, 3:6] == 1).all() and (got[1, 3:6, 3:6] == 1).all()
    # two volumes of different shapes in one launch, the second with a ragged grid; -7 never counts (it lies outside every volume)
    rs = np.random.RandomState(8)
    a, b = _few_symbols(rs, (3, 9, 9), L), _few_symbols(rs, (3, 5, 7), L)
    _check_channels_rule(cuda, [(a, [3, 0, 2, 1, 0, 3, 2, 2, 1]), (b, [2, 0, 3, 1, 3, 0])], 3, 3, L, centers, fallback)
    _check_channels_rule(cuda, [(a, [3] * 9), (b, [2, 0, 3, 1, 3, 0])], 3, 3, L, centers, fallback, with_q=False)
    # refusals, decided on the host: nothing is written
    rc, syms, qs = _raw_conceal_channels(cuda, [(a, [4] + [0] * 8)], 3, 3, L, centers, fallback)           # have > C
    assert rc == -1 and np.array_equal(syms[0], a) and (qs[0] == np.float32(Q_GUARD)).all()
    assert _raw_conceal_channels(cuda, [(a, [0] * 9)], 3, 3, L, centers, L)[0] == -1                       # fallback outside [0, L)
    assert _raw_conceal_channels(cuda, [(a, [0] * 9)], 3, 3, 17, np.zeros(17, np.float32), 0)[0] == -2     # L > 16
    vt = _lib.volume_table([(9, 9, 0, 0)])
    hv = (ctypes.c_uint16 * 9)(*([3] * 9))
    dev = torch.as_tensor(a.reshape(-1)).to(cuda)
    cen = torch.as_tensor(centers).to(cuda)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=cuda)
    call = lambda tiles, nbytes=1 << 16: _lib.lib.ic_pc_conceal_tiles_channels(
        _lib.ptr(dev), None, _lib.tile_table(tiles), len(tiles), vt, 1, hv, _lib.ptr(cen), L, fallback, 3, 3, 3, _lib.ptr(ws), nbytes,
        _lib.current_stream(cuda))
    assert call([(0, 0, 3, 3, 0, 0, 0, 0)]) == -1                             # a listed tile that holds all C channels
    hv[0] = 1
    assert call([(0, 0, 3, 3, 0, 0, 0, 0)]) == 0
    assert call([(0, 1, 3, 3, 0, 0, 0, 0)]) == -1 and call([(0, 0, 3, 2, 0, 0, 0, 0)]) == -1               # not a cell of the grid
    assert call([(0, 0, 3, 3, 0, 0, 0, 0)], 16) == -3                         # IC_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert _lib.lib.ic_pc_conceal_tiles_channels_workspace_bytes(0, 1, 9) == 0


# ---- files ----------------------------------------------------------------------------------------------------------------------

ENDS32 = [4, 8, 16, 32]


def _seg_start(data, c, g, t):
    from imgcomp_cvpr_amd import codec
    return codec.layer_prefix_bytes(data, g) + sum(len(b) for b in c.segments[g][:t])


def _flip(data, c, g, t):
    bad = bytearray(data)
    bad[_seg_start(data, c, g, t) + len(c.segments[g][t]) // 2] ^= 0x20
    return bytes(bad)


@pytest.fixture(scope='module')
def six(cdc):
    """a 40 x 56 image as a format-6 file: a (32, 5, 7) volume, four 4 x 4 tiles, layers 4, 8, 16, 32 -> (bytes, container, full symbols)"""
    from imgcomp_cvpr_amd import codec
    data = _write(cdc, 6, _image(40, 56, seed=3))
    c = codec.parse_container(data)
    assert (c.C, c.h, c.w, len(c.streams), c.layer_ends) == (32, 5, 7, 4, ENDS32)
    full = cdc.decode_symbols(data)[0]
    full.setflags(write=False)
    return data, c, full


def test_file_intact_and_prefixes(cdc, six):
    from imgcomp_cvpr_amd import codec
    data, c, full = six
    img, report = cdc.recover(data)
    assert np.array_equal(img, cdc.decompress(data)) and report == codec.RecoverReport(4, 4, True, [])
    sym, head, report = cdc.recover_symbols(data)
    assert np.array_equal(sym, full) and head == c and report.tiles == []
    for g in range(1, 5):
        cut = data[:codec.layer_prefix_bytes(data, g)]
        img, report = cdc.recover(cut)
        want, partial = cdc.decompress_partial(cut)
        assert np.array_equal(img, want), g
        assert (report.ntiles, report.layers_total, report.file_crc_ok) == (4, 4, False)
        assert [(d.index, d.layers, d.channels, d.reason) for d in report.tiles] == ([] if g == 4 else [(t, g, ENDS32[g - 1], 'truncated') for t in range(4)])
    sym, _, report = cdc.recover_symbols(data[:codec.layer_prefix_bytes(data, 0)])       # the header alone: the fill symbol everywhere
    assert (sym == cdc.pred.conceal_fallback()).all() and [d.layers for d in report.tiles] == [0] * 4
    with pytest.raises(ValueError, match='header damaged'):
        cdc.recover(data[:codec.layer_prefix_bytes(data, 0) - 1])
    with pytest.raises(ValueError, match='--salvage'):
        cdc.recover(_write(cdc, 4, _image(40, 56, seed=3)))
    # what stays as it was
    with pytest.raises(ValueError, match='out of scope'):
        cdc.salvage(data)
    with pytest.raises(ValueError, match='CRC'):
        cdc.decompress(data[:codec.layer_prefix_bytes(data, 2)])


def _check_file(cdc, six, damaged, have, reasons):
    """recover_symbols of `damaged` against the rule on the full decode, the image against the decoder's own pixels for those symbols"""
    from imgcomp_cvpr_amd import codec
    data, c, full = six
    fill, L = cdc.pred.conceal_fallback(), cdc.L
    assert fill == codec.fill_symbol(cdc.ae.get_centers_variable().detach().cpu().numpy())
    sym, head, report = cdc.recover_symbols(damaged)
    want = RR.recover(full, have, 4, 4, L, fill)
    assert np.array_equal(sym, want)
    img, report2 = cdc.recover(damaged)
    assert report2 == report and np.array_equal(img, cdc._image(want, c))
    grid = codec.tile_grid(5, 7, 4, 4)
    assert [(d.index, d.channels, d.reason, d.latent) for d in report.tiles] == [(t, have[t], reasons[t], grid[t]) for t in sorted(reasons)]
    assert [d.layers for d in report.tiles] == [([0] + ENDS32).index(have[t]) for t in sorted(reasons)]
    assert (report.ntiles, report.layers_total, report.file_crc_ok) == (4, 4, False)
    return sym, report


def test_file_cut_inside_a_layer(cdc, six):
    data, c, full = six
    n = _seg_start(data, c, 2, 2)                                             # behind tile 1's segment of layer 2
    sym, report = _check_file(cdc, six, data[:n], [16, 16, 8, 8], {0: 'truncated', 1: 'truncated', 2: 'truncated', 3: 'truncated'})
    assert len(c.segments[2][2]) > 1
    assert np.array_equal(sym[:16, :4], full[:16, :4]) and np.array_equal(sym[:8], full[:8])               # tiles 0 and 1 are the top four rows
    assert not np.array_equal(sym[8:16], cdc.decode_symbols(data, channels=8)[0][8:16]), 'layer 2 of tiles 0 and 1 must show'
    assert [d.pixels for d in report.tiles] == [(0, 0, 32, 32), (0, 32, 32, 24), (32, 0, 8, 32), (32, 32, 8, 24)]
    _check_file(cdc, six, data[:n + 1], [16, 16, 8, 8], {t: 'truncated' for t in range(4)})                # one byte into tile 2's segment
    # ... and in the last layer: tiles 0 and 1 are whole and not in the report
    _, report = _check_file(cdc, six, data[:_seg_start(data, c, 3, 2)], [32, 32, 16, 16], {2: 'truncated', 3: 'truncated'})
    assert [d.index for d in report.tiles] == [2, 3]


def test_file_flipped_bytes(cdc, six):
    data, c, full = six
    sym, _ = _check_file(cdc, six, _flip(data, c, 1, 2), [32, 32, 4, 32], {2: 'crc'})     # layers 2 and 3 of tile 2 are intact, and lost
    assert np.array_equal(sym[:, :4], full[:, :4]) and np.array_equal(sym[:4], full[:4])
    sym, _ = _check_file(cdc, six, _flip(data, c, 0, 0), [0, 32, 32, 32], {0: 'crc'})
    assert np.array_equal(sym, R.conceal(full, [0], 4, 4, cdc.L, cdc.pred.conceal_fallback()))      # filled from tiles 1 and 2, every channel
    _check_file(cdc, six, _flip(_flip(data, c, 3, 1), c, 2, 3)[:-2], [32, 16, 32, 8], {1: 'crc', 3: 'crc'})


def test_many_equals_single(cdc, six):
    from imgcomp_cvpr_amd import codec
    data, c, _ = six
    other = _write(cdc, 6, _image(64, 96, seed=5))                            # an (32, 8, 12) volume: six tiles
    two = _write(cdc, 6, _image(40, 56, seed=4), layers=[2, 32])              # other layer ends: a group of its own
    oc = codec.parse_container(other)
    datas = [data, data[:_seg_start(data, c, 2, 2)], _flip(data, c, 1, 2), other[:_seg_start(other, oc, 1, 3)], _flip(other, oc, 0, 4),
             two, two[:codec.layer_prefix_bytes(two, 1) + 3], data[:codec.layer_prefix_bytes(data, 3)], _flip(data, c, 0, 0)]
    singles = [cdc.recover(d) for d in datas]
    for budget in (1 << 31, 4 << 20):                                        # the second: several decode launches per group
        many = cdc.recover_many(datas, max_workspace_bytes=budget)
        assert len(many) == len(singles)
        for i, ((a, ra), (b, rb)) in enumerate(zip(many, singles)):
            assert np.array_equal(a, b) and ra == rb, (budget, i)
    assert [len(r.tiles) for _, r in singles] == [0, 4, 1, 6, 1, 0, 4, 4, 1]
    with pytest.raises(ValueError, match='file 1: header damaged'):
        cdc.recover_many([data, data[:50]])
    with pytest.raises(ValueError, match='file 2: .*--salvage'):
        cdc.recover_many([data, data, _write(cdc, 5, _image(40, 56, seed=3))])
    assert cdc.recover_many([]) == []


def test_cli(cdc, six, cuda, tmp_path, capsys):
    from PIL import Image
    from imgcomp_cvpr_amd import codec
    data, c, _ = six
    files = {'a_whole': data, 'b_cut': data[:_seg_start(data, c, 2, 2)], 'c_flip': _flip(data, c, 1, 2)}
    src = tmp_path / 'in'
    src.mkdir()
    for name, d in files.items():
        (src / (name + '.icf')).write_bytes(d)
    (src / 'd_header.icf').write_bytes(data[:60])
    lines = {}
    for name, d in files.items():
        icf, png = str(src / (name + '.icf')), str(tmp_path / (name + '.png'))
        assert codec.main(['decompress', icf, png, '--recover', '--device', str(cuda)]) == 0
        img, report = cdc.recover(d)
        out = capsys.readouterr().out
        assert codec._recover_line(icf, report) in out.splitlines() and np.array_equal(np.asarray(Image.open(png)), img)
        lines[name] = codec._recover_line(icf, report)
    assert 'all 4 tiles hold all 4 layers' in lines['a_whole'] and 'tile 2 (crc) layers 1 of 4 = 4 channels' in lines['c_flip']
    assert '4 of 4 tiles incomplete' in lines['b_cut'] and 'tile 3 (truncated) layers 2 of 4 = 8 channels, pixels y 32..40 x 32..56' in lines['b_cut']
    assert codec.main(['decompress', str(src / 'd_header.icf'), str(tmp_path / 'x.png'), '--recover', '--device', str(cuda)]) == 2
    assert 'header damaged' in capsys.readouterr().err
    for extra in ('--salvage', '--partial', '--channels=4'):
        assert codec.main(['decompress', str(src / 'a_whole.icf'), str(tmp_path / 'x.png'), '--recover', extra, '--device', str(cuda)]) == 2
        assert '--recover does not go with' in capsys.readouterr().err
    out_dir = tmp_path / 'out'
    assert codec.main(['decompress-dir', str(src), str(out_dir), '--recover', '--batch', '4', '--device', str(cuda)]) == 2      # d_header is skipped
    cap = capsys.readouterr()
    assert 'd_header.icf: header damaged' in cap.err and 'total: 3 of 4 files' in cap.out
    for name, d in files.items():
        assert lines[name] in cap.out.splitlines()
        assert np.array_equal(np.asarray(Image.open(str(out_dir / (name + '.png')))), cdc.recover(d)[0])
    assert not os.path.exists(str(out_dir / 'd_header.png'))
