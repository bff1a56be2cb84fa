"""-m gpu: layered tiles (container format 6) -- the segment encoder (ic_pc_encode_segments_f32) against the host coder, the raster tile
decoder that restarts at layer cuts (ic_pc_decode_tiles_batch_layers_f32) against the coded symbols, the preview rule and, with
tables under the test's control, the host decoder restarted at the cuts; then whole files.  Every comparison is an equality."""
import ctypes

import numpy as np
import pytest
import torch

from tests import codec_cases as cc
from tests.test_gpu_codec_decoder import GARBAGE_TABLES, PENDING_PREFIXES, _draw, _load, _model

pytestmark = pytest.mark.gpu
GUARD = 0xA5
SYM_GUARD, Q_GUARD = -7, -12345.625
SHAPES = [(5, 3, 4), (2, 1, 1), (3, 1, 9), (3, 9, 1)]


@pytest.fixture(scope='module')
def pred(cuda, configs, syn_weights):
    return _load(cuda, configs[0], configs[1], syn_weights, 1e9)


def _ends_variants(C):
    """[C], [1, 2, C] (what of it fits below C), one layer per channel"""
    out = [[C], sorted(set([1, min(2, C), C])), list(range(1, C + 1))]
    return [e for i, e in enumerate(out) if e not in out[:i]]


# ---- the encoder through the ABI ----------------------------------------------------------------------------------------------

def _logits(pred, sym):
    """(N,C,h,w) int64 device symbols -> the logits ic_pc_encode_f32 is given by encode_stream"""
    q = pred.centers[torch.nn.functional.pad(sym, (4, 4, 4, 4, 4, 0))].contiguous()
    return pred.pc.logits(q, is_training=False)


def _raw_encode(cuda, pred, sym, ends, cap, L=None, slack=512):
    """ic_pc_encode_segments_f32 with guarded buffers -> (rc, [[bytes per segment] per volume], status (N, nsegs) list)"""
    from imgcomp_cvpr_amd import _lib
    sym = torch.as_tensor(np.ascontiguousarray(sym)).to(cuda).long()
    N, count, G = int(sym.shape[0]), int(sym[0].numel()), max(len(ends), 1)
    logits = _logits(pred, sym)
    out = torch.full((N * G * cap + slack,), GUARD, dtype=torch.uint8, device=cuda)
    nbytes = torch.full((N * G + slack,), SYM_GUARD, dtype=torch.int64, device=cuda)
    status = torch.full((N * G + slack,), SYM_GUARD, dtype=torch.int32, device=cuda)
    host_ends = (ctypes.c_longlong * max(len(ends), 1))(*ends)
    rc = _lib.lib.ic_pc_encode_segments_f32(_lib.ptr(logits), _lib.ptr(sym), N, count, pred.pc.L if L is None else L, pred.freqs_resolution,
                                           host_ends, len(ends), _lib.ptr(out), cap, _lib.ptr(nbytes), _lib.ptr(status),
                                           _lib.current_stream(cuda))
    torch.cuda.synchronize()
    assert bool((out[N * G * cap:] == GUARD).all()) and bool((nbytes[N * G:] == SYM_GUARD).all()) and bool((status[N * G:] == SYM_GUARD).all())
    if rc != 0:
        assert bool((out == GUARD).all()) and bool((nbytes == SYM_GUARD).all()) and bool((status == SYM_GUARD).all()), 'a refused call wrote something'
        return rc, None, None
    host, nb, st = out[:N * G * cap].view(N, G, cap).cpu().numpy(), nbytes[:N * G].view(N, G).tolist(), status[:N * G].view(N, G).tolist()
    for n in range(N):
        for g in range(G):
            assert 0 <= nb[n][g] <= cap and (host[n, g, nb[n][g]:] == GUARD).all(), 'segment ({}, {}): a store at or beyond its end'.format(n, g)
    return rc, [[bytes(host[n, g, :nb[n][g]]) for g in range(G)] for n in range(N)], st


def _host_segments(pred, sym_chw, ends):
    """the host coder over get_all's tables, cut at the cumulative symbol counts `ends`"""
    freqs = pred.get_all(pred.pad_symbols_volume(sym_chw))[1]
    flat = sym_chw.reshape(-1).astype(np.int64)
    return [cc.host_encode(flat[max(1, a):b], freqs[max(1, a):b])[0] for a, b in zip([0] + list(ends), ends)]


@pytest.mark.parametrize('shape', SHAPES)
def test_encoder_segments_are_the_host_coders(cuda, pred, shape):
    from imgcomp_cvpr_amd import _lib
    C, plane = shape[0], shape[1] * shape[2]
    rs = np.random.RandomState(sum(shape))
    sym = rs.randint(0, pred.pc.L, size=(2,) + shape).astype(np.int64)
    cap = int(_lib.lib.ic_pc_encode_capacity_bytes(sym[0].size))
    whole = pred.encode_stream(sym)                                           # ic_pc_encode_f32
    for layer_ends in _ends_variants(C):
        ends = [e * plane for e in layer_ends]
        rc, segs, status = _raw_encode(cuda, pred, sym, ends, cap)
        assert rc == 0 and status == [[0] * len(ends)] * 2, (shape, ends, rc, status)
        for n in range(2):
            assert segs[n] == _host_segments(pred, sym[n], ends), (shape, ends, n)
            if len(ends) == 1:
                assert segs[n][0] == whole[n][0]                              # nsegs = 1: the existing entry, byte for byte
        surface = pred.encode_stream(sym, seg_ends=ends)
        assert [s for s, _ in surface] == segs and [f for _, f in surface] == [int(sym[n, 0, 0, 0]) for n in range(2)]
    if plane == 1:                                                            # ends[0] == 1: the empty segment
        assert _raw_encode(cuda, pred, sym, list(range(1, C + 1)), cap)[1][0][0] == b'\x80'
    # cuts anywhere, not only at channel planes
    ends = sorted(set([1, 2, sym[0].size // 2, sym[0].size]))
    assert _raw_encode(cuda, pred, sym, ends, cap)[1][1] == _host_segments(pred, sym[1], ends)


def test_encoder_capacity_and_refusals(cuda, pred):
    from imgcomp_cvpr_amd import _lib
    sym = np.random.RandomState(4).randint(0, pred.pc.L, size=(2, 5, 3, 4)).astype(np.int64)
    ends = [12, 24, 60]
    want = [_host_segments(pred, sym[n], ends) for n in range(2)]
    cap = max(len(want[n][g]) for n in range(2) for g in range(2))
    assert all(len(want[n][2]) > cap for n in range(2)), 'the long segment must not fit'
    rc, segs, status = _raw_encode(cuda, pred, sym, ends, cap)                # (the guards: nothing at or beyond capacity)
    assert rc == 0 and status == [[0, 0, 2]] * 2
    assert all(segs[n][g] == want[n][g] for n in range(2) for g in range(2))
    assert all(want[n][2].startswith(segs[n][2]) for n in range(2))
    with pytest.raises(ValueError, match='capacity too small'):
        pred.encode_stream(sym, seg_ends=ends, capacity=cap)
    big = int(_lib.lib.ic_pc_encode_capacity_bytes(60))
    for bad in ([12, 12, 60], [24, 12, 60], [0, 60], [12, 59], [12, 61], []):
        assert _raw_encode(cuda, pred, sym, bad, big)[0] == -1, bad           # IC_ERR_ARG
    assert _raw_encode(cuda, pred, sym, list(range(1, 17)) + [60], big)[0] == -2      # 17 segments: IC_ERR_UNSUPPORTED
    assert _raw_encode(cuda, pred, sym, ends, big, L=17)[0] == -2
    assert _raw_encode(cuda, pred, sym, list(range(1, 16)) + [60], big)[0] == 0       # 16 are served
    with pytest.raises(ValueError, match='wavefront'):
        pred.encode_stream(sym, seg_ends=ends, order='wavefront')


# ---- the decoder through the ABI ----------------------------------------------------------------------------------------------

def _raw_layers(cuda, pred, volumes, th, tw, ends, K, fill, want_syms=True, want_q=True, flags=0, unneeded='real', nlayers=None,
                ws_short=0, break_seg=None, slack=4096):
    """ic_pc_decode_tiles_batch_layers_f32 through the ABI.  volumes: [(streams, first_syms, (C,h,w))], streams[t] the tile's list of
    segments.  unneeded: what stands for the segments of layers that begin at or above K -- 'real' (their bytes), 'zero' ({0, 0}),
    'other' (other bytes at another place).  symbols, q, status and the workspace carry guard values; the volumes lie `slack` cells
    apart.  The tile descriptors' stream fields hold nonsense: they are not read.
    -> (return code, [symbols per volume] or None, [q per volume, device] or None, status list)"""
    from imgcomp_cvpr_amd import _lib, codec
    G = len(ends)
    junk = bytes(np.random.RandomState(99).randint(0, 256, size=37).astype(np.uint8))
    tiles, segs, blobs, pos, offs, total = [], [], [junk], len(junk), [], slack
    for n, (streams, firsts, (C, h, w)) in enumerate(volumes):
        for t, (y0, x0, a, b) in enumerate(codec.tile_grid(h, w, th, tw)):
            tiles.append((y0, x0, a, b, -5, 1 << 40, firsts[t], n))
            for g in range(len(streams[t])):
                needed = g == 0 or (g - 1 < len(ends) and ends[g - 1] < K)
                if needed or unneeded == 'real':
                    segs.append((pos, len(streams[t][g])))
                    blobs.append(bytes(streams[t][g]))
                    pos += len(streams[t][g])
                else:
                    segs.append((0, 0) if unneeded == 'zero' else (3, len(junk) - 3))
        offs.append(total)
        total += C * h * w + slack
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
    need = int(_lib.lib.ic_pc_decode_tiles_batch_layers_workspace_bytes(C, max(t[2] for t in tiles), max(t[3] for t in tiles), len(tiles),
                                                                        len(volumes), 24, min(max(nl, 1), 16)))
    assert need > int(_lib.lib.ic_pc_decode_tiles_batch_workspace_bytes(C, max(t[2] for t in tiles), max(t[3] for t in tiles), len(tiles),
                                                                        len(volumes), 24))
    ws = torch.full((need + slack,), GUARD, dtype=torch.uint8, device=cuda)
    centers = pred.centers.contiguous().float()
    host_ends = (ctypes.c_int * max(G, 1))(*ends)
    rc = _lib.lib.ic_pc_decode_tiles_batch_layers_f32(
        _lib.ptr(data), pos, table, len(tiles), vtable, len(volumes), pred.pc._tab, _lib.ptr(centers), pred.pc._k, pred.pc.L,
        pred.freqs_resolution, _lib.ptr(sym), _lib.ptr(q), _lib.ptr(status), C, _lib.ptr(ws), need - ws_short, int(flags),
        _lib.current_stream(cuda), int(K), int(fill), host_ends, nl, seg_table)
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


def _coded(pred, syms, th, tw, ends):
    vols = []
    for sym in syms:
        coded = pred.encode_tiles(sym, th, tw, layer_ends=ends)
        vols.append(([s for s, _ in coded], [f for _, f in coded], tuple(sym.shape)))
    return vols


def _check_all_k(cuda, pred, vols, syms, th, tw, ends, what):
    from imgcomp_cvpr_amd import codec
    fill, C = pred.conceal_fallback(), syms[0].shape[0]
    centers = pred.centers.contiguous().float()
    rc, full, _, status = _raw_layers(cuda, pred, vols, th, tw, ends, C, fill)
    assert rc == 0 and status == [0] * len(status), (what, rc, status)
    assert all(np.array_equal(a, b) for a, b in zip(full, syms)), '{}: the full decode is not what was coded'.format(what)
    for K in range(1, C + 1):
        wants = [codec.preview_symbols(f, K, fill) for f in full]
        for unneeded in ('real', 'zero', 'other'):
            rc, got, q, status = _raw_layers(cuda, pred, vols, th, tw, ends, K, fill, unneeded=unneeded)
            assert rc == 0 and status == [0] * len(status), (what, K, unneeded, rc, status)
            assert all(np.array_equal(g, want) for g, want in zip(got, wants)), '{} K = {} ({}): not the rule on the full decode'.format(what, K, unneeded)
            assert all(torch.equal(qq, centers[torch.as_tensor(want).to(cuda)]) for qq, want in zip(q, wants))
    return full


@pytest.mark.parametrize('shape', SHAPES)
def test_decoder_layers_single_tile(cuda, pred, shape):
    C = shape[0]
    sym = np.random.RandomState(10 + sum(shape)).randint(0, pred.pc.L, size=shape).astype(np.int64)
    for ends in _ends_variants(C):
        vols = _coded(pred, [sym], shape[1], shape[2], ends)
        assert vols[0][0][0] == _host_segments(pred, sym, [e * shape[1] * shape[2] for e in ends])
        _check_all_k(cuda, pred, vols, [sym], shape[1], shape[2], ends, '{} ends {}'.format(shape, ends))
        if len(ends) == 1:                                                    # G = 1: the segment is the format-4 stream of the tile
            assert vols[0][0][0][0] == pred.encode_tiles(sym, shape[1], shape[2])[0][0]


def test_decoder_layers_two_volumes_edge_tiles(cuda, pred):
    from imgcomp_cvpr_amd import codec
    rs = np.random.RandomState(21)
    syms = [rs.randint(0, pred.pc.L, size=s).astype(np.int64) for s in ((6, 5, 7), (6, 3, 2))]
    assert sorted(set(g[2:] for g in codec.tile_grid(5, 7, 4, 4))) == [(1, 3), (1, 4), (4, 3), (4, 4)]
    fill = pred.conceal_fallback()
    for ends in ([6], [1, 2, 6], [1, 2, 3, 4, 5, 6]):
        vols = _coded(pred, syms, 4, 4, ends)
        full = _check_all_k(cuda, pred, vols, syms, 4, 4, ends, 'two volumes, ends {}'.format(ends))
        for K in (2, 6):
            wants = [codec.preview_symbols(f, K, fill) for f in full]
            rc, none, q_only, status = _raw_layers(cuda, pred, vols, 4, 4, ends, K, fill, want_syms=False)
            assert rc == 0 and none is None and status == [0] * len(status)
            rc, s_only, none, status = _raw_layers(cuda, pred, vols, 4, 4, ends, K, fill, want_q=False)
            assert rc == 0 and none is None and all(np.array_equal(a, b) for a, b in zip(s_only, wants))
            centers = pred.centers.contiguous().float()
            assert all(torch.equal(qq, centers[torch.as_tensor(w).to(cuda)]) for qq, w in zip(q_only, wants))
            # the Python surface; entries of layers that are not needed may be None
            thin = [([[b if (g == 0 or ends[g - 1] < K) else None for g, b in enumerate(segs)] for segs in streams], firsts, shape)
                    for streams, firsts, shape in vols]
            both = pred.decode_tiles_batch(thin, 4, 4, want='both', channels=K, layer_ends=ends)
            for (qq, s), want in zip(both, wants):
                assert np.array_equal(s.cpu().numpy(), want) and torch.equal(qq, centers[s])
        assert all(np.array_equal(s.cpu().numpy(), f) for s, f in zip(pred.decode_tiles_batch(vols, 4, 4, want='symbols', layer_ends=ends), full))
    with pytest.raises(ValueError, match='conceal'):
        pred.decode_tiles_batch(vols, 4, 4, conceal=True, layer_ends=[1, 2, 3, 4, 5, 6])
    with pytest.raises(ValueError, match='need the segments'):
        pred.decode_tiles_batch([([[None] * 6] * 4, vols[0][1], (6, 5, 7))], 4, 4, layer_ends=[1, 2, 3, 4, 5, 6])


def test_decoder_refusals_write_nothing(cuda, pred):
    from imgcomp_cvpr_amd import _lib
    sym = np.random.RandomState(2).randint(0, pred.pc.L, size=(6, 5, 7)).astype(np.int64)
    fill, ends = pred.conceal_fallback(), [1, 2, 6]
    vols = _coded(pred, [sym], 4, 4, ends)
    assert _raw_layers(cuda, pred, vols, 4, 4, ends, 6, fill)[0] == 0
    for flags in (_lib.PC_DECODE_WAVEFRONT, _lib.PC_DECODE_RECOMPUTE, _lib.PC_DECODE_PER_LAYER):
        assert _raw_layers(cuda, pred, vols, 4, 4, ends, 6, fill, flags=flags)[0] == -2, flags            # IC_ERR_UNSUPPORTED
    for bad in ([2, 2, 6], [0, 2, 6], [1, 2, 5], [1, 2, 7], [2, 1, 6]):
        assert _raw_layers(cuda, pred, vols, 4, 4, bad, 6, fill)[0] == -1, bad                            # IC_ERR_ARG
    for nl in (0, 17, -1):
        assert _raw_layers(cuda, pred, vols, 4, 4, ends, 6, fill, nlayers=nl)[0] == -1, nl
    for K in (0, 7):
        assert _raw_layers(cuda, pred, vols, 4, 4, ends, K, fill)[0] == -1
    assert _raw_layers(cuda, pred, vols, 4, 4, ends, 2, pred.pc.L)[0] == -1
    # a needed segment outside [0, total_bytes): refused; the same descriptor in a layer that K does not reach: not looked at
    outside = [lambda total: (total - 1, 2), lambda total: (-1, 1), lambda total: (0, -1), lambda total: (total + 1, 0)]
    for seg in outside:
        assert _raw_layers(cuda, pred, vols, 4, 4, ends, 6, fill, break_seg=(3 * 1 + 2, seg))[0] == -1
        assert _raw_layers(cuda, pred, vols, 4, 4, ends, 1, fill, break_seg=(3 * 1 + 0, seg))[0] == -1
        assert _raw_layers(cuda, pred, vols, 4, 4, ends, 2, fill, break_seg=(3 * 1 + 2, seg))[0] == 0
    assert _raw_layers(cuda, pred, vols, 4, 4, ends, 6, fill, ws_short=1)[0] == -3                         # IC_ERR_WORKSPACE
    assert _lib.lib.ic_pc_decode_tiles_batch_layers_workspace_bytes(6, 4, 4, 4, 1, 24, 0) == 0
    assert _lib.lib.ic_pc_decode_tiles_batch_layers_workspace_bytes(6, 4, 4, 4, 1, 24, 17) == 0
    wide, _ = _model(cuda, [0, 1, 2, 3, 2, 1], 'res_shallow_64')
    assert wide.pc._k == 64
    wvols = _coded(wide, [sym], 4, 4, ends)                                   # the encoder knows no width
    assert _raw_layers(cuda, wide, wvols, 4, 4, ends, 6, 0)[0] == -2
    with pytest.raises(ValueError, match='k = 24, this one has k = 64'):
        wide.decode_tiles_batch(wvols, 4, 4, layer_ends=ends)


# ---- hard coder states on the device ------------------------------------------------------------------------------------------

def _const_segments(table, sym_chw, ends):
    """the host coder over one constant table, cut at the layer ends"""
    flat, plane = sym_chw.reshape(-1), sym_chw.shape[1] * sym_chw.shape[2]
    return [cc.host_encode(flat[max(1, a * plane):b * plane], [table] * (b * plane - max(1, a * plane)))[0] for a, b in zip([0] + list(ends), ends)]


def test_pending_run_across_the_cuts(cuda):
    """a run of pending bits longer than 64 is open at the cuts (24 and 48 symbols into a run of 60)"""
    model, table = _model(cuda, [0, 1, 2, 3, 2, 1])
    shape, steps = (4, 4, 6), 60
    for lead in (0, 3):
        prefix = PENDING_PREFIXES[lead]
        run, reached = cc.straddle_symbols(table, steps, prefix)
        assert reached > 64
        rs = np.random.RandomState(40 + lead)
        sym = np.array([int(rs.randint(6))] + list(prefix) + run + rs.randint(6, size=96 - 1 - lead - steps).tolist(), np.int64).reshape(shape)
        for ends in ([1, 2, 4], [1, 2, 3, 4], [4]):
            vols = _coded(model, [sym], 4, 6, ends)
            assert vols[0][0][0] == _const_segments(table, sym, ends), 'the device segments are not the host coder\'s'
            _check_all_k(cuda, model, vols, [sym], 4, 6, ends, 'pending run, lead {}, ends {}'.format(lead, ends))


def test_floor_frequency_symbols_across_the_cuts(cuda):
    model, table = _model(cuda, [0, 40, 40, 40, 40, 40])
    assert table[0] == 1
    rs = np.random.RandomState(17)
    sym = rs.randint(0, 6, size=(5, 3, 4)).astype(np.int64)
    sym[:3] = 0                                                               # runs of the frequency-1 symbol over two cuts
    for ends in ([1, 2, 5], [1, 2, 3, 4, 5]):
        vols = _coded(model, [sym], 3, 4, ends)
        assert vols[0][0][0] == _const_segments(table, sym, ends)
        _check_all_k(cuda, model, vols, [sym], 3, 4, ends, 'floor frequency, ends {}'.format(ends))


@pytest.mark.parametrize('bias', GARBAGE_TABLES, ids=['floor L=6', 'exact L=3', 'skewed L=16'])
def test_arbitrary_bytes_as_segments(cuda, bias):
    """bytes that no encoder wrote, every segment a string of its own: the symbols and the status are those of the word-level model
    of the decoder (codec_cases.model_decode, equal to the host decoder) restarted at every cut"""
    from imgcomp_cvpr_amd import codec
    model, table = _model(cuda, bias)
    L = len(table)
    rs = np.random.RandomState(80 + L)
    shape, tile, ends = (6, 5, 7), (4, 4), [1, 2, 6]
    valid = model.encode_stream(_draw(rs, table, (6, 4, 4)))[0]
    strings = [d for _, d in cc.garbage_strings(valid, seed=90 + L)]
    grid = codec.tile_grid(5, 7, 4, 4)
    for r in range(0, len(strings), 6):
        streams = [[strings[(r + 3 * t + g) % len(strings)] for g in range(3)] for t in range(4)]
        firsts = [int(v) for v in rs.randint(L, size=4)]
        want = np.full(shape, -1, np.int64)
        for t, (y0, x0, a, b) in enumerate(grid):
            flat = [firsts[t]]
            for g, (lo, hi) in enumerate(zip([0] + ends, ends)):
                n = hi * a * b - max(1, lo * a * b)
                got, status = cc.model_decode(streams[t][g], [table] * n)
                assert status == 0 and got == cc.host_decode(streams[t][g], [table] * n)
                flat += got
            want[:, y0:y0 + a, x0:x0 + b] = np.array(flat, np.int64).reshape(6, a, b)
        assert want.min() >= 0 and want.max() < L
        fill = model.conceal_fallback()
        for K in (1, 2, 6):
            rc, got, _, status = _raw_layers(cuda, model, [(streams, firsts, shape)], 4, 4, ends, K, fill, unneeded='zero')
            assert rc == 0 and status == [0] * 4, (r, K, status)
            assert got[0].min() >= 0 and got[0].max() < L
            assert np.array_equal(got[0], codec.preview_symbols(want, K, fill)), 'strings {}.., K = {}'.format(r, K)


def test_total_over_the_limit_with_cuts(cuda):
    """one over the coder's limit at every position: the status of a tile is 1 as soon as one coded symbol lies inside what is
    decoded, whichever segment holds it; a prefix that is the uncoded first symbol alone has consulted no table: status 0.
    What this cannot show is the fold itself (an error in an early segment, a clean last one): the tests control the tables through
    the last layer's bias, so a model's table is one row at every position, and a row over the limit fails in every segment that
    codes a symbol.  The one clean segment such a model has is an EMPTY one, and only segment 0 can be empty (the uncoded first
    symbol alone), which comes first; so with these tables the status with and without the fold are the same in every case."""
    from imgcomp_cvpr_amd import arithmetic_coding as ac
    model, table = _model(cuda, [40, 0, 0, 0], resolution=2.0 ** 30)
    assert sum(table) == ac.MAX_TOTAL + 1
    data = np.random.RandomState(9).randint(0, 256, size=40).astype(np.uint8).tobytes()
    fill = model.conceal_fallback()
    vol = ([[data[:9], data[9:20], data[20:]]], [2], (3, 1, 2))
    for K, want in ((1, 1), (2, 1), (3, 1)):
        rc, syms, _, status = _raw_layers(cuda, model, [vol], 1, 2, [1, 2, 3], K, fill)
        assert rc == 0 and status == [want] and syms[0].min() >= 0 and syms[0].max() < 4 and syms[0][0, 0, 0] == 2
    rc, syms, _, status = _raw_layers(cuda, model, [([[data[:9], data[9:20]]], [2], (2, 1, 1))], 1, 1, [1, 2], 1, fill)
    assert rc == 0 and status == [0] and syms[0].reshape(-1).tolist() == [2, fill]       # the first symbol alone: no table consulted


# ---- files ----------------------------------------------------------------------------------------------------------------------

def _image(H, W_, seed=9):
    from imgcomp_cvpr_amd import weights as W
    return np.ascontiguousarray(W.synthetic_image((1, 3, H, W_), 'natural', seed=seed)[0].transpose(1, 2, 0))


@pytest.fixture(scope='module')
def cdc(cuda, configs, syn_weights):
    from imgcomp_cvpr_amd import codec
    return codec.Codec(configs[0], configs[1], syn_weights, cuda)


FORMATS = {4: ((4, 4), 'raster', True, None), 5: ((4, 4), 'wavefront', False, None), 6: ((4, 4), 'raster', False, 'default')}


def _write(c, version, img, many=False, layers=None):
    c.tile, c.order, c.checked, c.layers = FORMATS[version]
    if layers is not None:
        c.layers = layers
    try:
        return c.compress_many(img) if many else c.compress(img)
    finally:
        c.tile, c.order, c.checked, c.layers = None, 'raster', False, None


@pytest.mark.parametrize('layers', ['default', [32], [1, 2, 32]], ids=['default', 'one layer', '1,2,32'])
def test_file_equals_format_4(cdc, layers):
    from imgcomp_cvpr_amd import codec
    img = _image(40, 56)
    data, four = _write(cdc, 6, img, layers=layers), _write(cdc, 4, img)
    head, head4 = codec.parse_container(data), codec.parse_container(four)
    ends = [4, 8, 16, 32] if layers == 'default' else layers
    assert head.version == 6 and head.layer_ends == ends and (head.h, head.w, len(head.streams)) == (5, 7, 4)
    assert head.first_syms == head4.first_syms
    if len(ends) == 1:
        assert [s[0] for s in head.streams] == head4.streams              # G = 1: the format-4 streams, byte for byte
    for K in [None] + ends:
        a, b = cdc.decode_symbols(data, channels=K)[0], cdc.decode_symbols(four, channels=K)[0]
        assert a.dtype == np.int64 and np.array_equal(a, b), K
        assert np.array_equal(cdc.decompress(data, channels=K), cdc.decompress(four, channels=K)), K
    assert np.array_equal(cdc.decompress(data, channels=5), cdc.decompress(four, channels=5))       # not a layer end
    ok, text = codec.verify_file(data)
    assert ok and 'G = {}'.format(len(ends)) in text
    flipped = bytearray(data)
    flipped[codec.layer_prefix_bytes(data, 0) + 3] ^= 0x04
    assert not codec.verify_file(bytes(flipped))[0]
    with pytest.raises(ValueError, match='CRC'):
        cdc.decompress(bytes(flipped))
    with pytest.raises(ValueError, match='out of scope'):
        cdc.salvage(data)


def test_prefix_decodes_as_a_preview(cdc):
    from imgcomp_cvpr_amd import codec
    img = _image(40, 56, seed=3)
    data = _write(cdc, 6, img)
    ends = [4, 8, 16, 32]
    previews = {e: cdc.decompress(data, channels=e) for e in ends}
    for g in range(1, 5):
        n = codec.layer_prefix_bytes(data, g)
        out, report = cdc.decompress_partial(data[:n])
        assert report == codec.PartialReport(4, g, ends[g - 1], False), (g, report)
        assert np.array_equal(out, previews[ends[g - 1]]), g
        if g > 1:
            out, report = cdc.decompress_partial(data[:n - 1])                # one byte less: the layer before
            assert report.layers_decoded == g - 1 and np.array_equal(out, previews[ends[g - 2]])
        else:
            with pytest.raises(ValueError, match='no complete layer'):
                cdc.decompress_partial(data[:n - 1])
    out, report = cdc.decompress_partial(data)
    assert report == codec.PartialReport(4, 4, 32, True) and np.array_equal(out, cdc.decompress(data))
    with pytest.raises(ValueError, match='header damaged'):
        cdc.decompress_partial(data[:codec.layer_prefix_bytes(data, 0) - 1])
    with pytest.raises(ValueError, match='header damaged'):
        cdc.decompress_partial(_write(cdc, 4, img))


def test_many_equals_single(cdc):
    imgs = [_image(40, 56, seed=3), _image(8, 8, seed=4), _image(64, 96, seed=5)]
    sixes = [_write(cdc, 6, im) for im in imgs]
    assert _write(cdc, 6, imgs, many=True) == sixes                       # compress_many: the same bytes, file by file
    datas = sixes + [_write(cdc, 4, im) for im in imgs] + [_write(cdc, 5, im) for im in imgs] + [_write(cdc, 6, imgs[0], layers=[2, 32])]
    for K in (None, 8):
        singles = [cdc.decompress(d, channels=K) for d in datas]
        many = cdc.decompress_many(datas, channels=K)
        assert len(many) == len(singles) and all(np.array_equal(a, b) for a, b in zip(many, singles)), K


def test_options_and_cli(cdc, cuda, configs, syn_weights, tmp_path, capsys):
    from PIL import Image
    from imgcomp_cvpr_amd import codec, config_parser as cp, weights as W
    for kw, why in ((dict(layers='default'), 'needs a tile extent'), (dict(tile=(4, 4), layers=[4, 31]), 'not C = 32'),
                    (dict(tile=(4, 4), layers='default', order='wavefront'), 'wavefront'), (dict(tile=(4, 4), layers='other'), "'default'")):
        with pytest.raises(ValueError, match=why):
            codec.Codec(configs[0], configs[1], syn_weights, cuda, **kw)
    assert cdc.layered_refusal is None
    pc64, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow_64'))
    w64 = W.synthetic_weights(configs[0], pc64)
    with pytest.raises(ValueError, match='k = 24, this one has k = 64'):
        codec.Codec(configs[0], pc64, w64, cuda, tile=(4, 4), layers='default')
    img = _image(40, 56, seed=6)
    src = str(tmp_path / 'in.png')
    Image.fromarray(img).save(src)
    icf, png = str(tmp_path / 'a.icf'), str(tmp_path / 'a.png')
    assert codec.main(['compress', src, icf, '--tile', '32', '--progressive', '--device', str(cuda)]) == 0
    capsys.readouterr()
    data = open(icf, 'rb').read()
    cdc.tile, cdc.layers = (4, 4), 'default'
    try:
        assert data == cdc.compress(img)
    finally:
        cdc.tile, cdc.layers = None, None
    cut = str(tmp_path / 'cut.icf')
    with open(cut, 'wb') as f:
        f.write(data[:codec.layer_prefix_bytes(data, 2) + 5])
    assert codec.main(['decompress', cut, png, '--partial', '--device', str(cuda)]) == 0
    assert 'layers decoded 2 of 4' in capsys.readouterr().out
    assert np.array_equal(np.asarray(Image.open(png)), cdc.decompress(data, channels=8))
    assert codec.main(['decompress', cut, png, '--device', str(cuda)]) == 2                    # the strict reader refuses the cut file
    assert 'CRC' in capsys.readouterr().err
    assert codec.main(['compress', src, icf, '--tile', '32', '--layers', '4,31', '--device', str(cuda)]) == 2
    assert 'not C = 32' in capsys.readouterr().err
    assert codec.main(['verify', cut]) == 1 and '2 of 4 layers complete' in capsys.readouterr().out
