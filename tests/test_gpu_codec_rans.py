"""-m gpu: lane-parallel rANS tiles (container format 12).  The encoder (ic_pc_encode_segments_f32 with nsegs = -W) and the decoder
(IC_PC_DECODE_RANS(W) on ic_pc_decode_tiles_batch_channels_f32) against the rule of tests/rans_rule.py over the device's own tables;
hard tables and byte strings no encoder wrote on a constant table; then whole files against format 5.  Every device buffer comes
from tests.fenced.fenced(), workspaces have exactly the queried size and are handed over dirty (0xFF, then 0x00; the outputs must be
bit-identical), every comparison is an equality."""
import ctypes
import struct

import numpy as np
import pytest
import torch

from tests import rans_rule as rr
from tests.fenced import OUT_FENCE, ZERO_FENCE, IN_FENCE, check_fences, fenced, poison, refence, snapshot, unchanged
from tests.test_gpu_codec_decoder import _load, _model

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1, 1), (3, 1, 9), (4, 5, 7), (8, 16, 16), (16, 16, 16))
CASES = [(s, W) for s in SHAPES for W in ((8, 16, 32, 64) if s == (4, 5, 7) else (8, 64))]
IDS = ['{}x{}x{}-W{}'.format(*(s + (W,))) for s, W in CASES]
N_ENC, L_ENC = 2, 6


@pytest.fixture(scope='module')
def pred(cuda, configs, syn_weights):
    return _load(cuda, configs[0], configs[1], syn_weights, 1e9)


# ---- the encoder through the ABI -------------------------------------------------------------------------------------------------------

def _enc_inputs(cuda, shape, W, L=L_ENC, seed=0, scale=3.0):
    """random logits and symbols in round order for N_ENC volumes of `shape`, holes where the rounds have them -> (device logits,
    symbols (N, R W), the device's own tables (N, R W, L))"""
    from imgcomp_cvpr_amd import _lib, codec
    rounds = codec.rans_rounds(shape[0], shape[1], shape[2], W)
    count = rounds.size
    rs = np.random.RandomState(seed + count + W)
    logits = (rs.randn(N_ENC, count, L) * scale).astype(np.float32)
    sym = rs.randint(0, L, size=(N_ENC, count)).astype(np.int64)
    sym[:, rounds.reshape(-1) < 0] = _lib.PC_ENCODE_SKIP
    dl = fenced(logits, torch.float32, cuda, IN_FENCE, 'logits')
    freqs = fenced((N_ENC * count, L), torch.int64, cuda, OUT_FENCE, 'freqs')
    pr = fenced((N_ENC * count, L), torch.float32, cuda, OUT_FENCE, 'pr')
    rc = _lib.lib.ic_pc_logits_to_freqs_f32(_lib.ptr(dl), N_ENC * count, L, 1e9, _lib.ptr(freqs), _lib.ptr(pr), _lib.current_stream(cuda))
    torch.cuda.synchronize()
    assert rc == 0
    check_fences(dl, freqs, pr)
    return dl, sym, freqs.cpu().numpy().reshape(N_ENC, count, L)


def _raw_encode(cuda, dl, coded, nsegs, cap=None, end0=None, count=None, L=L_ENC, resolution=1e9):
    """ic_pc_encode_segments_f32 with the given nsegs on fenced buffers, the integer input once between fences of 0xFF and once of
    0x00 -> (rc, [the last nbytes bytes of each volume's capacity], status list); a refused call must leave every output untouched"""
    from imgcomp_cvpr_amd import _lib
    N, n = coded.shape
    count = n if count is None else count
    cap = int(_lib.lib.ic_pc_encode_capacity_bytes(n)) if cap is None else cap
    ds = fenced(coded, torch.int64, cuda, IN_FENCE, 'symbols')
    results = []
    for fill in (IN_FENCE, ZERO_FENCE):
        refence(ds, fill)
        out = poison(fenced((N * cap,), torch.uint8, cuda, OUT_FENCE, 'bitstream'), 0x5A)
        nbytes = fenced((N,), torch.int64, cuda, OUT_FENCE, 'nbytes')
        status = fenced((N,), torch.int32, cuda, OUT_FENCE, 'status')
        before = snapshot(out, nbytes, status)
        host_ends = (ctypes.c_longlong * 1)(count if end0 is None else end0)
        rc = _lib.lib.ic_pc_encode_segments_f32(_lib.ptr(dl), _lib.ptr(ds), N, count, L, resolution, host_ends, nsegs, _lib.ptr(out), cap,
                                                _lib.ptr(nbytes), _lib.ptr(status), _lib.current_stream(cuda))
        torch.cuda.synchronize()
        check_fences(dl, ds, out, nbytes, status)
        if rc != 0:
            unchanged(before, out, nbytes, status)
            return rc, None, None
        host, nb = out.view(N, cap).cpu().numpy(), nbytes.tolist()
        assert all(0 <= b <= cap for b in nb)
        for v in range(N):                                                    # in front of the stream nothing was stored
            assert (host[v, :cap - nb[v]] == 0x5A).all() or status.tolist()[v] != 0
        results.append(([bytes(host[v, cap - nb[v]:]) for v in range(N)], status.tolist()))
    assert results[0] == results[1], 'the result depends on what lies around the symbols'
    return 0, results[0][0], results[0][1]


@pytest.mark.parametrize('shape,W', [c for c in CASES if c[0] != (1, 1, 1)], ids=[i for c, i in zip(CASES, IDS) if c[0] != (1, 1, 1)])
def test_encoder_bytes_are_the_rules(cuda, shape, W):
    """(the 1 x 1 x 1 tile has no round: count = 0 is IC_ERR_ARG as ever, the surface function writes its W states itself)"""
    from imgcomp_cvpr_amd import _lib
    assert _lib.PC_ENCODE_RANS(W) == -W
    dl, sym, freqs = _enc_inputs(cuda, shape, W)
    rc, tails, status = _raw_encode(cuda, dl, sym, -W)
    assert rc == 0 and status == [0] * N_ENC
    for v in range(N_ENC):
        want, st = rr.encode(freqs[v].tolist(), sym[v].tolist(), W)
        assert st == 0 and tails[v] == want, (shape, W, v, len(tails[v]), len(want))
    # the logits of a hole are not looked at
    holes = dl.clone()
    holes[torch.as_tensor(sym == -1).to(cuda)] = float('nan')
    assert _raw_encode(cuda, fenced(holes, torch.float32, cuda, IN_FENCE, 'logits with holes'), sym, -W) == (0, tails, status)
    # a capacity one word short: status 2, nothing outside the buffer (the fences), nothing claimed
    longest = max(len(t) for t in tails)
    rc, short, status = _raw_encode(cuda, dl, sym, -W, cap=longest - 2)
    assert rc == 0 and [s for s, t in zip(status, tails) if len(t) == longest] == [2] * sum(len(t) == longest for t in tails)
    assert all(s == 2 or short[v] == tails[v] for v, s in enumerate(status))
    rc, exact, status = _raw_encode(cuda, dl, sym, -W, cap=longest)
    assert rc == 0 and status == [0] * N_ENC and exact == tails


def test_encoder_refusals_write_nothing(cuda):
    shape, W = (4, 5, 7), 8
    dl, sym, _ = _enc_inputs(cuda, shape, W)
    count = sym.shape[1]
    assert _raw_encode(cuda, dl, sym, -W)[0] == 0
    for nsegs in (-1, -7, -65, -128, -9, -24, 0):
        assert _raw_encode(cuda, dl, sym, nsegs)[0] == -1, nsegs               # IC_ERR_ARG
    assert count % 8 == 0 and (count - 8) % 64 != 0
    assert _raw_encode(cuda, dl, sym, -64, count=count - 8, end0=count - 8)[0] == -1          # count % W != 0
    assert _raw_encode(cuda, dl, sym, -W, count=count - 8, end0=count - 8)[0] == 0            # (the same count in whole rounds of 8 is served)
    assert _raw_encode(cuda, dl, sym, -W, end0=count - W)[0] == -1            # ends[0] != count
    assert _raw_encode(cuda, dl, sym, -W, end0=count + W)[0] == -1
    bad = sym.copy()
    k = int(np.flatnonzero(sym[1] >= 0)[5])
    for v in (L_ENC, -2):
        bad[1, k] = v
        rc, tails, status = _raw_encode(cuda, dl, bad, -W)
        assert rc == 0 and status == [0, 3] and tails[1] == b''


# ---- the decoder through the ABI --------------------------------------------------------------------------------------------------------

def _raw_rans(cuda, pred, volumes, th, tw, W, K, fill, want_syms=True, want_q=True, flags=None, model=None):
    """ic_pc_decode_tiles_batch_channels_f32 with IC_PC_DECODE_RANS(W) (or `flags`) on fenced buffers.  volumes: [(streams,
    first_syms, (C,h,w))].  Two runs: workspace and the fences of the byte input 0xFF, then 0x00; the outputs must be bit-identical.
    -> (rc, [symbols per volume] or None, [q per volume] or None, status list)"""
    from imgcomp_cvpr_amd import _lib, codec
    model = pred if model is None else model
    if flags is None:
        flags = _lib.PC_DECODE_RANS(W)
    tiles, blobs, pos = [], [], 0
    for n, (streams, firsts, (C, h, w)) in enumerate(volumes):
        for t, (y0, x0, a, b) in enumerate(codec.tile_grid(h, w, th, tw)):
            tiles.append((y0, x0, a, b, pos, len(streams[t]), firsts[t], n))
            blobs.append(bytes(streams[t]))
            pos += len(streams[t])
    shapes = [s for _, _, s in volumes]
    C = shapes[0][0]
    table = _lib.tile_table(tiles)
    vtable, offs, total = _lib.packed_volume_table(shapes)
    data = fenced(torch.frombuffer(bytearray(b''.join(blobs)) or bytearray(1), dtype=torch.uint8), torch.uint8, cuda, IN_FENCE, 'streams')
    need = int(_lib.lib.ic_pc_decode_tiles_batch_workspace_bytes(C, max(t[2] for t in tiles), max(t[3] for t in tiles), len(tiles),
                                                                 len(volumes), model.pc._k))
    centers = fenced(model.centers.contiguous().float(), torch.float32, cuda, IN_FENCE, 'centres')
    runs = []
    for byte in (IN_FENCE, ZERO_FENCE):
        refence(data, byte)
        sym = fenced((total,), torch.int64, cuda, OUT_FENCE, 'symbols') if want_syms else None
        q = fenced((total,), torch.float32, cuda, OUT_FENCE, 'q') if want_q else None
        status = fenced((len(tiles),), torch.int32, cuda, OUT_FENCE, 'status')
        ws = poison(fenced((need,), torch.uint8, cuda, OUT_FENCE, 'workspace'), byte)
        before = snapshot(sym, q, status, ws)
        rc = _lib.lib.ic_pc_decode_tiles_batch_channels_f32(
            _lib.ptr(data), pos, table, len(tiles), vtable, len(volumes), model.pc._tab, _lib.ptr(centers), model.pc._k, model.pc.L,
            model.freqs_resolution, _lib.ptr(sym), _lib.ptr(q), _lib.ptr(status), C, _lib.ptr(ws), need, int(flags),
            _lib.current_stream(cuda), int(K), int(fill))
        torch.cuda.synchronize()
        check_fences(data, centers, sym, q, status, ws)
        if rc != 0:
            unchanged(before, sym, q, status, ws)                            # a refused call wrote nothing
            return rc, None, None, None
        runs.append((None if sym is None else sym.clone(), None if q is None else q.clone(), status.tolist()))
    (s0, q0, st0), (s1, q1, st1) = runs
    assert st0 == st1 and (s0 is None or torch.equal(s0, s1)) and (q0 is None or torch.equal(q0.view(torch.int32), q1.view(torch.int32))), \
        'the outputs depend on what the workspace held'
    cut = lambda buf: [buf[o:o + c * h * w].view(c, h, w) for (c, h, w), o in zip(shapes, offs)]
    if want_syms and want_q:
        for s, qq in zip(cut(s0), cut(q0)):
            assert int(s.min()) >= 0 and int(s.max()) < model.pc.L             # whatever the bytes and the status are
            assert torch.equal(qq, model.centers.contiguous().float()[s]), 'q is not centers[symbols], bit for bit'
    return rc, [s.cpu().numpy() for s in cut(s0)] if want_syms else None, cut(q0) if want_q else None, st0


def _tile_freqs(pred, tile_sym):
    C, a, b = tile_sym.shape
    return pred.get_all(pred.pad_symbols_volume(tile_sym))[1].reshape(C * a * b, -1)


def _rule_stream(pred, tile_sym, W):
    """the rule's bytes of one tile over the device's tables of its true symbols"""
    C, a, b = tile_sym.shape
    rows, flat = _tile_freqs(pred, tile_sym), tile_sym.reshape(-1)
    rounds = [i for row in rr.rounds(C, a, b, W) for i in row]
    data, st = rr.encode([rows[max(i, 0)].tolist() for i in rounds], [int(flat[i]) if i >= 0 else -1 for i in rounds], W)
    assert st == 0
    return data


def _coded(pred, sym, th, tw, W):
    coded = pred.encode_tiles(sym, th, tw, order='rans', lanes=W)
    return [b for b, _ in coded], [f for _, f in coded], tuple(sym.shape)


@pytest.mark.parametrize('shape,W', CASES, ids=IDS)
def test_one_tile_round_trip(cuda, pred, shape, W):
    from imgcomp_cvpr_amd import _lib, codec
    assert _lib.PC_DECODE_RANS(W) == W << 16
    C, h, w = shape
    fill, L = pred.conceal_fallback(), pred.pc.L
    sym = np.random.RandomState(C + h + W).randint(0, L, size=shape).astype(np.int64)
    streams, firsts, _ = vol = _coded(pred, sym, h, w, W)
    assert streams == [_rule_stream(pred, sym, W)] and firsts == [int(sym[0, 0, 0])]     # the surface function returns the rule's bytes
    assert pred.encode_stream(sym, order='rans', lanes=W) == (streams[0], firsts[0])
    if shape == (1, 1, 1):
        assert streams[0] == struct.pack('<{}I'.format(W), *([65536] * W))
    rc, got, q, status = _raw_rans(cuda, pred, [vol], h, w, W, C, fill)
    assert rc == 0 and status == [0], (rc, status)
    assert np.array_equal(got[0], sym)
    for K in sorted(set((1, max(1, C // 2), C - 1)) - {0, C}):               # channels = K: preview_symbols of the full decode
        rc, gk, _, status = _raw_rans(cuda, pred, [vol], h, w, W, K, fill)
        assert rc == 0 and status == [0] and np.array_equal(gk[0], codec.preview_symbols(sym, K, fill)), K
    both = pred.decode_tiles_batch([vol], h, w, want='both', order='rans', lanes=W)
    assert np.array_equal(both[0][1].cpu().numpy(), sym) and torch.equal(both[0][0], q[0])
    assert np.array_equal(pred.decode_tiles(streams, firsts, shape, h, w, order='rans', lanes=W), sym)
    # the end check: a word too few, a word too many
    if shape != (1, 1, 1):
        for damaged in (streams[0][:-2], streams[0] + b'\x00\x00'):
            rc, _, _, status = _raw_rans(cuda, pred, [([damaged], firsts, shape)], h, w, W, C, fill)
            assert rc == 0 and status == [4]
        with pytest.raises(ValueError, match=r"does not end where the coders' run ends.*status 4; volume 0, tile 0"):
            pred.decode_tiles_batch([([streams[0] + b'\x00\x00'], firsts, shape)], h, w, order='rans', lanes=W)


@pytest.mark.parametrize('W', (8, 64))
def test_ragged_grid_and_two_volumes(cuda, pred, W):
    from imgcomp_cvpr_amd import codec
    fill, L = pred.conceal_fallback(), pred.pc.L
    rs = np.random.RandomState(W)
    a, b = rs.randint(0, L, size=(4, 10, 11)).astype(np.int64), rs.randint(0, L, size=(4, 5, 7)).astype(np.int64)
    grid = codec.tile_grid(10, 11, 4, 4)
    assert sorted(set(g[2:] for g in grid)) == [(2, 3), (2, 4), (4, 3), (4, 4)]
    va, vb = _coded(pred, a, 4, 4, W), _coded(pred, b, 4, 4, W)
    for t, (y0, x0, p, r) in enumerate(grid):
        assert va[0][t] == _rule_stream(pred, a[:, y0:y0 + p, x0:x0 + r], W), t
    assert pred.encode_tiles_batch([a, b], 4, 4, order='rans', lanes=W) == [list(zip(va[0], va[1])), list(zip(vb[0], vb[1]))]
    rc, got, q, status = _raw_rans(cuda, pred, [va, vb], 4, 4, W, 4, fill)
    assert rc == 0 and status == [0] * (len(grid) + 4)
    assert np.array_equal(got[0], a) and np.array_equal(got[1], b)
    rc, got, _, status = _raw_rans(cuda, pred, [va, vb], 4, 4, W, 2, fill)
    assert rc == 0 and np.array_equal(got[0], codec.preview_symbols(a, 2, fill)) and np.array_equal(got[1], codec.preview_symbols(b, 2, fill))
    rc, none, q_only, _ = _raw_rans(cuda, pred, [va, vb], 4, 4, W, 4, fill, want_syms=False)
    assert rc == 0 and none is None and torch.equal(q_only[0], q[0]) and torch.equal(q_only[1], q[1])
    rc, s_only, none, _ = _raw_rans(cuda, pred, [va, vb], 4, 4, W, 4, fill, want_q=False)
    assert rc == 0 and none is None and np.array_equal(s_only[0], a)
    res = pred.decode_tiles_batch([va, vb], 4, 4, want='symbols', order='rans', lanes=W)
    assert np.array_equal(res[0].cpu().numpy(), a) and np.array_equal(res[1].cpu().numpy(), b)


def test_flag_conflicts_are_unsupported_and_write_nothing(cuda, pred, configs):
    from imgcomp_cvpr_amd import _lib, config_parser as cp, weights as Wt
    shape, W = (4, 5, 7), 8
    fill = pred.conceal_fallback()
    sym = np.random.RandomState(1).randint(0, pred.pc.L, size=shape).astype(np.int64)
    vol = _coded(pred, sym, 5, 7, W)
    R, WF = _lib.PC_DECODE_RANS(W), _lib.PC_DECODE_WAVEFRONT
    assert _raw_rans(cuda, pred, [vol], 5, 7, W, 4, fill)[0] == 0
    for flags in (R | WF, R | _lib.PC_DECODE_DEPTH(2), R | WF | _lib.PC_DECODE_DEPTH(2), R | _lib.PC_DECODE_RECOMPUTE, R | _lib.PC_DECODE_PER_LAYER,
                  _lib.PC_DECODE_RANS(12), _lib.PC_DECODE_RANS(4), _lib.PC_DECODE_RANS(128), _lib.PC_DECODE_RANS(255), R | 0x1000000):
        assert _raw_rans(cuda, pred, [vol], 5, 7, W, 4, fill, flags=flags)[0] == -2, hex(flags)
    pc64, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow_64'))
    pred64 = _load(cuda, configs[0], pc64, Wt.synthetic_weights(configs[0], pc64), 1e9)
    assert _raw_rans(cuda, pred, [vol], 5, 7, W, 4, fill, model=pred64)[0] == -2
    with pytest.raises(ValueError, match='k = 24, this one has k = 64'):
        pred64.decode_tiles_batch([vol], 5, 7, order='rans', lanes=W)

    # the other entries, each with arguments it would otherwise serve
    lib, ptr = _lib.lib, _lib.ptr
    C, h, w = shape
    streams, firsts, _ = vol
    tiles = [(0, 0, h, w, 0, len(streams[0]), firsts[0], 0)]
    table, nt, pos = _lib.tile_table(tiles), 1, len(streams[0])
    vtable, _, total = _lib.packed_volume_table([shape])
    data = fenced(torch.frombuffer(bytearray(streams[0]), dtype=torch.uint8), torch.uint8, cuda, IN_FENCE, 'streams')
    centers = fenced(pred.centers.contiguous().float(), torch.float32, cuda, IN_FENCE, 'centres')
    ends = (ctypes.c_int * 1)(C)
    segs = _lib.seg_table([(0, pos)])
    limits, zeros = (ctypes.c_int * nt)(C), (ctypes.c_int * nt)(0)
    k, Lm, res, tab, stream = pred.pc._k, pred.pc.L, pred.freqs_resolution, pred.pc._tab, _lib.current_stream(cuda)

    def refused(name, need, call):
        out = fenced((total,), torch.int64, cuda, OUT_FENCE, name + ' symbols')
        q = fenced((total,), torch.float32, cuda, OUT_FENCE, name + ' q')
        status = fenced((nt,), torch.int32, cuda, OUT_FENCE, name + ' status')
        ws = poison(fenced((int(need),), torch.uint8, cuda, OUT_FENCE, name + ' workspace'), 0xFF)
        before = snapshot(out, q, status, ws)
        for flags in (R, R | WF):
            rc = call(out, q, status, ws, int(need), flags)
            torch.cuda.synchronize()
            assert rc == -2, (name, hex(flags), rc)
            check_fences(data, centers, out, q, status, ws)
            unchanged(before, out, q, status, ws)

    batch = lambda out, q, status, ws, need, flags: (ptr(data), pos, table, nt, vtable, 1, tab, ptr(centers), k, Lm, res, ptr(out), ptr(q),
                                                      ptr(status), C, ptr(ws), need, flags, stream)
    refused('ic_pc_decode_f32', lib.ic_pc_decode_workspace_bytes(C, h, w, k),
            lambda out, q, status, ws, need, flags: lib.ic_pc_decode_f32(ptr(data), pos, 0, tab, ptr(centers), k, Lm, res, ptr(out), ptr(status),
                                                                         C, h, w, ptr(ws), need, flags, stream))
    refused('ic_pc_decode_channels_f32', lib.ic_pc_decode_workspace_bytes(C, h, w, k),
            lambda out, q, status, ws, need, flags: lib.ic_pc_decode_channels_f32(ptr(data), pos, 0, tab, ptr(centers), k, Lm, res, ptr(out),
                                                                                  ptr(status), C, h, w, ptr(ws), need, flags, stream, C, fill))
    refused('ic_pc_decode_tiles_f32', lib.ic_pc_decode_tiles_workspace_bytes(C, h, w, nt, k),
            lambda out, q, status, ws, need, flags: lib.ic_pc_decode_tiles_f32(ptr(data), pos, table, nt, tab, ptr(centers), k, Lm, res, ptr(out),
                                                                               ptr(status), C, h, w, ptr(ws), need, flags, stream))
    refused('ic_pc_decode_tiles_batch_f32', lib.ic_pc_decode_tiles_batch_workspace_bytes(C, h, w, nt, 1, k),
            lambda *a: lib.ic_pc_decode_tiles_batch_f32(*batch(*a)))
    for kind in ('layers', 'fronts'):
        need = getattr(lib, 'ic_pc_decode_tiles_batch_{}_workspace_bytes'.format(kind))(C, h, w, nt, 1, k, 1)
        refused(kind, need, lambda *a: getattr(lib, 'ic_pc_decode_tiles_batch_{}_f32'.format(kind))(*(batch(*a) + (C, fill, ends, 1, segs))))
        need = getattr(lib, 'ic_pc_decode_tiles_batch_{}_pertile_workspace_bytes'.format(kind))(C, h, w, nt, 1, k, 1)
        refused(kind + ' pertile', need,
                lambda *a: getattr(lib, 'ic_pc_decode_tiles_batch_{}_pertile_f32'.format(kind))(*(batch(*a) + (limits, fill, ends, 1, segs))))
        need = getattr(lib, 'ic_pc_decode_tiles_batch_{}_resume_workspace_bytes'.format(kind))(C, h, w, nt, 1, k, 1)
        refused(kind + ' resume', need,
                lambda *a: getattr(lib, 'ic_pc_decode_tiles_batch_{}_resume_f32'.format(kind))(*(batch(*a) + (zeros, limits, fill, ends, 1, segs))))

    # the Python layers say it in words
    for kw, why in ((dict(order='rans', lanes=12), 'W one of'), (dict(order='rans', lanes=W, conceal=True), 'conceal'),
                    (dict(order='rans', lanes=W, depth_block=2), "needs order='wavefront'|depth_block"),
                    (dict(order='rans', lanes=W, front_ends=[C]), 'front_ends'), (dict(order='wavefront', lanes=W), "order='rans'")):
        with pytest.raises(ValueError, match=why):
            pred.decode_tiles_batch([vol], 5, 7, **kw)
    for kw, why in ((dict(order='rans', lanes=12), 'W one of'), (dict(order='rans', lanes=W, layer_ends=[2, 4]), 'seg_ends'),
                    (dict(order='rans', lanes=W, front_ends=[4]), 'front_ends'), (dict(order='raster', lanes=W), "order='rans'")):
        with pytest.raises(ValueError, match=why):
            pred.encode_tiles(sym, 5, 7, **kw)


# ---- hard tables and byte strings no encoder wrote: a constant table, so the rule decodes without the network ---------------------

HARD = {
    'floor rows': ([0.0, 20.0, 20.0, 20.0, 20.0, 20.0], 1e9),
    'floor at the top': ([20.0, 20.0, 20.0, 20.0, 20.0, 0.0], 1e9),
    'one large entry': ([30.0, 0.0, 0.0, 0.0, 0.0, 0.0], 1e9),
    'L = 2': ([0.0, 3.0], 1e9),
    'L = 16': ([float(j % 5) for j in range(16)], 1e9),
}


def _const_decode(table, data, shape, W, first, fill, channels=None):
    """the rule decoder of a tile whose table is `table` at every position -> ((C,h,w) symbols as the entry returns them, status)"""
    C, h, w = shape
    out = np.full(C * h * w, fill, np.int64)
    out[0] = first
    stop = None if channels is None or channels == C else rr.preview_rounds(C, h, w, W, channels)
    st = rr.decode(data, rr.rounds(C, h, w, W), W, lambda o, i: table, out, stop=stop)
    out = out.reshape(shape)
    if stop is not None:
        out[channels:] = fill
    return out, st


@pytest.mark.parametrize('name', sorted(HARD))
def test_hard_tables(cuda, name):
    bias, resolution = HARD[name]
    model, table = _model(cuda, bias, resolution=resolution)
    L, fill = len(bias), model.conceal_fallback()
    print(name, table, rr.table(table))
    if 'floor' in name:
        assert min(rr.table(table)) == 1 and min(table) == 1
    for shape, W in (((4, 5, 7), 8), ((4, 5, 7), 64), ((3, 1, 9), 16)):
        rs = np.random.RandomState(len(name) + W)
        for kind in ('uniform', 'by the table', 'the rarest'):
            if kind == 'uniform':
                sym = rs.randint(0, L, size=shape).astype(np.int64)
            elif kind == 'by the table':
                sym = rs.choice(L, size=shape, p=np.array(table, float) / sum(table)).astype(np.int64)
            else:
                sym = np.full(shape, int(np.argmin(table)), np.int64)
            n = sym.size
            rounds = [i for row in rr.rounds(*(shape + (W,))) for i in row]
            want, st = rr.encode([table] * len(rounds), [int(sym.reshape(-1)[i]) if i >= 0 else -1 for i in rounds], W)
            assert st == 0
            streams, firsts, _ = vol = _coded(model, sym, shape[1], shape[2], W)
            assert streams == [want], (name, shape, W, kind)
            rc, got, _, status = _raw_rans(cuda, model, [vol], shape[1], shape[2], W, shape[0], fill)
            assert rc == 0 and status == [0] and np.array_equal(got[0], sym), (name, shape, W, kind)
            ref, st = _const_decode(table, want, shape, W, firsts[0], fill)
            assert st == 0 and np.array_equal(ref, sym) and n == sym.size


def test_a_total_over_the_limit_is_status_1_on_both_sides(cuda):
    """the smallest total above 2^30 + 2 that a constant bias row reaches: the resolution is a float32 (steps of 64 .. 128 here) and
    six equal frequencies move the total in steps of 96, so it is 2^30 + 2 + 30, not + 1 (the host coder's test has + 1 exactly);
    beside it the nearest total within the limit, on which both sides work"""
    from tests.test_gpu_codec_decoder import _device_tables
    from tests.util import dev
    L, shape, W = 6, (4, 5, 7), 8
    bias = [0.0] * L
    # the resolution at which the bias row's total is one over 2^30 + 2, and the one below it at which it is within: found on the device
    found = {}
    for res in (1.0737418e9 + 64.0 * k for k in range(-40, 41)):
        res = float(np.float32(res))
        total = int(_device_tables(dev(np.asarray(bias, np.float32)[None], cuda), res)[0].sum())
        found.setdefault(total > rr.MAX_TOTAL, (res, total))
    assert True in found and False in found, found
    sym = np.random.RandomState(3).randint(0, L, size=shape).astype(np.int64)
    model, table = _model(cuda, bias, resolution=found[True][0])
    assert sum(table) > rr.MAX_TOTAL
    print('over the limit: resolution {}, total {} = 2^30 + 2 + {}'.format(found[True][0], sum(table), sum(table) - rr.MAX_TOTAL))
    with pytest.raises(ValueError, match='total is too large'):
        model.encode_tiles(sym, 5, 7, order='rans', lanes=W)
    rounds = [i for row in rr.rounds(4, 5, 7, W) for i in row]
    assert rr.encode([table] * len(rounds), [int(sym.reshape(-1)[i]) if i >= 0 else -1 for i in rounds], W) == (None, 1)
    ok_model, ok_table = _model(cuda, bias, resolution=found[False][0])
    vol = _coded(ok_model, sym, 5, 7, W)
    fill = model.conceal_fallback()
    rc, got, _, status = _raw_rans(cuda, model, [vol], 5, 7, W, 4, fill)
    assert rc == 0 and status[0] & 1 and _const_decode(table, vol[0][0], shape, W, vol[1][0], fill)[1] & 1
    with pytest.raises(ValueError, match='total is too large'):
        model.decode_tiles_batch([vol], 5, 7, order='rans', lanes=W)
    rc, got, _, status = _raw_rans(cuda, ok_model, [vol], 5, 7, W, 4, fill)
    assert rc == 0 and status == [0] and np.array_equal(got[0], sym)


@pytest.mark.parametrize('W', (8, 64))
def test_byte_strings_no_encoder_wrote(cuda, W):
    """equalities with the rule decoder, which reads zeros past the end of any string: symbols and status"""
    shape = (4, 5, 7)
    model, table = _model(cuda, [0.0, 1.0, 2.0, 3.0, 2.0, 1.0])
    fill, L = model.conceal_fallback(), 6
    rs = np.random.RandomState(W)
    sym = rs.choice(L, size=shape, p=np.array(table, float) / sum(table)).astype(np.int64)
    streams, firsts, _ = _coded(model, sym, 5, 7, W)
    real, first = streams[0], firsts[0]
    strings = [b'', b'\x00', b'\xff', real, real + b'\x00\x00', real + b'\x07']
    strings += [real[:n] for n in range(1, 4 * W + 9)]
    strings += [bytes(rs.randint(0, 256, size=n).astype(np.uint8)) for n in (3, 4 * W - 1, 4 * W, 4 * W + 1, 4 * W + 40, 1000)]
    strings += [struct.pack('<{}I'.format(W), *([v] * W)) + real[4 * W:] for v in (0, 0xffffffff)]
    strings += [struct.pack('<{}I'.format(W), *([65536] * W)) + bytes([255]) * 300]
    # all of them as the tiles of ONE call: a volume of len(strings) tiles side by side
    n = len(strings)
    vol = (strings, [first] * n, (4, 5, 7 * n))
    rc, got, _, status = _raw_rans(cuda, model, [vol], 5, 7, W, 4, fill)
    assert rc == 0
    for t, s in enumerate(strings):
        ref, st = _const_decode(table, s, shape, W, first, fill)
        assert status[t] == st, (t, len(s), status[t], st)
        assert np.array_equal(got[0][:, :, 7 * t:7 * t + 7], ref), (t, len(s))
    assert status[3] == 0 and status[0] == 4 and status[4] == 4
    rc, got, _, status = _raw_rans(cuda, model, [vol], 5, 7, W, 2, fill)        # a preview is not end-checked
    assert rc == 0 and status == [0] * n
    for t, s in enumerate(strings):
        assert np.array_equal(got[0][:, :, 7 * t:7 * t + 7], _const_decode(table, s, shape, W, first, fill, channels=2)[0]), (t, len(s))


# ---- files ------------------------------------------------------------------------------------------------------------------------------

def _image(H, W_, seed=9):
    from imgcomp_cvpr_amd import weights as Wt
    return np.ascontiguousarray(Wt.synthetic_image((1, 3, H, W_), 'natural', seed=seed)[0].transpose(1, 2, 0))


@pytest.fixture(scope='module')
def cdc(cuda, configs, syn_weights):
    from imgcomp_cvpr_amd import codec
    return codec.Codec(configs[0], configs[1], syn_weights, cuda)


def _as(c, version, fn, W='default'):
    """run fn() with the Codec writing format 12 (W coders) or format 5, tiles of 8 x 8 cells (--tile 64)"""
    c.tile, c.order, c.rans = (8, 8), ('wavefront' if version == 5 else 'raster'), (W if version == 12 else None)
    try:
        return fn()
    finally:
        c.tile, c.order, c.rans = None, 'raster', None


@pytest.fixture(scope='module', params=[(128, 160), (100, 150)], ids=['128x160', '100x150'])
def files(request, cdc):
    H, W_ = request.param
    img = _image(H, W_, seed=H)
    enc, size = cdc.encode_symbols(img)
    sym = enc.symbols[0].cpu().numpy()
    return dict(img=img, sym=sym, H=H, W=W_, twelve=_as(cdc, 12, lambda: cdc.compress(img)), five=_as(cdc, 5, lambda: cdc.compress(img)))


def test_file_symbols_pixels_and_bytes(cdc, files):
    from imgcomp_cvpr_amd import codec
    f = files
    c = codec.parse_container(f['twelve'])
    assert isinstance(c, codec.RansContainer) and c.version == 12 and c.lanes == codec.DEFAULT_RANS_LANES and (c.th, c.tw) == (8, 8)
    print('{} x {}: format 12 {} bytes, format 5 {} bytes'.format(f['H'], f['W'], len(f['twelve']), len(f['five'])))
    got, _ = cdc.decode_symbols(f['twelve'])
    assert np.array_equal(got, f['sym'])
    assert np.array_equal(cdc.decompress(f['twelve']), cdc.decompress(f['five']))            # the pixels of the format-5 file
    streams, firsts = [], []
    for y0, x0, a, b in codec.tile_grid(c.h, c.w, 8, 8):
        ts = f['sym'][:, y0:y0 + a, x0:x0 + b]
        streams.append(_rule_stream(cdc.pred, ts, c.lanes))
        firsts.append(int(ts[0, 0, 0]))
    assert f['twelve'] == codec.build_rans_container(cdc.ae_name, cdc.pc_name, f['H'], f['W'], cdc.C, c.h, c.w, cdc.L, cdc.pred.freqs_resolution,
                                                     cdc.fingerprint, 8, 8, c.lanes, firsts, streams)
    fill = cdc.pred.conceal_fallback()
    assert np.array_equal(cdc.decompress(f['twelve'], channels=4), cdc.decompress(f['five'], channels=4))
    assert np.array_equal(cdc.decode_symbols(f['twelve'], channels=4)[0], codec.preview_symbols(f['sym'], 4, fill))
    ok, text = codec.verify_file(f['twelve'])
    assert ok and 'W = 16 coders per tile' in text and 'bytes of coder states' in codec.info_file(f['twelve'])
    assert _as(cdc, 12, cdc.written_version) == 12 and _as(cdc, 5, cdc.written_version) == 5
    other = _as(cdc, 12, lambda: cdc.compress(f['img']), W=64)               # another W: other bytes, the same symbols
    assert codec.parse_container(other).lanes == 64 and other != f['twelve'] and np.array_equal(cdc.decode_symbols(other)[0], f['sym'])


def test_transcode_both_ways(cdc, files):
    f = files
    assert _as(cdc, 12, lambda: cdc.transcode(f['five'])) == f['twelve']
    assert _as(cdc, 5, lambda: cdc.transcode(f['twelve'])) == f['five']
    assert _as(cdc, 12, lambda: cdc.transcode_many([f['five'], f['twelve']])) == [f['twelve'], f['twelve']]


def test_many_region_measure(cdc, files):
    f = files
    other = _image(72, 88, seed=3)
    twelves = _as(cdc, 12, lambda: cdc.compress_many([f['img'], other]))
    assert twelves[0] == f['twelve'] and twelves[1] == _as(cdc, 12, lambda: cdc.compress(other))
    fives = [f['five'], _as(cdc, 5, lambda: cdc.compress(other))]
    many = cdc.decompress_many(twelves + fives)
    singles = [cdc.decompress(d) for d in twelves + fives]
    assert all(np.array_equal(a, b) for a, b in zip(many, singles))
    assert np.array_equal(many[0], many[2]) and np.array_equal(many[1], many[3])
    full = singles[0]
    x, y, rw, rh = rect = (f['W'] - 30, f['H'] - 20, 30, 20)                  # a corner
    assert np.array_equal(cdc.decompress_region(f['twelve'], rect), full[y:y + rh, x:x + rw])
    assert np.array_equal(cdc.decompress_region(f['twelve'], (0, 0, 24, 16)), full[:16, :24])
    a, b = cdc.measure(f['img'], f['twelve']), cdc.measure(f['img'], f['five'])
    assert a.bytes == len(f['twelve']) and b.bytes == len(f['five'])
    assert a._replace(bytes=0, bpp=0.0) == b._replace(bytes=0, bpp=0.0)


def test_the_other_readers_refuse(cdc, files):
    twelve = files['twelve']
    why = r'format version 12 \(lane-parallel rANS tiles\) is not read by'
    for call in (cdc.salvage, cdc.decompress_partial, cdc.recover, cdc.repair, lambda d: cdc.open_stream().feed(d),
                 lambda d: cdc.open_stream(fronts=True).feed(d)):
        with pytest.raises(ValueError, match=why):
            call(twelve)
    from imgcomp_cvpr_amd import codec
    for kw, why in ((dict(rans=16), 'needs a tile extent'), (dict(rans=12, tile=(8, 8)), 'W one of'),
                    (dict(rans=16, tile=(8, 8), checked=True), 'checked=True'), (dict(rans=16, tile=(8, 8), depth_block=4), 'depth_block')):
        with pytest.raises(ValueError, match=why):
            codec.Codec._check_rans(**dict(dict(tile=None, checked=False, order='raster', layers=None, front_layers=None, depth_block=None), **kw))
