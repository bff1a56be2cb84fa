"""-m gpu: depth-mapped wavefront tiles (container format 10).  The encoder's skip marker (IC_PC_ENCODE_SKIP) against the host coder
over the kept symbols; the decoder's depth flag (IC_PC_DECODE_DEPTH) against the planted symbols, the preview rule and the format-5
decoder; then whole files against format 5.  Every device buffer comes from tests.fenced.fenced(), workspaces have exactly the
queried size and are handed over dirty (0xFF, then 0x00; the outputs must be bit-identical), every comparison is an equality."""
import ctypes

import numpy as np
import pytest
import torch

from tests import codec_cases as cc
from tests import depth_rule as dr
from tests.fenced import OUT_FENCE, ZERO_FENCE, IN_FENCE, check_fences, fenced, poison, refence, snapshot, unchanged
from tests.test_gpu_codec_decoder import _load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pred(cuda, configs, syn_weights):
    return _load(cuda, configs[0], configs[1], syn_weights, 1e9)


# ---- the encoder through the ABI: symbols equal to IC_PC_ENCODE_SKIP are stepped over ------------------------------------------

N_ENC, COUNT, L_ENC = 2, 200, 6


def _enc_inputs(cuda):
    from imgcomp_cvpr_amd import _lib
    rs = np.random.RandomState(11)
    logits = (rs.randn(N_ENC, COUNT, L_ENC) * 3.0).astype(np.float32)
    sym = rs.randint(0, L_ENC, size=(N_ENC, COUNT)).astype(np.int64)
    dl = fenced(logits, torch.float32, cuda, IN_FENCE, 'logits')
    freqs = fenced((N_ENC * COUNT, L_ENC), torch.int64, cuda, OUT_FENCE, 'freqs')
    pr = fenced((N_ENC * COUNT, L_ENC), torch.float32, cuda, OUT_FENCE, 'pr')
    rc = _lib.lib.ic_pc_logits_to_freqs_f32(_lib.ptr(dl), N_ENC * COUNT, L_ENC, 1e9, _lib.ptr(freqs), _lib.ptr(pr), _lib.current_stream(cuda))
    torch.cuda.synchronize()
    assert rc == 0
    check_fences(dl, freqs, pr)
    return dl, sym, freqs.cpu().numpy().reshape(N_ENC, COUNT, L_ENC)


def _raw_encode(cuda, dl, coded, ends=None, L=L_ENC):
    """ic_pc_encode_f32 (ends None) or ic_pc_encode_segments_f32 on fenced buffers, the integer input once between fences of 0xFF
    and once of 0x00 -> (rc, [[bytes per segment] per row], status rows)"""
    from imgcomp_cvpr_amd import _lib
    G = 1 if ends is None else len(ends)
    cap = int(_lib.lib.ic_pc_encode_capacity_bytes(COUNT))
    ds = fenced(coded, torch.int64, cuda, IN_FENCE, 'symbols')
    results = []
    for fill in (IN_FENCE, ZERO_FENCE):
        refence(ds, fill)
        out = fenced((N_ENC * G * cap,), torch.uint8, cuda, OUT_FENCE, 'bitstream')
        nbytes = fenced((N_ENC * G,), torch.int64, cuda, OUT_FENCE, 'nbytes')
        status = fenced((N_ENC * G,), torch.int32, cuda, OUT_FENCE, 'status')
        if ends is None:
            rc = _lib.lib.ic_pc_encode_f32(_lib.ptr(dl), _lib.ptr(ds), N_ENC, COUNT, L, 1e9, _lib.ptr(out), cap, _lib.ptr(nbytes),
                                           _lib.ptr(status), _lib.current_stream(cuda))
        else:
            host_ends = (ctypes.c_longlong * G)(*ends)
            rc = _lib.lib.ic_pc_encode_segments_f32(_lib.ptr(dl), _lib.ptr(ds), N_ENC, COUNT, L, 1e9, host_ends, G, _lib.ptr(out), cap,
                                                    _lib.ptr(nbytes), _lib.ptr(status), _lib.current_stream(cuda))
        torch.cuda.synchronize()
        check_fences(dl, ds, out, nbytes, status)
        assert rc == 0
        host, nb = out.view(N_ENC, G, cap).cpu().numpy(), nbytes.view(N_ENC, G).tolist()
        results.append(([[bytes(host[n, g, :nb[n][g]]) for g in range(G)] for n in range(N_ENC)], status.view(N_ENC, G).tolist()))
    assert results[0] == results[1], 'the result depends on what lies around the symbols'
    return results[0]


def _host_kept(sym_row, coded_row, freq_rows, a, b):
    """the host coder over the kept symbols of positions [max(1, a), b)"""
    idx = np.array([i for i in range(max(1, a), b) if coded_row[i] != -1], np.int64)
    return cc.host_encode(sym_row[idx], freq_rows[idx].reshape(len(idx), L_ENC))[0]


SKIPS = {
    'none': ([], []),
    'all': (range(COUNT), range(COUNT)),
    'around the chunk border': ([63, 64, 65], [64, 65, 66]),               # position 64 of the volume is lane 63 of the first chunk
    'the whole second chunk': (range(65, 129), range(64, 130)),
    'the last symbol': ([COUNT - 1], [COUNT - 2, COUNT - 1]),
    'every other one, and a run': (range(1, COUNT, 2), list(range(3, 40)) + list(range(100, 190, 3))),
    'the first coded one': ([1], [1, 2, 3]),
}


@pytest.fixture(scope='module')
def enc_inputs(cuda):
    return _enc_inputs(cuda)


@pytest.mark.parametrize('case', sorted(SKIPS))
def test_encoder_steps_over_skipped_symbols(cuda, enc_inputs, case):
    from imgcomp_cvpr_amd import _lib
    assert _lib.PC_ENCODE_SKIP == -1
    dl, sym, freqs = enc_inputs
    coded = sym.copy()
    for n in range(N_ENC):                                                   # two rows, two patterns
        coded[n, list(SKIPS[case][n])] = _lib.PC_ENCODE_SKIP
    streams, status = _raw_encode(cuda, dl, coded)
    assert status == [[0]] * N_ENC, (case, status)
    for n in range(N_ENC):
        assert streams[n][0] == _host_kept(sym[n], coded[n], freqs[n], 1, COUNT), (case, n)
    # the logits of a skipped position are not looked at: NaNs there change nothing
    holes = dl.clone()
    for n in range(N_ENC):
        holes[n, [i for i in SKIPS[case][n]]] = float('nan')
    assert _raw_encode(cuda, fenced(holes, torch.float32, cuda, IN_FENCE, 'logits with holes'), coded) == (streams, status), case
    if case == 'all':
        assert [s[0] for s in streams] == [b'\x80'] * N_ENC
    if case == 'none':                                                       # the bytes the entry has always written
        assert [s[0] for s in streams] == [cc.host_encode(sym[n, 1:], freqs[n, 1:])[0] for n in range(N_ENC)]


def test_encoder_other_symbols_out_of_range_stay_status_3(cuda, enc_inputs):
    dl, sym, freqs = enc_inputs
    for bad in (L_ENC, -2):
        coded = sym.copy()
        coded[0, 10:20] = -1
        coded[1, 70] = bad
        coded[1, 60:70] = -1
        streams, status = _raw_encode(cuda, dl, coded)
        assert status == [[0], [3]], (bad, status)
        assert streams[0][0] == _host_kept(sym[0], coded[0], freqs[0], 1, COUNT)


def test_encoder_segments_step_over_skipped_symbols(cuda, enc_inputs):
    dl, sym, freqs = enc_inputs
    coded = sym.copy()
    coded[0, list(range(40, 60)) + [129, 130, 199]] = -1
    coded[1, 50:130] = -1                                                    # a whole segment skipped: the one byte of an empty one
    ends = [50, 130, COUNT]
    streams, status = _raw_encode(cuda, dl, coded, ends)
    assert status == [[0, 0, 0]] * N_ENC
    for n in range(N_ENC):
        assert streams[n] == [_host_kept(sym[n], coded[n], freqs[n], a, b) for a, b in zip([0] + ends, ends)], n
    assert streams[1][1] == b'\x80'


# ---- the decoder through the ABI --------------------------------------------------------------------------------------------------

def _raw_depth(cuda, pred, volumes, th, tw, B, K, fill, want_syms=True, want_q=True, flags=None, entry='channels', model=None):
    """ic_pc_decode_tiles_batch_channels_f32 with IC_PC_DECODE_WAVEFRONT | IC_PC_DECODE_DEPTH(B) (or `flags`) on fenced buffers.
    volumes: [(streams, first_syms, (C,h,w))].  Two runs: workspace and the fences of the byte input 0xFF, then 0x00; the outputs
    must be bit-identical.  -> (rc, [symbols per volume] or None, [q per volume] or None, status list)"""
    from imgcomp_cvpr_amd import _lib, codec
    model = pred if model is None else model
    if flags is None:
        flags = _lib.PC_DECODE_WAVEFRONT | _lib.PC_DECODE_DEPTH(B)
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
    if want_syms and want_q and all(s == 0 for s in st0):
        for s, qq in zip(cut(s0), cut(q0)):
            assert int(s.min()) >= 0 and int(s.max()) < model.pc.L
            assert torch.equal(qq, model.centers.contiguous().float()[s]), 'q is not centers[symbols], bit for bit'
    return rc, [s.cpu().numpy() for s in cut(s0)] if want_syms else None, cut(q0) if want_q else None, st0


def _cell_depths(C, h, w, B, profile, seed):
    """(h, w) cell depths: blocks of B x B cells counted from the VOLUME's corner here -- the tiles cut them where they like"""
    rs = np.random.RandomState(seed)
    if profile == 'all dead':
        return np.zeros((h, w), int)
    if profile == 'all C':
        return np.full((h, w), C)
    blocks = rs.randint(0, C + 1, size=(-(-h // B), -(-w // B)))
    cells = np.repeat(np.repeat(blocks, B, 0), B, 1)[:h, :w].copy()
    if profile == 'dead first block':
        cells[:B, :B] = 0
        cells[-1, -1] = C
    return cells


def _coded_depth(pred, sym, th, tw, B):
    coded = pred.encode_tiles(sym, th, tw, order='wavefront', depth_block=B)
    return [b for b, _ in coded], [f for _, f in coded], tuple(sym.shape)


def _tile_freqs(pred, tile_sym):
    C, a, b = tile_sym.shape
    return pred.get_all(pred.pad_symbols_volume(tile_sym))[1].reshape(C, a, b, -1)


SHAPE, TILE = (5, 6, 7), (4, 5)


@pytest.mark.parametrize('profile', ['patches', 'dead first block', 'all dead', 'all C', 'one dead tile'])
@pytest.mark.parametrize('B', (1, 2, 3))
def test_decoder_depth_tiles(cuda, pred, B, profile):
    from imgcomp_cvpr_amd import codec
    C, h, w = SHAPE
    th, tw = TILE
    fill, L = pred.conceal_fallback(), pred.pc.L
    grid = codec.tile_grid(h, w, th, tw)
    assert sorted(set(g[2:] for g in grid)) == [(2, 2), (2, 5), (4, 2), (4, 5)]                 # four ragged shapes
    cells = _cell_depths(C, h, w, B, 'patches' if profile == 'one dead tile' else profile, seed=10 * B + len(profile))
    if profile == 'one dead tile':
        cells[:th, tw:] = 0                                                  # tile 1 wholly dead, the others not
        cells[0, 0] = C
    sym = dr.planted(SHAPE, fill, L, cells, seed=B)
    streams, firsts, _ = vol = _coded_depth(pred, sym, th, tw, B)
    # the encoder's Python layer: depth plane, then the host coder's bytes over the kept symbols and the device's tables
    for t, (y0, x0, a, b) in enumerate(grid):
        ts = sym[:, y0:y0 + a, x0:x0 + b]
        depth = dr.depth_plane(ts, fill, B)
        assert streams[t] == depth.tobytes() + dr.host_encode(ts, _tile_freqs(pred, ts), depth, B), (profile, B, t)
        assert firsts[t] == int(ts[0, 0, 0])
    if profile == 'one dead tile':
        assert streams[1] == bytes(len(streams[1]) - 1) + b'\x80'
    rc, got, q, status = _raw_depth(cuda, pred, [vol], th, tw, B, C, fill)
    assert rc == 0 and status == [0] * len(grid), (profile, B, rc, status)
    assert np.array_equal(got[0], sym), (profile, B)
    for K in (1, 3):                                                         # channels = K: the preview of the full decode
        rc, gk, _, status = _raw_depth(cuda, pred, [vol], th, tw, B, K, fill)
        assert rc == 0 and status == [0] * len(grid) and np.array_equal(gk[0], codec.preview_symbols(sym, K, fill)), (profile, B, K)
    # symbols = NULL and q = NULL
    rc, none, q_only, _ = _raw_depth(cuda, pred, [vol], th, tw, B, C, fill, want_syms=False)
    assert rc == 0 and none is None and torch.equal(q_only[0], q[0])
    rc, s_only, none, _ = _raw_depth(cuda, pred, [vol], th, tw, B, C, fill, want_q=False)
    assert rc == 0 and none is None and np.array_equal(s_only[0], sym)
    # the Python surface
    both = pred.decode_tiles_batch([vol], th, tw, want='both', order='wavefront', depth_block=B)
    assert np.array_equal(both[0][1].cpu().numpy(), sym) and torch.equal(both[0][0], q[0])
    assert np.array_equal(pred.decode_tiles_batch([vol], th, tw, want='symbols', order='wavefront', depth_block=B, channels=2)[0].cpu().numpy(),
                          codec.preview_symbols(sym, 2, fill))
    if profile == 'all C':                                                   # every position live: the symbols of the format-5 decoder
        five = pred.encode_tiles(sym, th, tw, order='wavefront')
        for t, (y0, x0, a, b) in enumerate(grid):
            assert streams[t][-(-a // B) * -(-b // B):] == five[t][0]        # and its bytes behind the plane
        ref = pred.decode_tiles_batch([([b for b, _ in five], [f for _, f in five], SHAPE)], th, tw, want='symbols', order='wavefront')[0]
        assert np.array_equal(got[0], ref.cpu().numpy())


def _candidates(S, C, h, w):
    """the kernel's candidates of front S (pc_front / pc_front_voxel): [(c, y, x) or None]"""
    cdiv = lambda n, k: 0 if n <= 0 else (n + k - 1) // k
    d_lo, d_hi = cdiv(S - (w - 1) - 2 * (h - 1), 4), min(C - 1, S >> 2)
    nd, iw = max(d_hi - d_lo + 1, 0), min(h, (w + 1) >> 1)
    out = []
    for e in range(nd * iw):
        d = d_lo + e // iw
        i = cdiv(S - 4 * d - (w - 1), 2) + e % iw
        j = S - 4 * d - 2 * i
        out.append((d, i, j) if i < h and j >= 0 else None)
    return out


BIG = (10, 14, 16)


@pytest.mark.parametrize('B', (2, 3))
def test_decoder_front_longer_than_a_chunk(cuda, pred, B):
    """one tile whose largest front has more than the 64 candidates the kernel takes at once, live and dead on both sides"""
    from imgcomp_cvpr_amd import codec
    C, h, w = BIG
    fill, L = pred.conceal_fallback(), pred.pc.L
    fronts = [_candidates(S, C, h, w) for S in range((w - 1) + 2 * (h - 1) + 4 * (C - 1) + 1)]
    assert sorted(p for f in fronts for p in f if p is not None) == sorted(dr.wavefront_positions(C, h, w))      # the model of the kernel's fronts
    longest = max(fronts, key=lambda f: sum(p is not None for p in f[64:]))  # the front with the most positions in its second chunk
    assert len(longest) > 64 and sum(p is not None for p in longest[64:]) >= 4
    for seed in range(64):                                                   # (host only) a profile that mixes both kinds on both sides
        cells = _cell_depths(C, h, w, B, 'patches', seed=seed)
        cells[-1, -1] = C                                                    # the sweep runs over all C channels
        sym = dr.planted(BIG, fill, L, cells, seed=20 + B)
        lv = dr.live(C, h, w, dr.depth_plane(sym, fill, B), B)
        if all(set(bool(lv[p]) for p in side if p is not None) == {True, False} for side in (longest[:64], longest[64:])):
            break
    for side in (longest[:64], longest[64:]):
        kinds = set(bool(lv[p]) for p in side if p is not None)
        assert kinds == {True, False}, 'live and dead slots on both sides of the chunk border'
    vol = _coded_depth(pred, sym, h, w, B)
    depth = dr.depth_plane(sym, fill, B)
    assert vol[0][0] == depth.tobytes() + dr.host_encode(sym, _tile_freqs(pred, sym), depth, B)
    rc, got, _, status = _raw_depth(cuda, pred, [vol], h, w, B, C, fill)
    assert rc == 0 and status == [0] and np.array_equal(got[0], sym)
    rc, got, _, status = _raw_depth(cuda, pred, [vol], h, w, B, 4, fill)
    assert rc == 0 and status == [0] and np.array_equal(got[0], codec.preview_symbols(sym, 4, fill))


def test_decoder_depth_255_and_no_coder_bytes(cuda, pred):
    """within defined behaviour: depths above C count as C, a coder part of no bytes reads as zeros"""
    from imgcomp_cvpr_amd import codec
    C, h, w = SHAPE
    th, tw = TILE
    fill, B = pred.conceal_fallback(), 2
    grid = codec.tile_grid(h, w, th, tw)
    streams = [bytes([255]) * (-(-a // B) * -(-b // B)) for _, _, a, b in grid]
    rc, got, q, status = _raw_depth(cuda, pred, [(streams, [1] * len(grid), SHAPE)], th, tw, B, C, fill)
    assert rc == 0 and status == [0] * len(grid)
    assert got[0].min() >= 0 and got[0].max() < pred.pc.L
    assert [int(got[0][0, y0, x0]) for y0, x0, _, _ in grid] == [1] * len(grid)     # live first positions: the uncoded first symbol
    # a stream shorter than its plane: status 2 for that tile, nothing of it decoded; the Python layer names the tile
    short = list(streams)
    short[2] = short[2][:-1]
    rc, _, _, status = _raw_depth(cuda, pred, [(short, [1] * len(grid), SHAPE)], th, tw, B, C, fill)
    assert rc == 0 and status == [0, 0, 2, 0]
    with pytest.raises(ValueError, match=r'stream shorter than its depth plane \(volume 0, tile 2'):
        pred.decode_tiles_batch([(short, [1] * len(grid), SHAPE)], th, tw, want='symbols', order='wavefront', depth_block=B)
    # the depth wins over the first symbol: a dead first block holds the fill
    dead = [bytes(len(s)) for s in streams]
    rc, got, _, status = _raw_depth(cuda, pred, [(dead, [(fill + 1) % pred.pc.L] * len(grid), SHAPE)], th, tw, B, C, fill)
    assert rc == 0 and status == [0] * len(grid) and (got[0] == fill).all()


def test_depth_flag_is_refused_everywhere_else(cuda, pred, configs):
    """IC_PC_DECODE_DEPTH on any other entry, without IC_PC_DECODE_WAVEFRONT, beside another flag or with k = 64: -2, nothing written"""
    from imgcomp_cvpr_amd import _lib, codec, config_parser as cp, weights as W
    lib, ptr = _lib.lib, _lib.ptr
    C, h, w = SHAPE
    th, tw = TILE
    fill, B = pred.conceal_fallback(), 2
    D, WF = _lib.PC_DECODE_DEPTH(B), _lib.PC_DECODE_WAVEFRONT
    assert D == 0x200 and _lib.PC_DECODE_DEPTH(255) == 0xff00
    sym = dr.planted(SHAPE, fill, pred.pc.L, _cell_depths(C, h, w, B, 'patches', 3), seed=3)
    vol = _coded_depth(pred, sym, th, tw, B)
    assert _raw_depth(cuda, pred, [vol], th, tw, B, C, fill)[0] == 0
    for flags in (D, D | WF | _lib.PC_DECODE_RECOMPUTE, D | _lib.PC_DECODE_PER_LAYER, D | WF | 0x10000):
        assert _raw_depth(cuda, pred, [vol], th, tw, B, C, fill, flags=flags)[0] == -2, hex(flags)
    pc64, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow_64'))
    pred64 = _load(cuda, configs[0], pc64, W.synthetic_weights(configs[0], pc64), 1e9)
    assert pred64.pc._k == 64
    assert _raw_depth(cuda, pred, [vol], th, tw, B, C, fill, model=pred64)[0] == -2
    with pytest.raises(ValueError, match='k = 24, this one has k = 64'):
        pred64.decode_tiles_batch([vol], th, tw, order='wavefront', depth_block=B)

    # the other entries, each with arguments it would otherwise serve
    grid = codec.tile_grid(h, w, th, tw)
    streams, firsts, _ = vol
    tiles, pos = [], 0
    for t, (y0, x0, a, b) in enumerate(grid):
        tiles.append((y0, x0, a, b, pos, len(streams[t]), firsts[t], 0))
        pos += len(streams[t])
    table, nt = _lib.tile_table(tiles), len(tiles)
    vtable, _, total = _lib.packed_volume_table([SHAPE])
    data = fenced(torch.frombuffer(bytearray(b''.join(streams)), dtype=torch.uint8), torch.uint8, cuda, IN_FENCE, 'streams')
    centers = fenced(pred.centers.contiguous().float(), torch.float32, cuda, IN_FENCE, 'centres')
    ends = (ctypes.c_int * 1)(C)
    segs = _lib.seg_table([(t[4], t[5]) for t in tiles])
    limits, zeros = (ctypes.c_int * nt)(*([C] * nt)), (ctypes.c_int * nt)(*([0] * nt))
    k, Lm, res, tab, stream = pred.pc._k, pred.pc.L, pred.freqs_resolution, pred.pc._tab, _lib.current_stream(cuda)

    def refused(name, need, call):
        out = fenced((total,), torch.int64, cuda, OUT_FENCE, name + ' symbols')
        q = fenced((total,), torch.float32, cuda, OUT_FENCE, name + ' q')
        status = fenced((nt,), torch.int32, cuda, OUT_FENCE, name + ' status')
        ws = poison(fenced((int(need),), torch.uint8, cuda, OUT_FENCE, name + ' workspace'), 0xFF)
        before = snapshot(out, q, status, ws)
        for flags in (D, D | WF):
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
    refused('ic_pc_decode_tiles_f32', lib.ic_pc_decode_tiles_workspace_bytes(C, th, tw, nt, k),
            lambda out, q, status, ws, need, flags: lib.ic_pc_decode_tiles_f32(ptr(data), pos, table, nt, tab, ptr(centers), k, Lm, res, ptr(out),
                                                                               ptr(status), C, h, w, ptr(ws), need, flags, stream))
    refused('ic_pc_decode_tiles_batch_f32', lib.ic_pc_decode_tiles_batch_workspace_bytes(C, th, tw, nt, 1, k),
            lambda *a: lib.ic_pc_decode_tiles_batch_f32(*batch(*a)))
    for kind in ('layers', 'fronts'):
        need = getattr(lib, 'ic_pc_decode_tiles_batch_{}_workspace_bytes'.format(kind))(C, th, tw, nt, 1, k, 1)
        refused(kind, need, lambda *a: getattr(lib, 'ic_pc_decode_tiles_batch_{}_f32'.format(kind))(*(batch(*a) + (C, fill, ends, 1, segs))))
        need = getattr(lib, 'ic_pc_decode_tiles_batch_{}_pertile_workspace_bytes'.format(kind))(C, th, tw, nt, 1, k, 1)
        refused(kind + ' pertile', need,
                lambda *a: getattr(lib, 'ic_pc_decode_tiles_batch_{}_pertile_f32'.format(kind))(*(batch(*a) + (limits, fill, ends, 1, segs))))
        need = getattr(lib, 'ic_pc_decode_tiles_batch_{}_resume_workspace_bytes'.format(kind))(C, th, tw, nt, 1, k, 1)
        refused(kind + ' resume', need,
                lambda *a: getattr(lib, 'ic_pc_decode_tiles_batch_{}_resume_f32'.format(kind))(*(batch(*a) + (zeros, limits, fill, ends, 1, segs))))

    # the Python layers say it in words
    for kw, why in ((dict(order='raster', depth_block=B), "needs order='wavefront'"), (dict(order='wavefront', depth_block=0), '1 .. 255'),
                    (dict(order='wavefront', depth_block=B, conceal=True), 'conceal'),
                    (dict(front_ends=[C], depth_block=B), "needs order='wavefront'")):
        with pytest.raises(ValueError, match=why):
            pred.decode_tiles_batch([vol], th, tw, **kw)
    with pytest.raises(ValueError, match="needs order='wavefront'"):
        pred.encode_tiles(sym, th, tw, depth_block=B)


# ---- files ----------------------------------------------------------------------------------------------------------------------

def _image(H, W_, seed=9):
    from imgcomp_cvpr_amd import weights as W
    return np.ascontiguousarray(W.synthetic_image((1, 3, H, W_), 'natural', seed=seed)[0].transpose(1, 2, 0))


@pytest.fixture(scope='module')
def cdc(cuda, configs, syn_weights):
    from imgcomp_cvpr_amd import codec
    return codec.Codec(configs[0], configs[1], syn_weights, cuda)


def _as(c, version, fn, B=4):
    """run fn() with the Codec writing format 10 (depth blocks of B) or format 5, tiles of 4 x 4 cells"""
    c.tile, c.order, c.depth_block = (4, 4), ('wavefront' if version == 5 else 'raster'), (B if version == 10 else None)
    try:
        return fn()
    finally:
        c.tile, c.order, c.depth_block = None, 'raster', None


def _cap_plane(h, w, C):
    """integer levels 0, 3, C / 2 and C in patches of 4 x 4 cells (the tiles, and the depth blocks of B = 4)"""
    levels = np.array([[C, 0, C // 2], [3, C, 0]])
    return levels[(np.arange(h) // 4)[:, None] % 2, (np.arange(w) // 4)[None, :] % 3].astype(np.float64)


@pytest.fixture(scope='module', params=[(64, 96), (50, 76)], ids=['64x96', '50x76'])
def files(request, cdc):
    H, W_ = request.param
    img = _image(H, W_, seed=H)
    h, w = -(-H // 8), -(-W_ // 8)
    plane = _cap_plane(h, w, cdc.C)
    assert sorted(set(plane.reshape(-1).tolist())) == [0, 3, cdc.C // 2, cdc.C]
    enc, _, size = cdc.encode_symbols_capped(img, plane)
    sym = enc.symbols[0].cpu().numpy()
    assert size == (H, W_) and sym.shape == (cdc.C, h, w)
    ten = _as(cdc, 10, lambda: cdc.compress(img, cap=plane))
    five = _as(cdc, 5, lambda: cdc.compress(img, cap=plane))
    return dict(img=img, plane=plane, sym=sym, ten=ten, five=five, H=H, W=W_, h=h, w=w)


def _live_share(codec, c):
    live = sum(int(codec.depth_live(c.C, a, b, codec.split_depth_stream(s, c.C, a, b, c.depth_block)[0], c.depth_block).sum())
               for (_, _, a, b), s in zip(codec.tile_grid(c.h, c.w, c.th, c.tw), c.streams))
    return live / float(c.C * c.h * c.w)


def test_file_symbols_pixels_and_bytes(cdc, files):
    from imgcomp_cvpr_amd import codec
    f = files
    fill = cdc.pred.conceal_fallback()
    assert np.array_equal(f['sym'], codec.cap_symbols(f['sym'], f['plane'], fill))           # the cap holds in the encoder's symbols
    c = codec.parse_container(f['ten'])
    assert isinstance(c, codec.DepthContainer) and c.version == 10 and c.depth_block == 4 and (c.th, c.tw) == (4, 4)
    share = _live_share(codec, c)
    print('{} x {}: live share {:.4f}, format 10 {} bytes, format 5 {} bytes'.format(f['H'], f['W'], share, len(f['ten']), len(f['five'])))
    assert share >= 0.25 and 1.0 - share >= 0.25, 'dead and live positions are each at least a quarter of the volume'
    got, _ = cdc.decode_symbols(f['ten'])
    assert got.dtype == np.int64 and np.array_equal(got, f['sym'])
    assert np.array_equal(cdc.decompress(f['ten']), cdc.decompress(f['five']))
    # the file: build_depth_container over depth_plane and the host coder's bytes of the kept symbols
    streams, firsts = [], []
    for y0, x0, a, b in codec.tile_grid(c.h, c.w, 4, 4):
        ts = f['sym'][:, y0:y0 + a, x0:x0 + b]
        depth = codec.depth_plane(ts, fill, 4)
        assert np.array_equal(depth, dr.depth_plane(ts, fill, 4))
        streams.append(depth.tobytes() + dr.host_encode(ts, _tile_freqs(cdc.pred, ts), depth, 4))
        firsts.append(int(ts[0, 0, 0]))
    assert f['ten'] == codec.build_depth_container(cdc.ae_name, cdc.pc_name, f['H'], f['W'], cdc.C, c.h, c.w, cdc.L, cdc.pred.freqs_resolution,
                                                   cdc.fingerprint, 4, 4, 4, firsts, streams)
    # a preview, and the host tools
    assert np.array_equal(cdc.decompress(f['ten'], channels=3), cdc.decompress(f['five'], channels=3))
    assert np.array_equal(cdc.decode_symbols(f['ten'], channels=3)[0], codec.preview_symbols(f['sym'], 3, fill))
    assert codec.verify_file(f['ten'])[0] and 'live share {:.4f}'.format(share) in codec.info_file(f['ten'])
    assert _as(cdc, 10, cdc.written_version) == 10 and _as(cdc, 5, cdc.written_version) == 5


def test_transcode_both_ways_without_the_autoencoder(cdc, files):
    f = files

    def never(*a, **kw):
        raise AssertionError('the autoencoder was run')

    names = ('encode', 'encode_capped', 'decode')
    for name in names:
        setattr(cdc.ae, name, never)                                         # instance attributes in front of the methods ...
    try:
        assert _as(cdc, 10, lambda: cdc.transcode(f['five'])) == f['ten']
        assert _as(cdc, 5, lambda: cdc.transcode(f['ten'])) == f['five']
        assert _as(cdc, 10, lambda: cdc.transcode_many([f['five'], f['ten']])) == [f['ten'], f['ten']]
        assert _as(cdc, 10, lambda: cdc.transcode(f['five'], cap=3)) == _as(cdc, 10, lambda: cdc.transcode(f['ten'], cap=3))
        for B in (1, 2):                                                     # another block size: other bytes, the same symbols
            other = _as(cdc, 10, lambda: cdc.transcode(f['ten']), B=B)
            assert other != f['ten'] and _as(cdc, 5, lambda: cdc.transcode(other)) == f['five']
    finally:
        for name in names:
            delattr(cdc.ae, name)                                            # ... and gone again: nothing bound to this object is left behind


def test_many_region_measure(cdc, files):
    f = files
    other = _image(40, 56, seed=3)
    tens = _as(cdc, 10, lambda: cdc.compress_many([f['img'], other], caps=[f['plane'], None]))
    assert tens[0] == f['ten'] and tens[1] == _as(cdc, 10, lambda: cdc.compress(other))
    fives = [f['five'], _as(cdc, 5, lambda: cdc.compress(other))]
    many = cdc.decompress_many(tens + fives)
    singles = [cdc.decompress(d) for d in tens + fives]
    assert all(np.array_equal(a, b) for a, b in zip(many, singles))
    assert np.array_equal(many[0], many[2]) and np.array_equal(many[1], many[3])
    full = singles[0]
    for rect in ((0, 0, 24, 16), (f['W'] - 30, f['H'] - 20, 30, 20), (17, 9, 40, 33)):
        x, y, rw, rh = rect
        assert np.array_equal(cdc.decompress_region(f['ten'], rect), full[y:y + rh, x:x + rw]), rect
    a, b = cdc.measure(f['img'], f['ten']), cdc.measure(f['img'], f['five'])
    assert a.bytes == len(f['ten']) and b.bytes == len(f['five'])
    assert a._replace(bytes=0, bpp=0.0) == b._replace(bytes=0, bpp=0.0)


def test_the_other_readers_refuse(cdc, files):
    ten = files['ten']
    why = r'format version 10 \(depth-mapped tiles\) is not read by'
    for call in (cdc.salvage, cdc.decompress_partial, cdc.recover, cdc.repair, lambda d: cdc.open_stream().feed(d),
                 lambda d: cdc.open_stream(fronts=True).feed(d)):
        with pytest.raises(ValueError, match=why):
            call(ten)


def test_uncapped_round_trip(cdc):
    from imgcomp_cvpr_amd import codec
    img = _image(64, 96, seed=2)
    enc, _ = cdc.encode_symbols(img)
    sym = enc.symbols[0].cpu().numpy()
    for B in (1, 4):
        ten = _as(cdc, 10, lambda: cdc.compress(img), B=B)
        five = _as(cdc, 5, lambda: cdc.compress(img))
        print('uncapped 64 x 96, B = {}: live share {:.4f}, format 10 {} bytes, format 5 {} bytes'.format(
            B, _live_share(codec, codec.parse_container(ten)), len(ten), len(five)))
        assert np.array_equal(cdc.decode_symbols(ten)[0], sym)
        assert np.array_equal(cdc.decompress(ten), cdc.decompress(five))
