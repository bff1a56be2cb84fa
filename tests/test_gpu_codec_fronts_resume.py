"""-m gpu: a front-ordered decode that goes on where the last call stopped -- the resumable wavefront tile decoder
(ic_pc_decode_tiles_batch_fronts_resume_f32) through the ABI against the full decode of the same bytes, call after call on one workspace;
the session (PredictionNetwork.open_layers(front_ends=...)) against decode_tiles_batch(front_ends=..., tile_layers=...); the stream decoder
and `stream --fronts` against Codec.recover of the same prefixes.  test_gpu_codec_resume.py on front-cut streams.
Every comparison is an equality."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import recover_rule as RR
from tests.test_gpu_codec_decoder import _load, _model
from tests.test_gpu_codec_fronts import _coded, _raw_fronts, _write
from tests.test_gpu_codec_layered import GUARD, Q_GUARD, SYM_GUARD, _image
from tests.test_gpu_codec_resume import _seg_start, _thin

pytestmark = pytest.mark.gpu

FRONTS, LAYERS = 'ic_pc_decode_tiles_batch_fronts_resume', 'ic_pc_decode_tiles_batch_layers_resume'


@pytest.fixture(scope='module')
def pred(cuda, configs, syn_weights):
    return _load(cuda, configs[0], configs[1], syn_weights, 1e9)


@pytest.fixture(scope='module')
def cdc(cuda, configs, syn_weights):
    from imgcomp_cvpr_amd import codec
    return codec.Codec(configs[0], configs[1], syn_weights, cuda)


# ---- the decoder through the ABI ----------------------------------------------------------------------------------------------

class _Raw(object):
    """ic_pc_decode_tiles_batch_fronts_resume_f32 through the ABI, call after call on ONE workspace and ONE pair of symbols / q buffers
    (test_gpu_codec_resume._Raw for the new entry): the tile descriptors' stream fields hold nonsense, the volumes lie `slack` cells
    apart, symbols, q, status and the tail of the workspace carry guard values.  The workspace proper starts as `ws_fill`.
    `want_sym` / `want_q` are the host's statement of what the two buffers must hold, as symbols: SYM_GUARD where no call has written (or
    where rearm() put the guards back), and after a call, per tile with status 0 or 1, the full decode in [cfrom, limit), the fill in
    [limit, C) and whatever stood there below cfrom.  A call may leave out symbols or q (outputs); that buffer then stays as it is."""

    def __init__(self, cuda, pred, volumes, full, th, tw, ends, slack=4096, ws_fill=0, k=24):
        from imgcomp_cvpr_amd import _lib, codec
        self.cuda, self.pred, self.volumes, self.full, self.ends, self.slack = cuda, pred, volumes, full, list(ends), slack
        self.tiles, self.cells, self.offs, total = [], [], [], slack
        for n, (streams, firsts, (C, h, w)) in enumerate(volumes):
            for t, (y0, x0, a, b) in enumerate(codec.tile_grid(h, w, th, tw)):
                self.tiles.append((y0, x0, a, b, -5, 1 << 40, firsts[t], n))
                self.cells.append((n, slice(y0, y0 + a), slice(x0, x0 + b), streams[t]))
            self.offs.append(total)
            total += C * h * w + slack
        self.total, self.C = total, volumes[0][2][0]
        self.sym = torch.full((total,), SYM_GUARD, dtype=torch.int64, device=cuda)
        self.q = torch.full((total,), Q_GUARD, dtype=torch.float32, device=cuda)
        self.shape_args = (self.C, max(t[2] for t in self.tiles), max(t[3] for t in self.tiles), len(self.tiles), len(volumes), k, len(ends))
        self.need = int(getattr(_lib.lib, FRONTS + '_workspace_bytes')(*self.shape_args))
        self.need_layers = int(getattr(_lib.lib, LAYERS + '_workspace_bytes')(*self.shape_args))
        assert self.need >= self.need_layers + len(self.tiles) * self.C * self.shape_args[1] * self.shape_args[2]
        self.ws = torch.full((self.need + slack,), GUARD, dtype=torch.uint8, device=cuda)
        self.ws[:self.need] = ws_fill
        self.want_sym = [np.full(shape, SYM_GUARD, np.int64) for _, _, shape in volumes]
        self.want_q = [np.full(shape, SYM_GUARD, np.int64) for _, _, shape in volumes]
        self.centers = pred.centers.contiguous().float()
        self.vtable = _lib.volume_table([(h, w, o, o) for (_, _, (_, h, w)), o in zip(volumes, self.offs)])

    want = property(lambda self: self.want_sym)

    def snap(self):
        return self.sym.clone(), self.q.clone(), self.ws.clone(), [w.copy() for w in self.want_sym], [w.copy() for w in self.want_q]

    def restore(self, state):
        self.sym.copy_(state[0])
        self.q.copy_(state[1])
        self.ws.copy_(state[2])
        self.want_sym, self.want_q = [w.copy() for w in state[3]], [w.copy() for w in state[4]]

    def rearm(self):
        """guard values back into symbols and q: a later call must leave them standing below its cfrom"""
        self.sym.fill_(SYM_GUARD)
        self.q.fill_(Q_GUARD)
        for w in self.want_sym + self.want_q:
            w[...] = SYM_GUARD

    def out(self):
        """[(symbols, q as int32 bits)] per volume, as the buffers stand"""
        got, qs = self.sym.cpu().numpy(), self.q.cpu().numpy().view(np.int32)
        return [(got[o:o + c * h * w].reshape(c, h, w), qs[o:o + c * h * w].reshape(c, h, w)) for (_, _, (c, h, w)), o in zip(self.volumes, self.offs)]

    def call(self, froms, limits, fill, unneeded='real', ws_short=0, flags=0, nlayers=None, break_seg=None, ends=None, outputs='both',
             entry=FRONTS, check=True):
        """-> (return code, status list or None).  unneeded: what stands for the segments this call has no use for -- those of layers below
        from[t] and of layers that begin at or above limits[t] --: 'real' (their bytes), 'zero' ({0, 0}), 'other' (other bytes at
        another place).  Checks the guards and, for a served call, symbols and q against what the calls so far must have left.
        entry=LAYERS: the raster entry on the same workspace (with its own, smaller size); check=False: the guards only -- what such a
        call decodes of front-ordered bytes is no matter here, rearm() behind it."""
        from imgcomp_cvpr_amd import _lib
        pred, cuda, G = self.pred, self.cuda, len(self.ends)
        junk = bytes(np.random.RandomState(97).randint(0, 256, size=43).astype(np.uint8))
        segs, blobs, pos = [], [junk], len(junk)
        for (n, ys, xs, streams), g_from, K in zip(self.cells, froms, limits):
            for g in range(G):
                needed = g_from <= g and (g == 0 or self.ends[g - 1] < K)
                if needed or unneeded == 'real':
                    segs.append((pos, len(streams[g])))
                    blobs.append(bytes(streams[g]))
                    pos += len(streams[g])
                else:
                    segs.append((0, 0) if unneeded == 'zero' else (7, len(junk) - 7))
        if break_seg is not None:
            i, seg = break_seg
            segs[i] = seg(pos)
        table, seg_table = _lib.tile_table(self.tiles), _lib.seg_table(segs)
        data = torch.frombuffer(bytearray(b''.join(blobs)), dtype=torch.uint8).to(cuda)
        nt = len(self.tiles)
        status = torch.full((nt + self.slack,), SYM_GUARD, dtype=torch.int32, device=cuda)
        before = (self.sym.clone(), self.q.clone(), self.ws.clone())
        use_ends = self.ends if ends is None else ends
        host_ends = (ctypes.c_int * max(len(use_ends), 1))(*use_ends)
        host_from, host_limits = (ctypes.c_int * nt)(*froms), (ctypes.c_int * nt)(*limits)
        need = self.need if entry == FRONTS else self.need_layers
        rc = getattr(_lib.lib, entry + '_f32')(
            _lib.ptr(data), pos, table, nt, self.vtable, len(self.volumes), pred.pc._tab, _lib.ptr(self.centers), pred.pc._k, pred.pc.L,
            pred.freqs_resolution, _lib.ptr(self.sym) if outputs != 'q' else None, _lib.ptr(self.q) if outputs != 'symbols' else None,
            _lib.ptr(status), self.C, _lib.ptr(self.ws), need - ws_short,
            int(flags), _lib.current_stream(cuda), host_from, host_limits, int(fill), host_ends, G if nlayers is None else nlayers, seg_table)
        torch.cuda.synchronize()
        assert bool((self.ws[self.need:] == GUARD).all()), 'workspace: written behind its stated size'
        assert bool((status[nt:] == SYM_GUARD).all()), 'status: written behind the table'
        if rc != 0:
            assert bool((status == SYM_GUARD).all()), 'a refused call wrote status'
            assert torch.equal(self.sym, before[0]) and torch.equal(self.q.view(torch.int32), before[1].view(torch.int32)), 'a refused call wrote symbols or q'
            assert torch.equal(self.ws, before[2]), 'a refused call wrote the workspace'
            return rc, None
        if outputs == 'q':
            assert torch.equal(self.sym, before[0]), 'symbols written by a call that was given none'
        if outputs == 'symbols':
            assert torch.equal(self.q.view(torch.int32), before[1].view(torch.int32)), 'q written by a call that was given none'
        status = status[:nt].tolist()
        if not check:
            return rc, status
        for (n, ys, xs, _), g_from, K, st in zip(self.cells, froms, limits, status):
            if st == 2:
                continue                                                      # the tile was not touched
            cfrom = self.ends[g_from - 1] if g_from else 0
            for want in ([self.want_sym] if outputs != 'q' else []) + ([self.want_q] if outputs != 'symbols' else []):
                want[n][cfrom:K, ys, xs] = self.full[n][cfrom:K, ys, xs]
                want[n][K:, ys, xs] = fill
        got = self.sym.cpu().numpy()
        qs = self.q.cpu().numpy()
        outside = np.ones(self.total, bool)
        centres = self.centers.cpu().numpy()
        for (_, _, (c, h, w)), o, want_sym, want_q in zip(self.volumes, self.offs, self.want_sym, self.want_q):
            outside[o:o + c * h * w] = False
            s = got[o:o + c * h * w].reshape(c, h, w)
            assert np.array_equal(s, want_sym), 'from {} limits {} ({}): symbols are not what the calls so far must have left'.format(froms, limits, unneeded)
            q_want = np.where(want_q == SYM_GUARD, np.float32(Q_GUARD), centres[np.clip(want_q, 0, len(centres) - 1)])
            assert np.array_equal(qs[o:o + c * h * w].reshape(c, h, w).view(np.int32), q_want.astype(np.float32).view(np.int32)), \
                'from {} limits {} ({}): q is not the centres of what the calls so far must have left'.format(froms, limits, unneeded)
        assert (got[outside] == SYM_GUARD).all() and (qs[outside] == np.float32(Q_GUARD)).all(), 'written outside the volumes'
        return rc, status


_CASES = {}


def _coded_case(cuda, pred, name, ends):
    """(volumes as _coded gives them, the full decode per volume, th, tw): coded once per (volume set, layer ends), the reference
    decoded once by the fronts entry and checked against what was coded"""
    key = (name, tuple(ends))
    if key not in _CASES:
        C = ends[-1]
        shapes, th, tw = {'5x7 at tile 4': ([(C, 5, 7)], 4, 4), '8x8 at tile 8': ([(C, 8, 8)], 8, 8),
                          'both at tile 4': ([(C, 5, 7), (C, 8, 8)], 4, 4)}[name]
        rs = np.random.RandomState(len(name) + sum(ends))
        syms = [rs.randint(0, pred.pc.L, size=s).astype(np.int64) for s in shapes]
        vols = _coded(pred, syms, th, tw, ends)
        rc, full, _, status = _raw_fronts(cuda, pred, vols, th, tw, ends, C, pred.conceal_fallback())
        assert rc == 0 and status == [0] * len(status) and all(np.array_equal(a, b) for a, b in zip(full, syms))
        for f in full:
            f.setflags(write=False)
        _CASES[key] = (vols, full, th, tw)
    return _CASES[key]


VOLUMES = ['5x7 at tile 4', '8x8 at tile 8', 'both at tile 4']
ENDS = {'1,2,C': [1, 2, 8], '3,4,7,C': [3, 4, 7, 8], 'default': [1, 2, 4, 8], 'G=16': list(range(1, 17))}


def test_a_layer_steps_through_later_channels():
    """what makes the symbol plane necessary, on the shapes of these tests: the 8 x 8 tile's fronts span six channels, so layer 0 of
    ends 1, 2, C already steps through symbols of layer 2, and the 4 x 4 and 4 x 3 tiles carry symbols of channels >= cfrom over every
    cut; the 1 x 4 and 1 x 3 edge tiles carry none (w + 2 h < 7: their fronts never span two channels)"""
    from imgcomp_cvpr_amd import codec
    order = codec.wavefront_order(8, 8, 8)
    assert (order[:codec.wavefront_prefix_count(8, 8, 8, 1)] // 64).max() == 5
    for h, w in ((4, 4), (4, 3), (1, 4), (1, 3), (8, 8)):
        for cfrom in (1, 2, 3, 4, 7):
            assert (codec.wavefront_prefix_count(8, h, w, cfrom) - cfrom * h * w > 0) == (w + 2 * h >= 7)


@pytest.mark.parametrize('ends', sorted(ENDS), ids=sorted(ENDS))
@pytest.mark.parametrize('volumes', VOLUMES)
def test_layer_by_layer(cuda, pred, volumes, ends):
    """fresh to layer 0, then one layer per call up to G: after every call [cfrom, cdec) is the full decode -- the symbols that an
    earlier launch stepped through included --, [cdec, C) the fill and [0, cfrom) what the call before left: the symbols of the earlier
    layers, or, re-armed between the calls, the guards.  Re-armed, a symbol of [cfrom, cdec) that an earlier launch decoded can only
    come from the symbol plane."""
    from imgcomp_cvpr_amd import codec
    assert ENDS['default'] == codec.default_layer_ends(8)
    ends = ENDS[ends]
    vols, full, th, tw = _coded_case(cuda, pred, volumes, ends)
    fill, G = pred.conceal_fallback(), len(ends)
    for rearm, unneeded in ((False, 'real'), (True, 'zero'), (False, 'other')):
        raw = _Raw(cuda, pred, vols, full, th, tw, ends)
        nt = len(raw.tiles)
        for g in range(G):
            if rearm:
                raw.rearm()
            rc, status = raw.call([g] * nt, [ends[g]] * nt, fill, unneeded=unneeded)
            assert rc == 0 and status == [0] * nt, (g, rc, status)
            if not rearm:
                assert all((w[:ends[g]] == f[:ends[g]]).all() and (w[ends[g]:] == fill).all() for w, f in zip(raw.want, full))
            else:
                assert all((w[:ends[g - 1] if g else 0] == SYM_GUARD).all() for w in raw.want)
                assert all(np.array_equal(w[ends[g - 1] if g else 0:ends[g]], f[ends[g - 1] if g else 0:ends[g]]) for w, f in zip(raw.want, full))
        rc, status = raw.call([G] * nt, [ends[-1]] * nt, fill, unneeded='zero')      # every tile whole: nothing is decoded or written
        assert rc == 0 and status == [0] * nt


@pytest.mark.parametrize('volumes', VOLUMES)
def test_jumps(cuda, pred, volumes):
    ends = ENDS['3,4,7,C']
    vols, full, th, tw = _coded_case(cuda, pred, volumes, ends)
    fill, G = pred.conceal_fallback(), len(ends)
    for path in ([0, 2, G], [0, G], [0, 1, G], [0, 3, G]):
        raw = _Raw(cuda, pred, vols, full, th, tw, ends)
        nt = len(raw.tiles)
        for a, b in zip(path, path[1:]):
            rc, status = raw.call([a] * nt, [ends[b - 1]] * nt, fill)
            assert rc == 0 and status == [0] * nt, (path, a, b, status)
        assert all(np.array_equal(w, f) for w, f in zip(raw.want, full)), path        # (call() has compared the buffers with want)


def test_symbols_or_q_alone(cuda, pred):
    """the kernel without `symbols` keeps the plane too: q alone layer by layer, then one call with symbols alone gets, re-armed, the
    symbols of its layer that the q-only launches stepped through; and the reverse for q, which comes from V"""
    ends = ENDS['1,2,C']
    vols, full, th, tw = _coded_case(cuda, pred, 'both at tile 4', ends)
    fill = pred.conceal_fallback()
    for first, last in (('q', 'symbols'), ('symbols', 'q'), ('q', 'q'), ('symbols', 'symbols')):
        raw = _Raw(cuda, pred, vols, full, th, tw, ends)
        nt = len(raw.tiles)
        assert raw.call([0] * nt, [1] * nt, fill, outputs=first) == (0, [0] * nt)
        assert raw.call([1] * nt, [2] * nt, fill, outputs=first, unneeded='zero') == (0, [0] * nt)
        raw.rearm()
        assert raw.call([2] * nt, [8] * nt, fill, outputs=last, unneeded='zero') == (0, [0] * nt)
        for w, f in zip(raw.want_sym if last == 'symbols' else raw.want_q, full):
            assert np.array_equal(w[2:], f[2:]) and (w[:2] == SYM_GUARD).all()


@pytest.mark.parametrize('ends', ['1,2,C', '3,4,7,C'])
def test_mixed_launch(cuda, pred, ends):
    """one launch with fresh tiles, tiles that continue at different layers, tiles with from == to and whole tiles: the per-tile
    preview rule on the full decode"""
    ends = ENDS[ends]
    vols, full, th, tw = _coded_case(cuda, pred, 'both at tile 4', ends)
    fill, G, C = pred.conceal_fallback(), len(ends), ends[-1]
    first = [1, 2, G, 1, 2, 1, G, 1]                                          # layers after the first call
    # tile 0 goes on to G, 1 stays (from == to), 2 is whole, 3 starts afresh at another limit, 4 goes one layer on, 5 afresh to G,
    # 6 whole, 7 stays
    second = [G, 2, G, 2, 3, G, G, 1]
    froms = [1, 2, G, 0, 2, 0, G, 1]
    for unneeded in ('real', 'zero', 'other'):
        raw = _Raw(cuda, pred, vols, full, th, tw, ends)
        nt = len(raw.tiles)
        assert nt == 8
        rc, status = raw.call([0] * nt, [ends[g - 1] for g in first], fill, unneeded=unneeded)
        assert rc == 0 and status == [0] * nt
        rc, status = raw.call(froms, [ends[g - 1] for g in second], fill, unneeded=unneeded)
        assert rc == 0 and status == [0] * nt
        rc, status = raw.call(second, [ends[g - 1] for g in second], fill, unneeded=unneeded)       # again: every tile has from == to
        assert rc == 0 and status == [0] * nt
        limits, i = [ends[g - 1] for g in second], 0
        for w, f, (_, _, (c, h, wd)) in zip(raw.want, full, vols):
            n = len(RR.grid(h, wd, th, tw))
            assert np.array_equal(w, RR.preview_per_tile(f, limits[i:i + n], th, tw, fill))
            i += n
    # a limit that is no layer end: the sweep stops there, and the slot then holds no layer end -- only a fresh start is served
    rc, status = raw.call([0] * nt, [C - 1] * nt, fill)
    assert rc == 0 and status == [0] * nt
    rc, status = raw.call([G - 1] * nt, [C] * nt, fill)
    assert rc == 0 and status == ([2] * nt if ends[G - 2] != C - 1 else [0] * nt)


@pytest.mark.parametrize('ends', sorted(ENDS), ids=sorted(ENDS))
def test_fresh_start_is_the_pertile_entry(cuda, pred, ends):
    """every from == 0: the symbols, q and status of ic_pc_decode_tiles_batch_fronts_pertile_f32, bit for bit"""
    ends = ENDS[ends]
    vols, full, th, tw = _coded_case(cuda, pred, 'both at tile 4', ends)
    fill, C = pred.conceal_fallback(), ends[-1]
    for limits in ([C] * 8, [1, 2, 3, C, C - 1, 5, ends[0], ends[1]], [ends[0]] * 8):
        for unneeded in ('real', 'zero'):
            rc, syms, qs, status = _raw_fronts(cuda, pred, vols, th, tw, ends, None, fill, limits=limits, unneeded=unneeded)
            assert rc == 0
            raw = _Raw(cuda, pred, vols, full, th, tw, ends)
            assert raw.call([0] * 8, limits, fill, unneeded=unneeded) == (0, status)
            for (s, qbits), want_s, want_q in zip(raw.out(), syms, qs):
                assert np.array_equal(s, want_s) and np.array_equal(qbits, want_q.cpu().numpy().view(np.int32)), (limits, unneeded)


def test_state_guard(cuda, pred):
    ends = ENDS['1,2,C']
    vols, full, th, tw = _coded_case(cuda, pred, '5x7 at tile 4', ends)
    fill, C = pred.conceal_fallback(), ends[-1]
    for ws_fill in (0, 0xFF, GUARD):                                          # a workspace no call has written: no such word is a cfrom
        raw = _Raw(cuda, pred, vols, full, th, tw, ends, ws_fill=ws_fill)
        for g_from in (1, 2, 3):
            rc, status = raw.call([g_from] * 4, [C] * 4, fill)
            assert rc == 0 and status == [2] * 4
            assert all((w == SYM_GUARD).all() for w in raw.want)              # (call() has compared the buffers with want: untouched)
    raw = _Raw(cuda, pred, vols, full, th, tw, ends)
    assert raw.call([0] * 4, [1, 1, 2, 2], fill) == (0, [0] * 4)              # tiles 0, 1 hold layer 0; tiles 2, 3 layers 0 and 1
    raw.rearm()
    rc, status = raw.call([2, 1, 1, 2], [C] * 4, fill)                        # tile 0 one layer beyond, tile 2 one layer short
    assert rc == 0 and status == [2, 0, 2, 0]
    assert (raw.want[0][:, :4, :4] == SYM_GUARD).all() and (raw.want[0][:, 4:, :4] == SYM_GUARD).all()
    rc, status = raw.call([1, 3, 2, 3], [C] * 4, fill)                        # the refused tiles are where they were: a correct call is served
    assert rc == 0 and status == [0] * 4
    assert np.array_equal(raw.want[0][1:, :4, :4], full[0][1:, :4, :4]) and np.array_equal(raw.want[0][2:, 4:, :4], full[0][2:, 4:, :4])


def test_state_guard_tells_the_two_orders_apart(cuda, pred):
    """one workspace of the larger size, given to both resume entries: a slot that the raster entry swept (its caches filled plane by
    plane) gets status 2 from the fronts entry, and a slot the fronts entry swept gets status 2 from the raster entry.  (What the raster
    entry decodes of these front-ordered bytes is no matter: its done word is.)"""
    ends = ENDS['1,2,C']
    vols, full, th, tw = _coded_case(cuda, pred, '5x7 at tile 4', ends)
    fill, C = pred.conceal_fallback(), ends[-1]
    raw = _Raw(cuda, pred, vols, full, th, tw, ends)
    assert raw.need > raw.need_layers
    rc, status = raw.call([0] * 4, [1, 1, 2, 2], fill, entry=LAYERS, check=False)
    assert rc == 0 and status == [0] * 4
    rc, status = raw.call([1, 1, 2, 2], [2, 2, C, C], fill, entry=LAYERS, check=False)       # (the raster entry itself continues there)
    assert rc == 0 and status == [0] * 4
    raw.rearm()
    rc, status = raw.call([2, 2, 3, 3], [C] * 4, fill)                        # the layers the raster sweeps ended at
    assert rc == 0 and status == [2] * 4 and all((w == SYM_GUARD).all() for w in raw.want)
    assert raw.call([0] * 4, [1, 1, 2, 2], fill) == (0, [0] * 4)              # the fronts entry, afresh
    state = raw.snap()
    rc, status = raw.call([1, 1, 2, 2], [C] * 4, fill, entry=LAYERS, check=False)
    assert rc == 0 and status == [2] * 4
    assert torch.equal(raw.sym, state[0]) and torch.equal(raw.q.view(torch.int32), state[1].view(torch.int32)), 'a tile with status 2 was written'
    assert raw.call([1, 1, 2, 2], [C] * 4, fill) == (0, [0] * 4)              # the slots are still the fronts entry's
    assert all(np.array_equal(w, f) for w, f in zip(raw.want, full))


def test_tile_with_a_coder_error(cuda):
    """test_gpu_codec_resume.test_tile_with_a_coder_error for front cuts: two 1 x 1 tiles of two channels (a 1 x 1 tile's fronts are its
    channels: segment 0 is the uncoded first symbol alone), one over the coder's limit at every position.  Behind a sweep that ended
    with status 1 the slot holds nothing that can be continued."""
    from imgcomp_cvpr_amd import arithmetic_coding as ac, codec
    assert codec.front_layer_cuts(2, 1, 1, [1, 2]) == [1, 2]
    model, table = _model(cuda, [40, 0, 0, 0], resolution=2.0 ** 30)
    assert sum(table) == ac.MAX_TOTAL + 1
    data = np.random.RandomState(9).randint(0, 256, size=40).astype(np.uint8).tobytes()
    fill = model.conceal_fallback()
    two = ([[data[:9], data[9:20]], [data[20:30], data[30:]]], [2, 3], (2, 1, 2))
    full = [np.zeros((2, 1, 2), np.int64)]
    full[0][0, 0] = [2, 3]
    raw = _Raw(cuda, model, [two], full, 1, 1, [1, 2])
    # (channel 1 of a full decode is no matter here: the buffers of `raw`, a call of its own)

    def call(froms, limits):
        from imgcomp_cvpr_amd import _lib
        segs, blobs, pos = [], [], 0
        for streams in two[0]:
            for b in streams:
                segs.append((pos, len(b)))
                blobs.append(b)
                pos += len(b)
        status = torch.full((2,), SYM_GUARD, dtype=torch.int32, device=cuda)
        blob = torch.frombuffer(bytearray(b''.join(blobs)), dtype=torch.uint8).to(cuda)
        rc = _lib.lib.ic_pc_decode_tiles_batch_fronts_resume_f32(
            _lib.ptr(blob), pos, _lib.tile_table(raw.tiles), 2, raw.vtable, 1, model.pc._tab, _lib.ptr(raw.centers), model.pc._k, model.pc.L,
            model.freqs_resolution, _lib.ptr(raw.sym), _lib.ptr(raw.q), _lib.ptr(status), 2, _lib.ptr(raw.ws), raw.need, 0,
            _lib.current_stream(cuda), (ctypes.c_int * 2)(*froms), (ctypes.c_int * 2)(*limits), int(fill), (ctypes.c_int * 2)(1, 2), 2,
            _lib.seg_table(segs))
        torch.cuda.synchronize()
        assert bool((raw.ws[raw.need:] == GUARD).all())
        o = raw.offs[0]
        return rc, status.tolist(), raw.sym[o:o + 4].view(2, 1, 2).cpu().numpy()

    rc, status, sym = call([0, 0], [1, 1])
    assert rc == 0 and status == [0, 0] and sym[0, 0].tolist() == [2, 3] and (sym[1] == fill).all()
    rc, status, sym = call([1, 0], [2, 1])                                    # tile 0 goes on into its coded channel: the coder's error
    assert rc == 0 and status == [1, 0] and 0 <= sym[1, 0, 0] < 4 and sym[1, 0, 1] == fill and sym[0, 0].tolist() == [2, 3]
    raw.sym.fill_(SYM_GUARD)
    for g_from in (1, 2):                                                     # neither what it held (1) nor what it was asked for (2)
        rc, status, sym = call([g_from, 1], [2, 1])
        assert rc == 0 and status == [2, 0], g_from
        assert (sym[:, 0, 0] == SYM_GUARD).all() and sym[0, 0, 1] == SYM_GUARD and sym[1, 0, 1] == fill
    rc, status, sym = call([0, 1], [1, 2])                                    # afresh up to the first symbol: served again
    assert rc == 0 and status == [0, 1] and sym[0, 0, 0] == 2


def test_refusals_write_nothing(cuda, pred):
    from imgcomp_cvpr_amd import _lib
    ends = ENDS['1,2,C']
    vols, full, th, tw = _coded_case(cuda, pred, '5x7 at tile 4', ends)
    fill, C, G = pred.conceal_fallback(), ends[-1], len(ends)
    raw = _Raw(cuda, pred, vols, full, th, tw, ends)
    assert raw.call([0] * 4, [1, 2, C, 2], fill) == (0, [0] * 4)             # tiles hold 1, 2, 3, 2 layers
    froms, limits = [1, 2, 3, 0], [C, 2, C, 5]
    for t in range(4):
        for bad in (-1, G + 1, 17):
            assert raw.call(froms[:t] + [bad] + froms[t + 1:], limits, fill)[0] == -1, (t, bad)             # IC_ERR_ARG
        for bad in (0, C + 1, -1):
            assert raw.call(froms, limits[:t] + [bad] + limits[t + 1:], fill)[0] == -1, (t, bad)
    assert raw.call([2, 2, 3, 0], [1, 2, C, 5], fill)[0] == -1                # tile 0: the limit lies below cfrom = 2
    assert raw.call([1, 2, 3, 0], [C, 2, C - 1, 5], fill)[0] == -1            # tile 2: whole, its limit can only be C
    assert raw.call(froms, limits, pred.pc.L)[0] == -1
    # a segment outside [0, total_bytes): refused where the call reads it, not looked at below from[t] nor at or above the limit
    outside = [lambda total: (total - 1, 2), lambda total: (-1, 1), lambda total: (0, -1), lambda total: (total + 1, 0)]
    for seg in outside:
        assert raw.call(froms, limits, fill, break_seg=(G * 0 + 1, seg))[0] == -1      # tile 0 continues with layer 1
        assert raw.call(froms, limits, fill, break_seg=(G * 0 + 2, seg))[0] == -1
        assert raw.call(froms, limits, fill, break_seg=(G * 3 + 0, seg))[0] == -1      # tile 3 starts afresh: segment 0
        assert raw.call(froms, limits, fill, break_seg=(G * 3 + 2, seg))[0] == -1      # ... limit 5: layer 2 begins at 2
        state = raw.snap()
        for i in (G * 0 + 0, G * 1 + 0, G * 1 + 1, G * 1 + 2, G * 2 + 0, G * 2 + 2):   # below from[t], or from == to, or whole
            assert raw.call(froms, limits, fill, break_seg=(i, seg)) == (0, [0] * 4), i
            raw.restore(state)                                                # (the served call has moved tiles 0 and 3 on)
    assert raw.call(froms, limits, fill, ws_short=1)[0] == -3                                               # IC_ERR_WORKSPACE
    assert raw.call(froms, limits, fill, ws_short=raw.need - raw.need_layers)[0] == -3                      # the raster entry's size is too small
    for flags in (_lib.PC_DECODE_WAVEFRONT, _lib.PC_DECODE_RECOMPUTE, _lib.PC_DECODE_PER_LAYER):
        assert raw.call(froms, limits, fill, flags=flags)[0] == -2, flags                                   # IC_ERR_UNSUPPORTED
    for nl in (0, 17):
        assert raw.call(froms, limits, fill, nlayers=nl)[0] == -1, nl
        assert _lib.lib.ic_pc_decode_tiles_batch_fronts_resume_workspace_bytes(C, 4, 4, 4, 1, 24, nl) == 0
    for bad in ([2, 2, C], [1, 2, C - 1]):
        assert raw.call([0] * 4, [1] * 4, fill, ends=bad)[0] == -1, bad
    wide, _ = _model(cuda, [0, 1, 2, 3, 2, 1], 'res_shallow_64')
    other = _Raw(cuda, wide, vols, full, th, tw, ends, k=24)                  # (a refusal reads no stream: the k = 24 model's will do)
    assert other.call([0] * 4, [C] * 4, 0)[0] == -2                                                         # k = 64
    assert raw.call(froms, limits, fill) == (0, [0] * 4)                      # after all the refusals the workspace still serves


# ---- the session --------------------------------------------------------------------------------------------------------------

def test_session_advance(cuda, pred, monkeypatch):
    from imgcomp_cvpr_amd import codec
    plans, real = [], codec.resume_plan
    monkeypatch.setattr(codec, 'resume_plan', lambda done, now, ends: plans.append((done, now)) or real(done, now, ends))
    rs = np.random.RandomState(12)
    shapes, ends = [(8, 5, 7), (8, 8, 8)], [1, 2, 4, 8]
    syms = [rs.randint(0, 3, size=s).astype(np.int64) for s in shapes]       # three symbols: the concealment's votes have majorities
    vols = _coded(pred, syms, 4, 4, ends)
    sequences = [
        [[[1] * 4, [1] * 4], [[2] * 4, [2] * 4], [[3] * 4, [3] * 4], [[4] * 4, [4] * 4]],                     # a file arriving, seen at its layer ends
        [[[1, 1, 0, 0], [0] * 4], [[1, 1, 1, 1], [1, 1, 0, 0]], [[2, 1, 1, 1], [1] * 4], [[2, 2, 2, 2], [2, 2, 1, 1]],
         [[4, 2, 2, 2], [2, 2, 1, 1]], [[4, 4, 3, 2], [2, 3, 1, 4]], [[4] * 4, [4, 4, 1, 4]], [[4] * 4, [4, 4, 1, 4]]],
        [[[0] * 4, [0] * 4], [[4] * 4, [4] * 4]],                                                             # nothing, then everything
        [[[3, 3, 3, 3], [2, 2, 2, 2]], [[1, 3, 4, 0], [2, 1, 2, 3]], [[4, 3, 4, 2], [4, 4, 4, 4]]],           # layers taken back, a tile that leaves
    ]
    for seq in sequences:
        session = pred.open_layers(shapes, 4, 4, front_ends=ends)
        assert session.fronts and session.entry == 'ic_pc_decode_tiles_batch_fronts_resume_f32'
        del plans[:]
        for step, layers in enumerate(seq):
            thin = _thin(vols, layers)
            (got, held) = session.advance([(s, f) for s, f, _ in thin], layers, want='both')
            (want, want_held) = pred.decode_tiles_batch(thin, 4, 4, want='both', front_ends=ends, tile_layers=layers)
            assert held == want_held, (step, layers)
            for (q, s), (wq, ws) in zip(got, want):
                assert torch.equal(s, ws) and torch.equal(q.view(torch.int32), wq.view(torch.int32)), (step, layers)
            assert session.done == layers
        assert session.launches == sum(1 for layers in seq if any(sum(layers, [])))
        if seq is sequences[0]:
            assert plans == [(g - 1, g) for g in range(1, 5) for _ in range(8)]      # every tile continued where it stopped, three times
        if seq is sequences[1]:                                               # once all tiles are in the launch, every tile continues
            assert plans[-8 * 5:] == [(b, l) for before, layers in zip(seq[2:7], seq[3:8]) for b, l in zip(sum(before, []), sum(layers, []))]
    need = session.ws.numel()
    plain = pred.open_layers(shapes, 4, 4, ends)                              # the positional use of today: plane cuts, the smaller workspace
    assert not plain.fronts and plain.entry == 'ic_pc_decode_tiles_batch_layers_resume_f32' and plain.ws.numel() < need
    with pytest.raises(ValueError, match='{} bytes, max_workspace_bytes is {}'.format(need, need - 1)):
        pred.open_layers(shapes, 4, 4, front_ends=ends, max_workspace_bytes=need - 1)
    pred.open_layers(shapes, 4, 4, front_ends=ends, max_workspace_bytes=need)
    for kw in (dict(), dict(layer_ends=ends, front_ends=ends)):
        with pytest.raises(ValueError, match='exactly one of the two'):
            pred.open_layers(shapes, 4, 4, **kw)


# ---- files --------------------------------------------------------------------------------------------------------------------

ENDS32 = [4, 8, 16, 32]


@pytest.fixture(scope='module')
def eight(cdc):
    """a 64 x 96 image at --tile 32 --front-progressive: a (32, 8, 12) volume, six 4 x 4 tiles, front layers 4, 8, 16, 32"""
    from imgcomp_cvpr_amd import codec
    data = _write(cdc, 8, _image(64, 96, seed=5))
    c = codec.parse_container(data)
    assert (c.version, c.C, c.h, c.w, len(c.streams), c.layer_ends) == (8, 32, 8, 12, 6, ENDS32)
    return data, c


_RECOVERED = {}


def _recover(cdc, data, n):
    """Codec.recover(data[:n]), computed once per state of the file (test_gpu_codec_resume._recover)"""
    from imgcomp_cvpr_amd import codec
    _, layers, reasons, ok = codec.parse_recover(data[:n])
    key = (hash(data), tuple(layers), tuple(sorted(reasons.items())), ok)
    if key not in _RECOVERED:
        _RECOVERED[key] = cdc.recover(data[:n])
    return _RECOVERED[key], layers


@pytest.mark.parametrize('chunk', [1, 37, 4096, None], ids=['1', '37', '4096', 'whole'])
def test_stream_decoder(cdc, eight, chunk):
    from imgcomp_cvpr_amd import codec
    data, c = eight
    head = codec.layer_prefix_bytes(data, 0)
    layer_ends_at = {codec.layer_prefix_bytes(data, g): g for g in range(1, 5)}
    dec = cdc.open_stream(fronts=True)
    step = len(data) if chunk is None else chunk
    for pos in range(0, len(data), step):
        ready = dec.feed(data[pos:pos + step])
        n = min(pos + step, len(data))
        assert dec.bytes_fed == n and ready == (n >= head)
        if not ready:
            assert dec.progress() == ()
            with pytest.raises(ValueError, match='no complete layer'):
                dec.image()
            continue
        (want, want_report), layers = _recover(cdc, data, n)
        assert dec.progress() == tuple(layers)
        if not any(layers):
            with pytest.raises(ValueError, match='no complete layer'):
                dec.image()
            continue
        launches = dec._session.launches if dec._session else 0
        img, report = dec.image()
        assert np.array_equal(img, want) and report == want_report, n
        again, report2 = dec.image()                                          # no new layer: the picture again, no launch
        assert again is img and report2 == report and dec._session.launches in (launches, launches + 1)
        if n in layer_ends_at:
            partial, partial_report = cdc.decompress_partial(data[:n])
            assert np.array_equal(img, partial) and partial_report.layers_decoded == layer_ends_at[n]
    assert np.array_equal(img, cdc.decompress(data)) and report == codec.RecoverReport(6, 4, True, [])
    assert dec._session.fronts and dec._session.done == [[4] * 6]
    # a launch per feed that brought a layer: every (tile, layer) fed byte by byte, one for the file fed whole
    assert dec._session.launches == {1: 24, None: 1}.get(chunk, dec._session.launches) and dec._session.launches <= 24


def test_stream_decoder_continues(cdc, eight, monkeypatch):
    """fed at the four layer ends: four launches, and every tile continues three times at the layer it stopped at; a format-6 file
    streams through the same decoder as before"""
    from imgcomp_cvpr_amd import codec
    data, c = eight
    dec, seen, pos = cdc.open_stream(fronts=True), [], 0
    real = codec.resume_plan
    monkeypatch.setattr(codec, 'resume_plan', lambda done, now, ends: seen.append((done, now)) or real(done, now, ends))
    for g in range(1, 5):
        n = codec.layer_prefix_bytes(data, g) if g < 4 else len(data)
        assert dec.feed(data[pos:n])
        pos = n
        img, report = dec.image()
        assert np.array_equal(img, _recover(cdc, data, n)[0][0])
    assert seen == [(g - 1, g) for g in range(1, 5) for _ in range(6)] and dec._session.launches == 4
    six = _write(cdc, 6, _image(64, 96, seed=5))
    dec = cdc.open_stream(fronts=True)
    assert dec.feed(six)
    assert np.array_equal(dec.image()[0], cdc.decompress(six)) and not dec._session.fronts
    with pytest.raises(ValueError, match=r'is not streamed.*--recover'):
        cdc.open_stream().feed(data)                                          # without the option: refused as before


@pytest.fixture(scope='module')
def flipped(eight):
    """one flipped byte in tile 2's segment of layer 1"""
    data, c = eight
    bad = bytearray(data)
    bad[_seg_start(data, c, 1, 2) + len(c.segments[1][2]) // 2] ^= 0x20
    return bytes(bad)


def test_damaged_segment(cdc, eight, flipped):
    data, c = eight
    dec = cdc.open_stream(fronts=True)
    cuts = [_seg_start(data, c, g, t) for g in range(4) for t in (0, 3)][1:] + [len(data)]
    pos = 0
    for n in cuts:
        assert dec.feed(flipped[pos:n])
        pos = n
        (want, want_report), layers = _recover(cdc, flipped, n)
        assert layers[2] <= 1
        img, report = dec.image()
        assert np.array_equal(img, want) and report == want_report, n
    assert dec._session.done == [[4, 4, 1, 4, 4, 4]]
    assert [(d.index, d.layers, d.channels, d.reason) for d in report.tiles] == [(2, 1, 4, 'crc')] and report.file_crc_ok is False


def test_stream_command(cdc, eight, flipped, cuda, tmp_path, capsys):
    from PIL import Image
    from imgcomp_cvpr_amd import codec
    data, c = eight
    icf, out = tmp_path / 'pic.icf', tmp_path / 'out'
    icf.write_bytes(flipped)
    assert codec.main(['stream', str(icf), str(out), '--fronts', '--chunk', '1000', '--device', str(cuda)]) == 0
    lines = capsys.readouterr().out.splitlines()
    names = sorted(os.listdir(str(out)))
    assert len(names) == len(lines) and len(names) >= 2 and all(n.startswith('pic.') and n.endswith('.png') and len(n) == 17 for n in names)
    shown = None
    for pos in range(0, len(flipped), 1000):                                  # a picture exactly where a tile has gained a layer
        n = min(pos + 1000, len(flipped))
        if n < codec.layer_prefix_bytes(data, 0):
            continue
        (want, want_report), layers = _recover(cdc, flipped, n)
        name = 'pic.{:09d}.png'.format(n)
        if layers == shown or not any(layers):
            assert name not in names
            continue
        shown = layers
        assert name in names and np.array_equal(np.asarray(Image.open(str(out / name))), want), n
        assert codec._recover_line(str(out / name), want_report) in lines
    assert shown == [4, 4, 1, 4, 4, 4]
    whole = tmp_path / 'whole.icf'
    whole.write_bytes(data)
    assert codec.main(['stream', str(whole), str(out), '--fronts', '--device', str(cuda)]) == 0          # the default chunk
    capsys.readouterr()
    last = sorted(n for n in os.listdir(str(out)) if n.startswith('whole.'))[-1]
    assert np.array_equal(np.asarray(Image.open(str(out / last))), cdc.decompress(data))
    before = sorted(os.listdir(str(out)))
    assert codec.main(['stream', str(whole), str(out), '--device', str(cuda)]) == 2            # without --fronts: the refusal of before
    err = capsys.readouterr().err
    assert '--recover' in err and '--fronts' in err and sorted(os.listdir(str(out))) == before
    assert codec.main(['stream', str(whole), str(out), '--fronts', '--recover', '--device', str(cuda)]) == 2
    assert '--recover does not go with stream' in capsys.readouterr().err
