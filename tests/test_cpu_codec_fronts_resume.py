"""A front-ordered decode that goes on where the last call stopped, on the host: the resumed wavefront sweep restated on flags and split
into launches, the symbols a sweep carries over a cut, the C ABI of ic_pc_decode_tiles_batch_fronts_resume_f32 as far as it goes without
a device, the feed of a format-8 file, and the --fronts option."""
import argparse
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from imgcomp_cvpr_amd import codec
from tests.test_cpu_codec_fronts import _NoModel, _ends_variants, _file8
from tests.test_cpu_codec_preview import _prototype
from tests.test_cpu_codec_wavefront import _front

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW, PARENT = 'ic_pc_decode_tiles_batch_fronts_resume_f32', 'ic_pc_decode_tiles_batch_layers_resume_f32'
NEW_WS, PARENT_WS = 'ic_pc_decode_tiles_batch_fronts_resume_workspace_bytes', 'ic_pc_decode_tiles_batch_layers_resume_workspace_bytes'

OTHER = [(0, a, b) for a in range(3) for b in range(3)] + [(1, 0, 0), (1, 0, 1), (1, 0, 2), (1, 1, 0), (1, 1, 1)]
FIRST = OTHER[:13]


# ---- the schedule, launch by launch ---------------------------------------------------------------------------------------------

class _Slot(object):
    """what a tile's slot of the workspace holds, as flags: V (pad voxels known from the start) and the three caches"""

    def __init__(self, C, h, w):
        self.shape = (C, h, w)
        self.V = np.ones((C + 4, h + 8, w + 8), bool)
        self.V[4:, 4:h + 4, 4:w + 4] = False
        self.A = [np.zeros((C + 3, h + 6, w + 6), bool), np.zeros((C + 2, h + 4, w + 4), bool), np.zeros((C + 1, h + 2, w + 2), bool)]


def _launch(slot, ends, gfrom, K):
    """pc_dec_wave_body<.., LIM, SEG, FROM> on flags: one launch on a slot, from layer gfrom (0: the slot is filled afresh) up to the
    channel limit K.  Asserts that every cache / V voxel read was written before -- by this launch or an earlier one on the slot -- and
    that none is written twice.  -> (steps, {segment: symbols it gave, in order}, the steps (counted from 0) at which the coder restarted)"""
    C, h, w = slot.shape
    if gfrom == 0:
        slot.__init__(C, h, w)
    V, (A0, A1, A2) = slot.V, slot.A
    T_base = (w - 1) + 2 * (h - 1) - 4 + 28
    T_stop = (w + 3) + 2 * (h + 3) + 4 * (K + 3)
    assert T_stop == T_base + 4 * K
    if gfrom == 0:
        T_first, seg_next, T_cut = 7, 1, (T_base + 4 * ends[0] if len(ends) > 1 else 1 << 30)
        per_seg, current = {0: []}, 0                                         # segment 0 is read from the start
    else:
        cfrom = ends[gfrom - 1]
        T_first, seg_next, T_cut = T_base + 4 * cfrom + 1, gfrom, T_base + 4 * cfrom
        per_seg, current = {}, None                                           # a coder at rest: no segment is open
    steps, restarts = 0, []
    for T in range(T_first, T_stop + 1):
        for out, src, taps, back in ((A0, V, FIRST, 7), (A1, A0, OTHER, 14), (A2, A1, OTHER, 21)):
            todo = _front(T - back, *out.shape)
            for d, i, j in todo:
                assert not out[d, i, j] and all(src[d + a, i + b, j + c] for a, b, c in taps), (gfrom, K, T, d, i, j)
                assert out is not A2 or A0[d + 2, i + 2, j + 2]
            for v in todo:
                out[v] = True
        if T > T_cut:                                                         # the restart: before this front's first symbol
            restarts.append(steps)
            current = seg_next
            per_seg[current] = []
            seg_next += 1
            T_cut = T_base + 4 * ends[seg_next - 1] if seg_next < len(ends) else 1 << 30
        todo = _front(T - 28, C, h, w)
        for c, y, x in todo:
            assert not V[c + 4, y + 4, x + 4] and all(A2[c + a, y + b, x + k] for a, b, k in OTHER), (gfrom, K, T, c, y, x)
        for c, y, x in todo:
            assert current is not None, 'a symbol decoded by a coder at rest'
            V[c + 4, y + 4, x + 4] = True
            per_seg[current].append((c * h + y) * w + x)
        steps += 1
    return steps, per_seg, restarts


def _paths(G):
    """every way from layer 0 to G through layer ends: single steps and jumps"""
    for n in range(G):
        for mid in itertools.combinations(range(1, G), n):
            yield (0,) + mid + (G,)


@pytest.mark.parametrize('shape', [(2, 1, 1), (5, 3, 4), (6, 5, 7), (3, 1, 9), (3, 9, 1), (32, 16, 16)])
def test_wavefront_schedule_continued(shape):
    C, h, w = shape
    full = codec.wavefront_order(C, h, w)
    variants = [e for e in _ends_variants(C) if len(e) <= codec.MAX_LAYERS] + ([[4, 8, 16, 32]] if C == 32 else [])
    single = (w + 3) + 2 * (h + 3) + 4 * (C + 3) - 6
    for ends in variants:
        G = len(ends)
        cuts = codec.front_layer_cuts(C, h, w, ends)
        slot = _Slot(C, h, w)
        for path in _paths(G):
            total = 0
            for a, b in zip(path, path[1:]):
                K = ends[b - 1]
                steps, per_seg, restarts = _launch(slot, ends, a, K)
                total += steps
                cfrom = ends[a - 1] if a else 0
                assert steps == (4 * (K - cfrom) if a else single - 4 * (C - K)), (shape, ends, path, a, b)
                # the segments opened: the layers >= a that begin below the limit, no other; none below a
                assert sorted(per_seg) == [g for g in range(a, G) if g == 0 or ends[g - 1] < K] == list(range(a, b)), (shape, ends, path, a)
                if a:
                    assert restarts[0] == 0                                   # the cut that starts the coder on segment a: in the first step
                assert len(restarts) == b - a - (0 if a else 1)
                for g, got in per_seg.items():                                # segment g gives order[cuts[g - 1] : cuts[g]]
                    assert np.array_equal(np.array(got, np.int64), full[([0] + cuts)[g]:cuts[g]]), (shape, ends, path, g)
                assert sum(len(v) for v in per_seg.values()) == cuts[b - 1] - (cuts[a - 1] if a else 0)
                assert slot.V[4:K + 4, 4:h + 4, 4:w + 4].all()
                assert int(slot.V[4:, 4:h + 4, 4:w + 4].sum()) == cuts[b - 1] == codec.wavefront_prefix_count(C, h, w, K)
            assert total == single, (shape, ends, path)                       # every front swept once, whatever the path
            assert slot.V.all() and all(A.sum() > 0 for A in slot.A)
        if shape == (32, 16, 16) and ends == [4, 8, 16, 32]:
            fresh = [_launch(slot, ends, 0, K)[0] for K in ends]
            assert fresh == [79, 95, 127, 191] and sum(fresh) == 492 and single == 191      # the step arithmetic of the design


def test_a_limit_that_is_no_layer_end_cannot_be_continued():
    """the model says why the guard word must match exactly: behind a sweep to K = 3 of ends 1, 2, 6 a continuation at layer 2 (cfrom = 2)
    would write voxels again, one at layer 3 = G would read voxels that nobody wrote"""
    slot = _Slot(6, 5, 7)
    _launch(slot, [1, 2, 6], 0, 3)
    with pytest.raises(AssertionError):
        _launch(slot, [1, 2, 6], 2, 6)
    slot = _Slot(6, 5, 7)
    _launch(slot, [1, 2, 4, 6], 0, 2)
    with pytest.raises(AssertionError):
        _launch(slot, [1, 2, 4, 6], 3, 6)


@pytest.mark.parametrize('shape', [(2, 1, 1), (5, 3, 4), (6, 5, 7), (3, 1, 9), (3, 9, 1), (8, 4, 4), (8, 4, 3), (8, 1, 4), (8, 1, 3), (8, 8, 8), (8, 1, 5),
                                   (8, 2, 3), (8, 3, 1), (8, 2, 2), (32, 16, 16)])
def test_symbols_carried_over_a_cut(shape):
    """a front sweep to cfrom has stepped through wavefront_prefix_count - cfrom h w symbols of channels >= cfrom: what the resumed call
    cannot decode again and must still deliver.  The last front of channel cfrom - 1 is (w - 1) + 2 (h - 1) + 4 (cfrom - 1), the first
    symbol of channel cfrom lies on front 4 cfrom: there are such symbols exactly if w + 2 h >= 7 (and cfrom < C) -- not on tiles as
    small as 1 x 4 or 2 x 2, whose fronts never span two channels."""
    C, h, w = shape
    order = codec.wavefront_order(C, h, w)
    for cfrom in range(1, C + 1):
        n = codec.wavefront_prefix_count(C, h, w, cfrom)
        early = int((order[:n] // (h * w) >= cfrom).sum())
        assert early == n - cfrom * h * w, (shape, cfrom)
        assert (early > 0) == (w + 2 * h >= 7 and cfrom < C), (shape, cfrom)
        if C * h * w <= 512:                                                  # and the model of the launch agrees
            slot = _Slot(C, h, w)
            _launch(slot, [cfrom, C] if cfrom < C else [C], 0, cfrom)
            assert int(slot.V[4 + cfrom:, 4:h + 4, 4:w + 4].sum()) == early


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------

def test_new_entry_header_bindings_exports():
    from imgcomp_cvpr_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'imgcomp_hip.h')).read(), flags=re.S)
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    exported = set(re.findall(r' T (ic_[a-z0-9_]+)', out))
    for parent, new in ((PARENT, NEW), (PARENT_WS, NEW_WS)):
        assert _prototype(text, new) == _prototype(text, parent), new         # argument for argument
        pr, pa = _lib.PROTOTYPES[parent]
        nr, na = _lib.PROTOTYPES[new]
        assert nr is pr and list(na) == list(pa) and len(na) == len(_prototype(text, new)), new
        assert new in exported and parent in exported
        assert getattr(_lib.lib, new).argtypes == list(na)
    assert _lib.lib.ic_abi_version() == 2


def test_workspace_size():
    from imgcomp_cvpr_amd import _lib
    new, parent = getattr(_lib.lib, NEW_WS), getattr(_lib.lib, PARENT_WS)
    align = lambda b: (b + 255) & ~255
    good = ((32, 16, 16, 24, 1, 24, 4), (6, 4, 4, 4, 1, 24, 3), (8, 4, 3, 8, 2, 24, 16), (32, 16, 16, 1000, 7, 24, 1), (1, 1, 1, 1, 1, 24, 1))
    bad = ((32, 16, 16, 24, 1, 24, 0), (32, 16, 16, 24, 1, 24, 17), (32, 16, 16, 0, 1, 24, 4), (32, 16, 16, 24, 0, 24, 4), (0, 16, 16, 24, 1, 24, 4))
    for args in good:
        C, th, tw, ntiles = args[:4]
        a, b = int(new(*args)), int(parent(*args))
        assert a > b > 0 and a - b >= ntiles * C * th * tw, args              # strictly above, by the symbol planes at least
        assert a == b + ntiles * align(C * th * tw), args                     # ... which are aligned, one per tile
        assert int(new(*args)) == a
    for args in bad:
        assert int(new(*args)) == 0 == int(parent(*args)), args
    # monotone in the number of tiles and in the largest tile: a session's workspace for all tiles serves every smaller launch
    assert new(32, 16, 16, 23, 1, 24, 4) <= new(32, 16, 16, 24, 1, 24, 4) and new(32, 15, 16, 24, 1, 24, 4) <= new(32, 16, 16, 24, 1, 24, 4)


def _host_call(entry=NEW, ends=(1, 2, 6), froms=None, limits=None, segs=None, flags=0, k=24, L=6, fill=0, ws_bytes=None, ntiles=1, nlayers=None,
               tile=(0, 0, 4, 4, 0, 0, 0, 0), total=100):
    """a resume entry with host tables that are real and device pointers that are not (test_cpu_codec_fronts._host_call): every refusal
    is decided on the host, before any device call, so nothing is dereferenced.  The workspace size is 0 unless given: the size check is
    the last of the host's, so a call that none of the earlier checks stops returns IC_ERR_WORKSPACE and still reaches no device."""
    from imgcomp_cvpr_amd import _lib
    G = len(ends)
    fake = ctypes.c_void_p(0x1000)
    tab = (_lib.c_void_p * 8)(*([0x1000] * 8))
    table = _lib.tile_table([tile] * ntiles)
    vtable = _lib.volume_table([(5, 7, 0, 0)])
    seg_table = _lib.seg_table(list(segs) if segs is not None else [(0, 10)] * (G * ntiles))
    host_ends = (ctypes.c_int * max(G, 1))(*ends)
    host_from = (ctypes.c_int * ntiles)(*(froms if froms is not None else [0] * ntiles))
    host_limits = (ctypes.c_int * ntiles)(*(limits if limits is not None else [6] * ntiles))
    return getattr(_lib.lib, entry)(fake, total, table, ntiles, vtable, 1, tab, fake, k, L, 1e9, fake, fake, fake, 6, fake,
                                    0 if ws_bytes is None else ws_bytes, flags, None, host_from, host_limits, fill, host_ends,
                                    G if nlayers is None else nlayers, seg_table)


@pytest.mark.parametrize('entry', [NEW, PARENT])
def test_host_side_refusals_need_no_device(entry):
    """the refusals test_gpu_codec_resume.test_refusals_write_nothing lists, decided without a device -- and the same for both entries"""
    from imgcomp_cvpr_amd import _lib
    ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
    G = 3
    call = lambda **kw: _host_call(entry, **kw)
    assert call() == WORKSPACE                                                # every check passes but the last
    for bad in (-1, G + 1, 17):                                               # from
        assert call(froms=[bad]) == ARG, bad
        assert call(ntiles=2, froms=[0, bad], limits=[6, 6]) == ARG, bad
    for bad in (0, 7, -1):                                                    # limit
        assert call(limits=[bad]) == ARG, bad
        assert call(ntiles=2, limits=[6, bad]) == ARG, bad
    assert call(froms=[2], limits=[1]) == ARG                                 # the limit lies below cfrom = 2
    assert call(froms=[2], limits=[2]) == WORKSPACE                           # from == to: served
    assert call(froms=[3], limits=[5]) == ARG                                 # whole: the limit can only be C
    assert call(froms=[3], limits=[6]) == WORKSPACE
    for bad in ((2, 2, 6), (0, 2, 6), (1, 2, 5), (1, 2, 7), (2, 1, 6)):       # ends
        assert call(ends=bad) == ARG, bad
    for nl in (0, 17, -1):
        assert call(nlayers=nl) == ARG, nl
    assert call(fill=6) == ARG and call(fill=-1) == ARG
    # a segment outside [0, total_bytes): refused where the call reads it, not looked at below from[t] nor at or above the limit
    ok = (0, 10)
    for seg in ((99, 2), (-1, 1), (0, -1), (101, 0)):
        assert call(segs=[seg, ok, ok]) == ARG, seg                           # a fresh start reads segment 0
        assert call(segs=[ok, ok, seg]) == ARG, seg
        assert call(segs=[ok, ok, seg], limits=[2]) == WORKSPACE, seg         # layer 2 begins at 2: not looked at
        assert call(segs=[seg, ok, ok], froms=[1]) == WORKSPACE, seg          # a tile that continues does not need segment 0
        assert call(segs=[seg, seg, ok], froms=[2]) == WORKSPACE, seg         # nor any segment below from[t]
        assert call(segs=[ok, seg, ok], froms=[1]) == ARG, seg
        assert call(segs=[ok, ok, seg], froms=[2]) == ARG, seg
        assert call(segs=[seg, seg, seg], froms=[2], limits=[2]) == WORKSPACE, seg      # from == to: nothing is read
        assert call(segs=[seg, seg, seg], froms=[3]) == WORKSPACE, seg        # whole: nothing is read
        assert call(ntiles=2, froms=[1, 0], limits=[6, 1], segs=[seg, ok, ok, ok, seg, seg]) == WORKSPACE, seg
        assert call(ntiles=2, froms=[1, 0], limits=[6, 1], segs=[ok, ok, ok, seg, ok, ok]) == ARG, seg
    assert call(tile=(0, 0, 4, 4, 0, 0, 6, 0)) == ARG                         # first symbol not below L
    assert call(tile=(3, 0, 4, 4, 0, 0, 0, 0)) == ARG                         # a tile outside its 5 x 7 volume
    for flags in (_lib.PC_DECODE_WAVEFRONT, _lib.PC_DECODE_RECOMPUTE, _lib.PC_DECODE_PER_LAYER):
        assert call(flags=flags) == UNSUPPORTED, flags                        # the order is the entry's own: flags is 0
    assert call(k=64) == UNSUPPORTED and call(L=17) == UNSUPPORTED
    need = int(getattr(_lib.lib, entry.replace('_f32', '_workspace_bytes'))(6, 4, 4, 1, 1, 24, 3))
    assert need > 0 and call(ws_bytes=need - 1) == WORKSPACE
    if entry == NEW:                                                          # the raster entry's size does not serve the new one
        assert call(ws_bytes=int(getattr(_lib.lib, PARENT_WS)(6, 4, 4, 1, 1, 24, 3))) == WORKSPACE


# ---- the feed -----------------------------------------------------------------------------------------------------------------

def test_stream_header_bytes_with_fronts():
    for ends in ([1, 2, 8], [8], list(range(1, 9))):
        data, six, _, _ = _file8(ends=ends)
        head = codec.layer_prefix_bytes(data, 0)
        known = [n for n in range(len(data) + 1) if codec.stream_header_bytes(data[:n], fronts=True) is not None]
        assert known == list(range(known[0], len(data) + 1)) and known[0] < head
        assert all(codec.stream_header_bytes(data[:n], fronts=True) == head for n in known)
        assert known == [n for n in range(len(six) + 1) if codec.stream_header_bytes(six[:n]) is not None]      # as early as format 6 tells
        for n in range(len(six) + 1):                                         # a format-6 file: the option changes nothing
            assert codec.stream_header_bytes(six[:n], fronts=True) == codec.stream_header_bytes(six[:n])
        for n in range(6, len(data) + 1, 7):                                  # the default still refuses, from the version word on
            with pytest.raises(ValueError, match=r'format version 8 .* is not streamed.*--recover'):
                codec.stream_header_bytes(data[:n])
            with pytest.raises(ValueError, match=r'format version 8 .* is not streamed.*--recover'):
                codec.stream_header_bytes(data[:n], fronts=False)
        assert codec.stream_header_bytes(data[:5]) is None and codec.stream_header_bytes(data[:5], fronts=True) is None
    for version in (0, 3, 7, 9):                                              # other versions: refused in the words of before
        bad = data[:4] + bytes([version, 0]) + data[6:40]
        with pytest.raises(ValueError, match='header damaged: format version {} is not the layered version 6'.format(version)):
            codec.stream_header_bytes(bad, fronts=True)
    for version in (4, 5):
        with pytest.raises(ValueError, match=r'--salvage.*decompress'):
            codec.stream_header_bytes(data[:4] + bytes([version, 0]) + data[6:40], fronts=True)


def test_feed_byte_by_byte():
    data, six, _, _ = _file8()
    head = codec.layer_prefix_bytes(data, 0)
    for source in (data, six):                                                # fronts=True on a format-6 file behaves as before
        dec, plain = codec.StreamDecoder(_NoModel(), fronts=True), codec.StreamDecoder(_NoModel())
        for n in range(1, len(source) + 1):
            assert dec.feed(source[n - 1:n]) is (n >= head), n
            assert dec.bytes_fed == n
            assert dec.progress() == (tuple(codec.parse_recover(source[:n])[1]) if n >= head else ())
            if source is six:
                assert plain.feed(source[n - 1:n]) is (n >= head) and plain.progress() == dec.progress()
        assert dec.progress() == (3,) * 4 and dec._session is None
    dec = codec.StreamDecoder(_NoModel(), fronts=True)
    assert dec.feed(data[:head]) is True and dec.progress() == (0,) * 4
    with pytest.raises(ValueError, match='no complete layer'):                # the header alone: no picture yet, and nothing was launched
        dec.image()
    assert dec.fronts and not codec.StreamDecoder(_NoModel()).fronts
    with pytest.raises(ValueError, match=r'format version 8 .* is not streamed.*--recover'):      # the default still raises
        codec.StreamDecoder(_NoModel()).feed(data[:6])
    bad = bytearray(data)
    bad[head - 20] ^= 1
    dec = codec.StreamDecoder(_NoModel(), fronts=True)
    assert dec.feed(bytes(bad[:head - 1])) is False
    with pytest.raises(ValueError, match='header damaged'):
        dec.feed(bytes(bad[head - 1:head]))


def test_open_stream_and_open_layers_keywords():
    from imgcomp_cvpr_amd import probclass
    shell = codec.Codec.__new__(codec.Codec)
    dec = shell.open_stream(fronts=True)
    assert isinstance(dec, codec.StreamDecoder) and dec.fronts and dec.max_workspace_bytes == 1 << 31
    assert not shell.open_stream().fronts and shell.open_stream(1 << 20).max_workspace_bytes == 1 << 20
    pred = probclass.PredictionNetwork.__new__(probclass.PredictionNetwork)
    for kw in (dict(), dict(layer_ends=[1, 2], front_ends=[1, 2])):           # exactly one of the two ends
        with pytest.raises(ValueError, match='exactly one of the two'):
            pred.open_layers([(2, 1, 1)], 1, 1, **kw)


# ---- the option ---------------------------------------------------------------------------------------------------------------

def _flags(command, **kw):
    base = dict(command=command, tile=None, checked=False, wavefront=False, salvage=False, channels=None, layers=None, progressive=False,
                front_layers=None, front_progressive=False, partial=False, recover=False, chunk=None, batch=8, fronts=False)
    base.update(kw)
    return argparse.Namespace(**base)


def test_option_table():
    codec.check_option_args(_flags('stream', fronts=True))
    codec.check_option_args(_flags('stream', fronts=True, chunk=4096))
    codec.check_option_args(_flags('stream'))
    for command in ('compress', 'decompress', 'compress-dir', 'decompress-dir'):
        for kw in (dict(), dict(partial=True), dict(recover=True), dict(channels=4), dict(front_progressive=True)):
            if any(kw) and command.startswith('compress') != ('front_progressive' in kw):
                continue
            flags = _flags(command, fronts=True, tile=128 if command.startswith('compress') else None, **kw)
            with pytest.raises(ValueError, match='--fronts belongs to stream'):
                codec.check_option_args(flags)
            flags.fronts = False
            codec.check_option_args(flags)                                    # the option alone is what was refused
    for kw, why in ((dict(recover=True), '--recover does not go with stream'), (dict(partial=True), '--partial does not go with stream'),
                    (dict(channels=4), '--channels does not go with stream'), (dict(tile=128), '--tile belongs to compress'),
                    (dict(front_progressive=True), '--front-progressive belongs to compress')):
        with pytest.raises(ValueError, match=why):
            codec.check_option_args(_flags('stream', fronts=True, **kw))
    old = argparse.Namespace(command='decompress', tile=None, checked=False, wavefront=False, salvage=True, channels=None)
    codec.check_option_args(old)                                              # a namespace without the key reads as no --fronts


def test_command_line_refuses_before_any_model(tmp_path, capsys):
    src = tmp_path / 'a.icf'
    src.write_bytes(_file8()[0])
    png = tmp_path / 'a.png'
    png.write_bytes(b'x')
    for argv in (['decompress', str(src), str(tmp_path / 'x.png'), '--fronts'], ['decompress', str(src), str(tmp_path / 'x.png'), '--recover', '--fronts'],
                 ['compress', str(png), str(tmp_path / 'x.icf'), '--tile', '32', '--front-progressive', '--fronts'],
                 ['compress-dir', str(tmp_path), str(tmp_path / 'o'), '--fronts'], ['decompress-dir', str(tmp_path), str(tmp_path / 'o'), '--fronts']):
        assert codec.main(argv + ['--device', 'no-such-device']) == 2, argv
        assert '--fronts belongs to stream' in capsys.readouterr().err
    assert codec.main(['stream', str(src), str(tmp_path / 'out'), '--fronts', '--recover', '--device', 'no-such-device']) == 2
    assert '--recover does not go with stream' in capsys.readouterr().err
    assert not (tmp_path / 'out').exists() and not (tmp_path / 'o').exists() and not (tmp_path / 'x.png').exists()
