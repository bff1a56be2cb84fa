"""Front-layered tiles (container format 8) on the host: the cut rule (front_layer_cuts), the host coder restarted at the cuts over
the wavefront-ordered tables, the wavefront decoder's schedule with the restarts restated on flags, the container and its readers,
the options, and the C ABI of the two new entries as far as it goes without a device."""
import argparse
import ctypes
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from imgcomp_cvpr_amd import codec
from tests import codec_cases as cc
from tests.test_cpu_codec_layered import ENDS, HEAD, _file as _file6
from tests.test_cpu_codec_preview import SHAPES, _prototype
from tests.test_cpu_codec_wavefront import _front

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ends_variants(C):
    """the three of the layered GPU tests: [C], [1, 2, C] (what of it fits below C), one layer per channel"""
    out = [[C], sorted(set([1, min(2, C), C])), list(range(1, C + 1))]
    return [e for i, e in enumerate(out) if e not in out[:i]]


# ---- the cuts -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', SHAPES)
def test_cuts(shape):
    C, h, w = shape
    order = codec.wavefront_order(C, h, w)
    c, y, x = order // (h * w), (order // w) % h, order % w
    T = x + 2 * y + 4 * c
    for ends in _ends_variants(C):
        if len(ends) > codec.MAX_LAYERS:                                      # (32, 16, 16), a layer per channel: more than the format holds
            with pytest.raises(ValueError, match='layer count G = 32'):
                codec.front_layer_cuts(C, h, w, ends)
            continue
        cuts = codec.front_layer_cuts(C, h, w, ends)
        assert len(cuts) == len(ends) and all(isinstance(n, int) for n in cuts)
        assert all(a < b for a, b in zip(cuts, cuts[1:])) and cuts[0] >= 1 and cuts[-1] == C * h * w
        assert cuts == [codec.wavefront_prefix_count(C, h, w, e) for e in ends]
        for g, (lo, hi) in enumerate(zip([0] + cuts, cuts)):
            t_g = (w - 1) + 2 * (h - 1) + 4 * (ends[g] - 1)
            t_before = (w - 1) + 2 * (h - 1) + 4 * (ends[g - 1] - 1) if g else -1
            assert (T[lo:hi] > t_before).all() and (T[lo:hi] <= t_g).all()    # whole fronts: a cut never falls inside one
            assert (T[hi:] > t_g).all()
            assert set(np.flatnonzero(c < ends[g]).tolist()) <= set(range(hi))      # segments 0 .. g hold every symbol of the channels below e_g
            assert hi >= ends[g] * h * w
            empty = max(1, lo) == hi                                          # (index 0 is the uncoded first symbol)
            assert empty == (g == 0 and ends[0] == 1 and h == 1 and w == 1), (shape, ends, g)
    for bad, why in (([], 'G = 0'), ([C + 1], 'not C'), ([0, C], 'not increasing')):
        with pytest.raises(ValueError, match=why):
            codec.front_layer_cuts(C, h, w, bad)


def test_cuts_of_the_design():
    """the passenger table of the design: the symbols in the prefix at the default ends"""
    assert codec.front_layer_cuts(32, 16, 16, [4, 8, 16, 32]) == [2368, 3392, 5440, 8192]
    assert codec.front_layer_cuts(32, 8, 8, [4, 8, 16, 32]) == [400, 656, 1168, 2048]
    assert codec.front_layer_cuts(3, 1, 1, [1, 3]) == [1, 3]                  # e_0 = 1 on a 1 x 1 tile: the empty segment 0
    assert codec.front_layer_cuts(6, 4, 4, [1, 2, 6]) != codec.front_layer_cuts(6, 1, 3, [1, 2, 6])       # edge tiles: their own cuts


# ---- the host coder over the permuted tables, restarted at the cuts ---------------------------------------------------------------

def _host_front_segments(symbols, tabs, order, cuts):
    s, f = symbols[order], tabs[order]
    return [cc.host_encode(s[max(1, a):b], f[max(1, a):b])[0] for a, b in zip([0] + list(cuts), cuts)]


@pytest.mark.parametrize('shape', [(2, 1, 1), (5, 3, 4), (6, 5, 7), (3, 1, 9), (3, 9, 1)])
def test_host_coder_restarted_at_the_cuts(shape):
    C, h, w = shape
    n = C * h * w
    order = codec.wavefront_order(C, h, w)
    fill = 4
    for seed, gain in ((1, 1.0), (2, 12.0)):
        rs = np.random.RandomState(seed)
        tabs = cc.softmax_tables(np.maximum(rs.randn(n, 6) * gain, 0).astype(np.float32))
        sym = rs.randint(0, 6, size=n).astype(np.int64)
        whole = cc.host_encode(sym[order][1:], tabs[order][1:])[0]
        for ends in _ends_variants(C):
            cuts = codec.front_layer_cuts(C, h, w, ends)
            segs = _host_front_segments(sym, tabs, order, cuts)
            if len(ends) == 1:
                assert segs == [whole]                                        # G = 1 is the format-5 stream
            if shape == (2, 1, 1) and ends[0] == 1:
                assert segs[0] == b'\x80'
            got = np.full(n, fill, np.int64)
            got[0] = sym[0]
            for g, (a, b) in enumerate(zip([0] + cuts, cuts)):
                a = max(1, a)
                piece = cc.host_decode(segs[g], list(tabs[order][a:b]))
                assert cc.model_decode(segs[g], list(tabs[order][a:b])) == (piece, 0)
                got[order[a:b]] = piece
                # the segments 0 .. g alone: the preview of e_g on the channels below it
                vol = got.reshape(shape)
                assert np.array_equal(vol[:ends[g]], codec.preview_symbols(sym.reshape(shape), ends[g], fill)[:ends[g]]), (shape, ends, g)
            assert np.array_equal(got, sym)


@pytest.mark.parametrize('shape', [(2, 1, 1), (5, 3, 4), (6, 5, 7), (3, 1, 9), (3, 9, 1), (4, 1, 1), (32, 16, 16)])
def test_wavefront_schedule_with_restarts(shape):
    """pc_dec_wave_body<.., LIM, SEG> on flags instead of values: the loop of the wavefront decoder ended at T_stop(cdec), with the
    coder restarted when phase 4 first comes to a front above t_g.  Every cache voxel read was written once before; a restart falls
    between two fronts and exactly at the cut n_g of the stream's order; segment g gives the symbols order[n_{g-1}:n_g]; only the
    segments of layers that begin below cdec are opened, and cdec need not be a layer end."""
    C, h, w = shape
    other = [(0, a, b) for a in range(3) for b in range(3)] + [(1, 0, 0), (1, 0, 1), (1, 0, 2), (1, 1, 0), (1, 1, 1)]
    first = other[:13]
    full = codec.wavefront_order(C, h, w)
    variants = [e for e in _ends_variants(C) if len(e) <= codec.MAX_LAYERS] + ([[4, 8, 16, 32]] if C == 32 else [])
    for ends in variants:
        cuts = codec.front_layer_cuts(C, h, w, ends)
        for K in sorted(set([1, 2, max(C // 4, 1), C - 1, C] + ends) & set(range(1, C + 1))):
            V = np.ones((C + 4, h + 8, w + 8), bool)
            V[4:, 4:h + 4, 4:w + 4] = False
            A0, A1, A2 = np.zeros((C + 3, h + 6, w + 6), bool), np.zeros((C + 2, h + 4, w + 4), bool), np.zeros((C + 1, h + 2, w + 2), bool)
            T_base = (w - 1) + 2 * (h - 1) - 4 + 28
            seg_next, T_cut = 1, (T_base + 4 * ends[0] if len(ends) > 1 else 1 << 30)
            per_seg, steps = [[]], 0
            T_stop = (w + 3) + 2 * (h + 3) + 4 * (K + 3)
            for T in range(7, T_stop + 1):
                steps += 1
                for out, src, taps, back in ((A0, V, first, 7), (A1, A0, other, 14), (A2, A1, other, 21)):
                    todo = _front(T - back, *out.shape)
                    for d, i, j in todo:
                        assert not out[d, i, j] and all(src[d + a, i + b, j + c] for a, b, c in taps), (K, T, d, i, j)
                        assert out is not A2 or A0[d + 2, i + 2, j + 2]
                    for v in todo:
                        out[v] = True
                if T > T_cut:                                                 # the restart: before this front's first symbol
                    assert sum(len(p) for p in per_seg) == cuts[seg_next - 1], (shape, ends, K, T)
                    per_seg.append([])
                    seg_next += 1
                    T_cut = T_base + 4 * ends[seg_next - 1] if seg_next < len(ends) else 1 << 30
                todo = _front(T - 28, C, h, w)
                for c, y, x in todo:
                    assert not V[c + 4, y + 4, x + 4] and all(A2[c + a, y + b, x + k] for a, b, k in other), (K, T, c, y, x)
                for c, y, x in todo:
                    V[c + 4, y + 4, x + 4] = True
                    per_seg[-1].append((c * h + y) * w + x)
            n = codec.wavefront_prefix_count(C, h, w, K)
            opened = [g for g in range(len(ends)) if g == 0 or ends[g - 1] < K]
            assert list(range(len(per_seg))) == opened, (shape, ends, K)      # the layers that begin below K, no other
            for g, got in enumerate(per_seg):
                lo, hi = ([0] + cuts)[g], min(cuts[g], n)
                assert np.array_equal(np.array(got, np.int64), full[lo:hi]), (shape, ends, K, g)
            assert V[4:K + 4, 4:h + 4, 4:w + 4].all()
            assert steps == (w + 3) + 2 * (h + 3) + 4 * (C + 3) - 6 - 4 * (C - K)
            if shape == (32, 16, 16) and ends == [4, 8, 16, 32] and K in ends:
                assert steps == {4: 79, 8: 95, 16: 127, 32: 191}[K]           # the step arithmetic of the design


# ---- the container ------------------------------------------------------------------------------------------------------------

def _file8(ends=ENDS, seed=3, head=HEAD):
    """the format-8 file of the fields of test_cpu_codec_layered._file -> (bytes, the format-6 file of the same fields, segments, firsts)"""
    six, segments, firsts = _file6(ends=ends, seed=seed, head=head)
    args = [head[k] for k in ('ae_name', 'pc_name', 'H', 'W', 'C', 'h', 'w', 'L', 'resolution', 'fingerprint', 'th', 'tw')]
    return codec.build_front_layered_container(*(args + [firsts, ends, segments])), six, segments, firsts


def _with_version(data, v):
    cut = codec.layer_prefix_bytes(data, 0) - 4
    head = data[:4] + struct.pack('<H', v) + data[6:cut]
    body = head + struct.pack('<I', zlib.crc32(head) & 0xffffffff) + data[cut + 4:-4]
    return body + struct.pack('<I', zlib.crc32(body) & 0xffffffff)


def test_round_trip_and_layout():
    data, six, segments, firsts = _file8()
    c, c6 = codec.parse_container(data), codec.parse_container(six)
    assert isinstance(c, codec.LayeredContainer) and isinstance(c, codec._TILED) and c.version == 8 == codec.FORMAT_VERSION_FRONTS
    assert c6.version == 6 and c[1:] == c6[1:]                                # only the version word tells them apart
    assert c.layer_ends == ENDS and c.segments == segments and c.first_syms == firsts
    assert c.streams == [[segments[g][t] for g in range(3)] for t in range(4)]
    assert data == _with_version(six, 8) and len(data) == len(six)            # the bytes of format 6 with version 8
    assert data[6:codec.layer_prefix_bytes(data, 0) - 4] == six[6:codec.layer_prefix_bytes(six, 0) - 4]
    one = _file8(ends=[8])[0]
    assert codec.parse_container(one).layer_ends == [8] and codec.parse_container(one).version == 8


def test_every_flip_and_every_truncation_is_refused():
    data = _file8()[0]
    for i in range(len(data)):
        bad = bytearray(data)
        bad[i] ^= 1 << (i % 8)
        with pytest.raises(ValueError, match='magic|version|CRC|truncated'):
            codec.parse_container(bytes(bad))
    for n in range(len(data)):
        with pytest.raises(ValueError, match='magic|version|CRC|truncated'):
            codec.parse_container(data[:n])


def test_versions():
    data, six, _, _ = _file8()

    def resealed(v):
        body = data[:4] + struct.pack('<H', v) + data[6:-4]
        return body + struct.pack('<I', zlib.crc32(body) & 0xffffffff)
    # the sentences the existing tests pin still match; the sentence has only grown at its end
    with pytest.raises(ValueError, match=r'unsupported format version 3 \(this codec reads versions 1, 2 and 4\) and the wavefront version 5'):
        codec.parse_container(resealed(3))
    with pytest.raises(ValueError, match=r'unsupported format version 7 .* and the layered version 6 and the front-layered version 8$'):
        codec.parse_container(resealed(7))
    for v in (0, 3, 7, 9):
        with pytest.raises(ValueError, match='unsupported format version {}'.format(v)):
            codec.parse_container(resealed(v))
    for v in (0, 3, 4, 5, 7):
        with pytest.raises(ValueError, match='header damaged: format version {} is not the layered version 6: only a layered file'.format(v)):
            codec.parse_partial(resealed(v))
        with pytest.raises(ValueError, match='header damaged: format version {} is not the layered version 6'.format(v)):
            codec.layer_prefix_bytes(resealed(v), 1)
    for v in (0, 3, 7):
        with pytest.raises(ValueError, match='header damaged: format version {} is not the layered version 6'.format(v)):
            codec.parse_recover(resealed(v))
    for v in (4, 5):
        with pytest.raises(ValueError, match=r'--salvage.*decompress'):
            codec.parse_recover(resealed(v))
    with pytest.raises(ValueError, match='unsupported format version 7'):
        codec.parse_salvage(resealed(7))
    with pytest.raises(ValueError, match='format version 8 .* is not salvaged: salvage of layered files is out of scope'):
        codec.parse_salvage(data)


def test_readers_read_it_as_format_6():
    data, six, segments, _ = _file8()
    bounds = [codec.layer_prefix_bytes(data, g) for g in range(4)]
    assert bounds == [codec.layer_prefix_bytes(six, g) for g in range(4)] == [codec.layer_prefix_bytes(codec.parse_container(data), g) for g in range(4)]
    for n in sorted(set(bounds + [b - 1 for b in bounds] + [b + 1 for b in bounds] + [len(data), len(data) - 1, 40])):
        if n < bounds[0]:
            for read in (codec.parse_partial, codec.parse_recover):
                with pytest.raises(ValueError, match='header damaged'):
                    read(data[:n])
            continue
        (c, complete, ok), (c6, complete6, ok6) = codec.parse_partial(data[:n]), codec.parse_partial(six[:n])
        assert c.version == 8 and c[1:] == c6[1:] and (complete, ok) == (complete6, ok6), n
        (c, layers, reasons, ok), (c6, layers6, reasons6, ok6) = codec.parse_recover(data[:n]), codec.parse_recover(six[:n])
        assert c.version == 8 and c[1:] == c6[1:] and (layers, reasons, ok) == (layers6, reasons6, ok6), n
    for g in range(3):                                                        # a flipped byte in a segment
        for t in range(4):
            pos = bounds[g] + sum(len(b) for b in segments[g][:t]) + len(segments[g][t]) // 2
            bad, bad6 = bytearray(data), bytearray(six)
            bad[pos] ^= 0x40
            bad6[pos] ^= 0x40
            assert codec.parse_partial(bytes(bad))[1:] == codec.parse_partial(bytes(bad6))[1:] == (g, False)
            assert codec.parse_recover(bytes(bad))[1:] == codec.parse_recover(bytes(bad6))[1:]
            assert codec.parse_recover(bytes(bad))[2] == {t: 'crc'}
    ok, text = codec.verify_file(data)
    assert ok and 'format 8' in text and 'G = 3' in text and 'ends 1,2,8' in text
    assert 'prefix lengths ' + ','.join(str(b) for b in bounds) in text
    ok, text = codec.verify_file(data[:bounds[2]])
    assert not ok and '2 of 3 layers complete' in text


class _NoModel(object):
    def _recover_head(self, data):
        return codec.parse_recover(data)


def test_stream_refuses_it():
    data = _file8()[0]
    dec = codec.StreamDecoder(_NoModel())
    assert dec.feed(data[:5]) is False
    with pytest.raises(ValueError, match=r'format version 8 .* is not streamed.*--recover'):
        dec.feed(data[5:6])
    with pytest.raises(ValueError, match=r'format version 8 .* is not streamed.*--recover'):
        codec.StreamDecoder(_NoModel()).feed(data)
    with pytest.raises(ValueError, match='--recover'):
        codec.stream_header_bytes(data)
    assert codec.stream_header_bytes(_file8()[1]) == codec.layer_prefix_bytes(data, 0)      # format 6 streams as before


def test_model_checks():
    class _Pred(object):
        freqs_resolution = 1e9
    shell = codec.Codec.__new__(codec.Codec)
    shell.ae_name, shell.pc_name, shell.fingerprint, shell.C, shell.L, shell.factor, shell.pred = 'cvpr/low', 'cvpr/res_shallow', 0x1234abcd, 8, 6, 8, _Pred()
    shell.wavefront_refusal = shell.layered_refusal = None
    c = codec.parse_container(_file8()[0])
    shell.check_container(c)
    shell.layered_refusal = 'layered tiles: k = 64'
    with pytest.raises(ValueError, match='format 8 cannot be read with this model: layered tiles'):
        shell.check_container(c)
    shell.layered_refusal, shell.wavefront_refusal = None, 'wavefront order: k = 64'
    with pytest.raises(ValueError, match='format 8 cannot be read with this model: wavefront order'):
        shell.check_container(c)
    shell.check_container(codec.parse_container(_file8()[1]))                 # format 6 does not ask for the wavefront order


# ---- options ------------------------------------------------------------------------------------------------------------------

def _flags(command, **kw):
    base = dict(command=command, tile=None, checked=False, wavefront=False, salvage=False, channels=None, layers=None, progressive=False,
                front_layers=None, front_progressive=False, partial=False, recover=False, chunk=None, batch=8)
    base.update(kw)
    return argparse.Namespace(**base)


def test_option_clashes():
    for command in ('compress', 'compress-dir'):
        codec.check_option_args(_flags(command, tile=128, front_layers='4,8,16,32'))
        codec.check_option_args(_flags(command, tile=128, front_progressive=True))
        codec.check_option_args(_flags(command, tile=128, front_layers='32'))
        codec.check_option_args(_flags(command, tile=128, front_progressive=True, checked=True))      # as --layers: the checksums are there anyway
    for command in ('decompress', 'decompress-dir'):                          # reading needs no option
        for kw in (dict(), dict(channels=4), dict(partial=True), dict(recover=True)):
            codec.check_option_args(_flags(command, **kw))
    for flags, why in ((_flags('compress', front_layers='4,32'), '--front-layers needs --tile'),
                       (_flags('compress-dir', front_progressive=True), '--front-progressive needs --tile'),
                       (_flags('compress', tile=128, front_layers='4,32', wavefront=True), '--front-layers does not go with --wavefront'),
                       (_flags('compress-dir', tile=128, front_progressive=True, wavefront=True), '--front-progressive does not go with --wavefront'),
                       (_flags('compress', tile=128, front_layers='4,32', layers='4,32'), '--front-layers does not go with --layers'),
                       (_flags('compress', tile=128, front_layers='4,32', progressive=True), '--front-layers does not go with --progressive'),
                       (_flags('compress', tile=128, front_progressive=True, layers='4,32'), '--front-progressive does not go with --layers'),
                       (_flags('compress', tile=128, front_progressive=True, progressive=True), '--front-progressive does not go with --progressive'),
                       (_flags('compress', tile=128, front_layers='4,32', front_progressive=True), '--front-layers does not go with --front-progressive'),
                       (_flags('decompress', front_layers='4,32'), '--front-layers belongs to compress'),
                       (_flags('decompress-dir', front_progressive=True), '--front-progressive belongs to compress'),
                       (_flags('stream', front_progressive=True), '--front-progressive belongs to compress'),
                       (_flags('compress', tile=128, front_layers='4,x'), r"--front-layers '4,x' is not a comma-separated list of integers"),
                       (_flags('compress', tile=128, front_layers='8,4'), '--front-layers .*increasing'),
                       (_flags('compress', tile=128, front_layers='0,4'), '--front-layers .*increasing'),
                       # what was refused before stays refused, in its words
                       (_flags('compress', tile=128, layers='4,32', wavefront=True), '--layers does not go with --wavefront: a layer is no prefix'),
                       (_flags('compress', tile=128, layers='4,x'), r"--layers '4,x' is not a comma-separated")):
        with pytest.raises(ValueError, match=why):
            codec.check_option_args(flags)
    old = argparse.Namespace(command='compress', tile=128, checked=False, wavefront=True, salvage=False, channels=None)
    codec.check_option_args(old)                                              # a namespace without the keys reads as no option
    assert codec._front_layers_option(_flags('compress', tile=128, front_layers='4,32'), 32) == [4, 32]
    assert codec._front_layers_option(_flags('compress', tile=128, front_progressive=True), 32) == 'default'
    assert codec._front_layers_option(_flags('compress', tile=128), 32) is None
    with pytest.raises(ValueError, match='not C = 32'):
        codec._front_layers_option(_flags('compress', tile=128, front_layers='4,31'), 32)


def test_command_line_refuses_before_any_model(tmp_path, capsys):
    src = tmp_path / 'a.png'
    src.write_bytes(b'x')
    for extra, why in ((['--front-progressive'], '--front-progressive needs --tile'),
                       (['--tile', '32', '--front-layers', '4,32', '--wavefront'], '--front-layers does not go with --wavefront'),
                       (['--tile', '32', '--front-progressive', '--progressive'], '--front-progressive does not go with --progressive'),
                       (['--tile', '32', '--front-layers', '4,31'], 'not C = 32')):
        assert codec.main(['compress', str(src), str(tmp_path / 'a.icf'), '--device', 'no-such-device'] + extra) == 2, extra
        assert why in capsys.readouterr().err
    assert not (tmp_path / 'a.icf').exists()


def test_codec_keyword_refusals():
    """decided before any model is built: a call without configs or weights gets that far"""
    for kw, why in ((dict(front_layers='default'), 'front_layers needs a tile extent'),
                    (dict(front_layers=[4, 32]), 'front_layers needs a tile extent'),
                    (dict(tile=(4, 4), front_layers='default', layers='default'), 'front_layers does not go with layers'),
                    (dict(tile=(4, 4), front_layers=[4, 32], layers=[4, 32]), 'front_layers does not go with layers'),
                    (dict(tile=(4, 4), front_layers='default', order='wavefront'), "front_layers does not go with order='wavefront'"),
                    (dict(tile=(4, 4), front_layers='other'), "'default' or a sequence of layer ends"),
                    (dict(tile=(4, 4), layers='default', order='wavefront'), 'a layer is no prefix of a wavefront-ordered stream')):
        with pytest.raises(ValueError, match=why):
            codec.Codec(None, None, None, **kw)

    class _Cfg(object):
        num_chan_bn = 32
    with pytest.raises(ValueError, match='not C = 32'):
        codec.Codec(_Cfg(), None, None, tile=(4, 4), front_layers=[4, 31])
    # the attributes set after construction, as main does: the same refusals when compress asks
    shell = codec.Codec.__new__(codec.Codec)
    shell.C, shell.wavefront_refusal, shell.layered_refusal = 32, None, None
    shell.tile, shell.order, shell.layers, shell.front_layers = (4, 4), 'raster', None, 'default'
    assert shell._front_ends() == [4, 8, 16, 32]
    shell.front_layers = [1, 32]
    assert shell._front_ends() == [1, 32]
    shell.front_layers = None
    assert shell._front_ends() is None
    for attrs, why in ((dict(tile=None), 'needs a tile extent'), (dict(layers='default'), 'does not go with layers'),
                       (dict(order='wavefront'), "does not go with order='wavefront'"), (dict(front_layers=[4, 31]), 'not C = 32'),
                       (dict(wavefront_refusal='wavefront order: no'), 'wavefront order: no'), (dict(layered_refusal='layered tiles: no'), 'layered tiles: no')):
        shell.tile, shell.order, shell.layers, shell.front_layers = (4, 4), 'raster', None, 'default'
        shell.wavefront_refusal = shell.layered_refusal = None
        for k, v in attrs.items():
            setattr(shell, k, v)
        with pytest.raises(ValueError, match=why):
            shell._front_ends()


def test_prediction_network_keyword_refusals():
    from imgcomp_cvpr_amd import probclass
    pred = probclass.PredictionNetwork.__new__(probclass.PredictionNetwork)
    vols = [([[b'', b'']], [0], (2, 1, 1))]
    for kw in (dict(front_ends=[1, 2], layer_ends=[1, 2]), dict(front_ends=[1, 2], order='wavefront')):
        with pytest.raises(ValueError, match='front_ends cuts the wavefront order at fronts by itself'):
            pred.decode_tiles_batch(vols, 1, 1, **kw)
        with pytest.raises(ValueError, match='front_ends cuts the wavefront order at fronts by itself'):
            pred.encode_tiles(np.zeros((2, 1, 1), np.int64), 1, 1, **kw)
        with pytest.raises(ValueError, match='front_ends cuts the wavefront order at fronts by itself'):
            pred.encode_tiles_batch([np.zeros((2, 1, 1), np.int64)], 1, 1, **kw)
    with pytest.raises(ValueError, match='conceal'):
        pred.decode_tiles_batch(vols, 1, 1, front_ends=[1, 2], conceal=True)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------

PAIRS = (('ic_pc_decode_tiles_batch_layers_f32', 'ic_pc_decode_tiles_batch_fronts_f32'),
         ('ic_pc_decode_tiles_batch_layers_pertile_f32', 'ic_pc_decode_tiles_batch_fronts_pertile_f32'),
         ('ic_pc_decode_tiles_batch_layers_workspace_bytes', 'ic_pc_decode_tiles_batch_fronts_workspace_bytes'),
         ('ic_pc_decode_tiles_batch_layers_pertile_workspace_bytes', 'ic_pc_decode_tiles_batch_fronts_pertile_workspace_bytes'))


def test_new_entries_header_bindings_exports():
    from imgcomp_cvpr_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'imgcomp_hip.h')).read(), flags=re.S)
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    exported = set(re.findall(r' T (ic_[a-z0-9_]+)', out))
    for parent, new in PAIRS:
        assert _prototype(text, new) == _prototype(text, parent), new         # argument for argument
        pr, pa = _lib.PROTOTYPES[parent]
        nr, na = _lib.PROTOTYPES[new]
        assert nr is pr and list(na) == list(pa) and len(na) == len(_prototype(text, new)), new
        assert new in exported and parent in exported
        assert getattr(_lib.lib, new).argtypes == list(na)
    assert _lib.lib.ic_abi_version() == 2


def test_workspace_sizes_are_the_layered_entries():
    from imgcomp_cvpr_amd import _lib
    lib = _lib.lib
    good = ((32, 16, 16, 24, 1, 24, 4), (6, 4, 4, 4, 1, 24, 3), (8, 4, 3, 8, 2, 24, 16), (32, 16, 16, 1000, 7, 24, 1), (1, 1, 1, 1, 1, 24, 1))
    bad = ((32, 16, 16, 24, 1, 24, 0), (32, 16, 16, 24, 1, 24, 17), (32, 16, 16, 0, 1, 24, 4), (32, 16, 16, 24, 0, 24, 4), (0, 16, 16, 24, 1, 24, 4))
    for args in good + bad:                                                   # the tuples of test_cpu_codec_resume.test_workspace_size
        a, b = int(lib.ic_pc_decode_tiles_batch_fronts_workspace_bytes(*args)), int(lib.ic_pc_decode_tiles_batch_layers_workspace_bytes(*args))
        c, d = int(lib.ic_pc_decode_tiles_batch_fronts_pertile_workspace_bytes(*args)), int(lib.ic_pc_decode_tiles_batch_layers_pertile_workspace_bytes(*args))
        assert a == b and c == d and (a > 0) == (args in good) and (c > a or args in bad), args


def _host_call(entry, per, ends=(1, 2, 6), limit=6, limits=None, segs=None, flags=0, k=24, L=6, fill=0, ws_bytes=None, ntiles=1, nlayers=None,
               tile=(0, 0, 4, 4, 0, 0, 0, 0), total=100):
    """one of the two entries with host tables that are real and device pointers that are not: every refusal is decided on the host,
    before any device call, so nothing is dereferenced.  The workspace size is 0 unless given: the size check is the last of the
    host's, so a call that none of the earlier checks stops returns IC_ERR_WORKSPACE and still reaches no device."""
    from imgcomp_cvpr_amd import _lib
    lib = _lib.lib
    G = len(ends)
    fake = ctypes.c_void_p(0x1000)
    tab = (_lib.c_void_p * 8)(*([0x1000] * 8))
    table = _lib.tile_table([tile] * ntiles)
    vtable = _lib.volume_table([(5, 7, 0, 0)])
    seg_table = _lib.seg_table(list(segs) if segs is not None else [(0, 10)] * (G * ntiles))
    host_ends = (ctypes.c_int * max(G, 1))(*ends)
    nl = G if nlayers is None else nlayers
    head = (fake, total, table, ntiles, vtable, 1, tab, fake, k, L, 1e9, fake, fake, fake, 6, fake, 0 if ws_bytes is None else ws_bytes,
            flags, None)
    if per:
        host_limits = (ctypes.c_int * ntiles)(*(limits if limits is not None else [limit] * ntiles))
        return getattr(lib, entry)(*(head + (host_limits, fill, host_ends, nl, seg_table)))
    return getattr(lib, entry)(*(head + (limit, fill, host_ends, nl, seg_table)))


@pytest.mark.parametrize('entry,per', [('ic_pc_decode_tiles_batch_fronts_f32', False), ('ic_pc_decode_tiles_batch_fronts_pertile_f32', True)])
def test_host_side_refusals_need_no_device(entry, per):
    from imgcomp_cvpr_amd import _lib
    ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
    call = lambda **kw: _host_call(entry, per, **kw)
    for bad in ((2, 2, 6), (0, 2, 6), (1, 2, 5), (1, 2, 7), (2, 1, 6)):
        assert call(ends=bad) == ARG, bad
    for nl in (0, 17, -1):
        assert call(nlayers=nl) == ARG, nl
    for K in (0, 7, -1):
        assert call(limit=K) == ARG, K
    assert call(fill=6) == ARG and call(fill=-1) == ARG
    for seg in ((99, 2), (-1, 1), (0, -1), (101, 0)):                         # a segment outside [0, total_bytes)
        assert call(segs=[(0, 10), (0, 10), seg]) == ARG, seg
        assert call(segs=[seg, (0, 10), (0, 10)], limit=1) == ARG, seg        # segment 0 is always read
        assert call(segs=[(0, 10), (0, 10), seg], limit=2, ws_bytes=0) == WORKSPACE, seg      # layer 2 begins at 2: not looked at, the next check speaks
    assert call(tile=(0, 0, 4, 4, 0, 0, 6, 0)) == ARG                         # first symbol not below L
    assert call(tile=(3, 0, 4, 4, 0, 0, 0, 0)) == ARG                         # a tile outside its 5 x 7 volume
    for flags in (_lib.PC_DECODE_WAVEFRONT, _lib.PC_DECODE_RECOMPUTE, _lib.PC_DECODE_PER_LAYER):
        assert call(flags=flags) == UNSUPPORTED, flags                        # the order is the entry's own: flags is 0
    assert call(k=64) == UNSUPPORTED and call(L=17) == UNSUPPORTED
    need = int(getattr(_lib.lib, entry.replace('_f32', '_workspace_bytes'))(6, 4, 4, 1, 1, 24, 3))
    assert need > 0 and call(ws_bytes=need - 1) == WORKSPACE and call() == WORKSPACE      # (the latter: every earlier check passes)
    if per:
        assert call(ntiles=2, limits=[6, 0]) == ARG and call(ntiles=2, limits=[7, 1]) == ARG
        assert call(ntiles=2, limits=[1, 2], segs=[(0, 10), (101, 0), (101, 0), (0, 10), (0, 10), (-1, 1)], ws_bytes=0) == WORKSPACE
        assert call(ntiles=2, limits=[1, 2], segs=[(0, 10), (101, 0), (101, 0), (0, 10), (-1, 1), (0, 10)], ws_bytes=0) == ARG
