"""Recovery of layered files (container format 6) on the host: the NumPy statement of the per-(tile, channel) concealment rule
against the whole-tile rule, the reader that counts every tile's leading intact segments (parse_recover), the options."""
import argparse
import struct

import numpy as np
import pytest

from imgcomp_cvpr_amd import codec
from tests import conceal_rule as R
from tests import recover_rule as RR
from tests.test_cpu_codec_layered import ENDS, HEAD, _file


# ---- the rule ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape,th,tw', [((6, 5, 7), 4, 4), ((3, 9, 9), 3, 3)])
def test_rule_with_whole_tiles_is_the_conceal_rule(shape, th, tw):
    C, L = shape[0], 6
    rs = np.random.RandomState(sum(shape))
    nt = len(R.grid(shape[1], shape[2], th, tw))
    sets = [[], list(range(nt)), [0], [nt - 1], [nt // 2]] + [sorted(rs.choice(nt, size=int(rs.randint(1, nt)), replace=False).tolist()) for _ in range(12)]
    for damaged in sets:
        sym = rs.randint(0, L, size=shape).astype(np.int64)
        sym[1] = rs.randint(0, 2, size=shape[1:]) * (L - 1)                   # few distinct symbols: the vote is a decision, ties happen
        have = [0 if t in damaged else C for t in range(nt)]
        assert np.array_equal(RR.conceal_channels(sym, have, th, tw, L, 2), R.conceal(sym, damaged, th, tw, L, 2)), damaged


def test_rule_per_channel():
    L, C = 6, 4
    sym = np.random.RandomState(5).randint(0, L, size=(C, 3, 9)).astype(np.int64)       # three 3 x 3 tiles in a row
    sym[:, :, 2] = 1                                                          # tile 0's right column
    sym[:, :, 6] = 4                                                          # tile 2's left column
    got = RR.conceal_channels(sym, [3, 1, 2], 3, 3, L, 5)
    assert np.array_equal(got[:1], sym[:1]) and np.array_equal(got[:, :, :3][:3], sym[:, :, :3][:3])      # what a tile holds stays
    assert (got[1, :, 3:6] == 1).all()                                        # channel 1: both neighbours hold it, 3 : 3, the smaller symbol
    assert (got[2, :, 3:6] == 1).all()                                        # channel 2: tile 0 alone
    assert (got[3, :, 3:6] == 5).all() and (got[3] == 5).all()                # channel 3: nobody
    assert (got[2, :, 6:] == 5).all()                                         # tile 2's only neighbour lacks channel 2 itself
    sym2 = sym.copy()
    sym2[:, :, 3:6] = 0                                                       # what stands in a tile's missing channels is never read
    sym2[0, :, 3:6] = sym[0, :, 3:6]
    assert np.array_equal(RR.conceal_channels(sym2, [3, 1, 2], 3, 3, L, 5), got)
    assert np.array_equal(RR.conceal_channels(sym, [4, 4, 4], 3, 3, L, 5), sym)
    same = RR.recover(sym, [2, 2, 2], 3, 3, L, 5)                             # all tiles stop at one K: the preview
    assert np.array_equal(same, codec.preview_symbols(sym, 2, 5))
    assert np.array_equal(RR.preview_per_tile(sym, [4, 0, 1], 3, 3, 5)[:, :, 3:6], np.full((C, 3, 3), 5))


# ---- the reader -------------------------------------------------------------------------------------------------------------

G, NT = len(ENDS), 4


def _seg_start(data, segments, g, t):
    return codec.layer_prefix_bytes(data, g) + sum(len(b) for b in segments[g][:t])


def test_parse_recover_intact():
    data, segments, firsts = _file()
    c, layers, reasons, ok = codec.parse_recover(data)
    assert isinstance(c, codec.LayeredContainer) and c == codec.parse_container(data)
    assert layers == [G] * NT and reasons == {} and ok is True
    c, layers, reasons, ok = codec.parse_recover(data[:-1])                   # the CRC over the file alone is cut
    assert layers == [G] * NT and reasons == {} and ok is False
    assert codec.parse_recover(data + b'tail')[1:] == ([G] * NT, {}, True)    # bytes behind the declared end are ignored


def test_parse_recover_cut_files():
    data, segments, _ = _file()
    for g in range(G + 1):                                                    # at a layer end: every tile holds g layers
        c, layers, reasons, ok = codec.parse_recover(data[:codec.layer_prefix_bytes(data, g)])
        assert layers == [g] * NT and ok is False
        assert reasons == ({} if g == G else {t: 'truncated' for t in range(NT)})
        assert [[b is not None for b in layer] for layer in c.segments] == [[gg < g] * NT for gg in range(G)]
        assert codec.parse_partial(data[:codec.layer_prefix_bytes(data, g)])[1] == g
    for g, t in ((1, 2), (0, 0), (2, 3), (1, 0)):                             # inside layer g: the tiles in front of the cut hold it
        a = _seg_start(data, segments, g, t)
        b = a + len(segments[g][t])
        for n in (a + 1, b - 1) if b - a > 1 else (a,):
            c, layers, reasons, ok = codec.parse_recover(data[:n])
            assert layers == [g + 1] * t + [g] * (NT - t), (g, t, n)
            assert reasons == {u: 'truncated' for u in range(NT)} if g + 1 < G else reasons == {u: 'truncated' for u in range(t, NT)}
            assert ok is False and codec.parse_partial(data[:n])[1] == g
        assert codec.parse_recover(data[:b])[1] == [g + 1] * (t + 1) + [g] * (NT - t - 1)


def test_parse_recover_flipped_bytes():
    data, segments, _ = _file()
    for g, t in ((0, 0), (1, 2), (2, 1), (0, 3)):
        bad = bytearray(data)
        bad[_seg_start(data, segments, g, t) + len(segments[g][t]) // 2] ^= 0x10
        c, layers, reasons, ok = codec.parse_recover(bytes(bad))
        assert layers == [g if u == t else G for u in range(NT)] and reasons == {t: 'crc'} and ok is False
        # the later layers of that tile are intact in the file -- and dropped: they cannot be decoded behind a missing one
        assert all(c.segments[gg][t] == segments[gg][t] for gg in range(G) if gg != g) and c.segments[g][t] is None
        assert codec.parse_partial(bytes(bad))[1] == g
    two = bytearray(data)
    two[_seg_start(data, segments, 1, 1)] ^= 1
    two[_seg_start(data, segments, 0, 1)] ^= 1                                # the reason is the FIRST bad segment's
    cut = bytes(two[:_seg_start(data, segments, 2, 2) + 1]) if len(segments[2][2]) > 1 else bytes(two[:_seg_start(data, segments, 2, 2)])
    c, layers, reasons, ok = codec.parse_recover(cut)
    assert layers == [3, 0, 2, 2] and reasons == {1: 'crc', 2: 'truncated', 3: 'truncated'}


def test_parse_recover_refusals():
    data, _, firsts = _file()
    head_end = codec.layer_prefix_bytes(data, 0)
    for n in (0, 5, 40, head_end - 1):
        with pytest.raises(ValueError, match='header damaged'):
            codec.parse_recover(data[:n])
    for pos in (7, head_end - 20, head_end - 2):
        bad = bytearray(data)
        bad[pos] ^= 0x01
        with pytest.raises(ValueError, match='header damaged'):
            codec.parse_recover(bytes(bad))
    with pytest.raises(ValueError, match='header damaged'):
        codec.parse_recover(b'XXXX' + data[4:])
    args = [HEAD[k] for k in ('ae_name', 'pc_name', 'H', 'W', 'C', 'h', 'w', 'L')]
    tail = [HEAD[k] for k in ('resolution', 'fingerprint')]
    others = [codec.build_container(*(args + [0] + tail + [b'abc']))] + \
             [build(*(args + tail + [4, 4, firsts, [b'ab'] * NT]))
              for build in (codec.build_tiled_container, codec.build_checked_container, codec.build_wavefront_container)]
    assert [struct.unpack('<H', d[4:6])[0] for d in others] == [1, 2, 4, 5]
    for d in others:
        codec.parse_container(d)
        with pytest.raises(ValueError, match=r'--salvage.*decompress'):
            codec.parse_recover(d)
    with pytest.raises(ValueError, match='out of scope'):                     # the salvage reader keeps refusing format 6
        codec.parse_salvage(data)


def _flags(command, **kw):
    base = dict(command=command, tile=None, checked=False, wavefront=False, salvage=False, channels=None, layers=None, progressive=False,
                partial=False, recover=False)
    base.update(kw)
    return argparse.Namespace(**base)


def test_option_clashes():
    codec.check_option_args(_flags('decompress', recover=True))
    codec.check_option_args(_flags('decompress-dir', recover=True))
    for flags, why in ((_flags('compress', recover=True), '--recover belongs to decompress'),
                       (_flags('compress-dir', tile=128, recover=True), '--recover belongs to decompress'),
                       (_flags('decompress', recover=True, salvage=True), '--recover does not go with --salvage'),
                       (_flags('decompress', recover=True, partial=True), '--recover does not go with --partial'),
                       (_flags('decompress-dir', recover=True, channels=4), '--recover does not go with --channels')):
        with pytest.raises(ValueError, match=why):
            codec.check_option_args(flags)
    old = argparse.Namespace(command='decompress', tile=None, checked=False, wavefront=False, salvage=True, channels=None)
    codec.check_option_args(old)                                              # a namespace without the key reads as no --recover
    report = codec.RecoverReport(4, 4, False, [codec.RecoveredTile(2, 1, 4, 'crc', (4, 0, 1, 4), (28, 0, 8, 32))])
    line = codec._recover_line('a.icf', report)
    assert 'a.icf: recovered, 1 of 4 tiles incomplete: tile 2 (crc) layers 1 of 4 = 4 channels, pixels y 28..36 x 0..32' in line
    assert line.endswith('the CRC over the file is missing or wrong')
    assert codec._recover_line('a.icf', codec.RecoverReport(4, 4, True, [])) == 'a.icf: recovered, all 4 tiles hold all 4 layers'
