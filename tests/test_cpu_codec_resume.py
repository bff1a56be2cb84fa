"""A layered decode that goes on where the last call stopped, on the host: the plan per tile (resume_plan), the options of the `stream`
command, what StreamDecoder.feed says about the bytes before any device is asked, the size of the resumable entry's workspace."""
import argparse
import struct

import pytest

from imgcomp_cvpr_amd import codec
from tests.test_cpu_codec_layered import ENDS, HEAD, _file

ENDS32 = [4, 8, 16, 32]


# ---- the plan -----------------------------------------------------------------------------------------------------------------

def test_resume_plan():
    # no progress: from == to, nothing is decoded; a whole tile says so with from == G
    assert [codec.resume_plan(g, g, ENDS32) for g in range(1, 5)] == [(1, 4), (2, 8), (3, 16), (4, 32)]
    # 0 -> g: the fresh start, up to the end of layer g - 1
    assert [codec.resume_plan(0, g, ENDS32) for g in range(1, 5)] == [(0, 4), (0, 8), (0, 16), (0, 32)]
    # mixed progress: every tile of a launch by itself
    done, now = [1, 2, 0, 3, 4, 2], [2, 4, 1, 3, 4, 3]
    assert [codec.resume_plan(d, n, ENDS32) for d, n in zip(done, now)] == [(1, 8), (2, 32), (0, 4), (3, 16), (4, 32), (2, 16)]
    # a restart after a decoder failure: the session has put the tile back to 0 layers done
    assert codec.resume_plan(0, 3, ENDS32) == (0, 16)
    # layers taken back: what the slot holds above them is of no use
    assert codec.resume_plan(3, 1, ENDS32) == (0, 4) and codec.resume_plan(4, 3, ENDS32) == (0, 16)
    # nothing there: the tile stays out of the launch
    assert codec.resume_plan(0, 0, ENDS32) == (0, 0) and codec.resume_plan(2, 0, ENDS32) == (0, 0)
    # ends of one plane, and a single layer
    one = list(range(1, 9))
    assert [codec.resume_plan(g, g + 1, one) for g in range(8)] == [(g, g + 1) for g in range(8)]
    assert codec.resume_plan(2, 7, one) == (2, 7) and codec.resume_plan(8, 8, one) == (8, 8)
    assert codec.resume_plan(0, 1, [32]) == (0, 32) and codec.resume_plan(1, 1, [32]) == (1, 32)
    # what the entry asks of every pair: 0 <= from <= G, cfrom <= channels <= C
    for ends in (ENDS32, one, [32], [1, 2, 8]):
        G = len(ends)
        for d in range(G + 1):
            for n in range(1, G + 1):
                g_from, channels = codec.resume_plan(d, n, ends)
                assert 0 <= g_from <= G and (ends[g_from - 1] if g_from else 0) <= channels <= ends[-1] and channels == ends[n - 1]
    for d, n in ((-1, 1), (5, 1), (1, 5), (1, -1)):
        with pytest.raises(ValueError, match='resume plan'):
            codec.resume_plan(d, n, ENDS32)


# ---- the options --------------------------------------------------------------------------------------------------------------

def _flags(command, **kw):
    base = dict(command=command, tile=None, checked=False, wavefront=False, salvage=False, channels=None, layers=None, progressive=False,
                partial=False, recover=False, chunk=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_option_clashes():
    codec.check_option_args(_flags('stream'))
    codec.check_option_args(_flags('stream', chunk=1))
    codec.check_option_args(_flags('stream', chunk=1 << 20))
    for command in ('compress', 'decompress', 'compress-dir', 'decompress-dir'):
        with pytest.raises(ValueError, match='--chunk belongs to stream'):
            codec.check_option_args(_flags(command, chunk=4096, tile=128 if command.startswith('compress') else None))
    for bad in (0, -5):
        with pytest.raises(ValueError, match='--chunk {} is not at least 1'.format(bad)):
            codec.check_option_args(_flags('stream', chunk=bad))
    for kw, why in ((dict(salvage=True), '--salvage does not go with stream'), (dict(partial=True), '--partial does not go with stream'),
                    (dict(recover=True), '--recover does not go with stream'), (dict(channels=4), '--channels does not go with stream'),
                    (dict(tile=128), '--tile belongs to compress'), (dict(checked=True, tile=128), '--tile belongs to compress'),
                    (dict(progressive=True), '--progressive belongs to compress'), (dict(layers='4,32'), '--layers belongs to compress'),
                    (dict(wavefront=True), '--wavefront belongs to compress'), (dict(checked=True), '--checked belongs to compress')):
        with pytest.raises(ValueError, match=why):
            codec.check_option_args(_flags('stream', **kw))
    old = argparse.Namespace(command='decompress', tile=None, checked=False, wavefront=False, salvage=True, channels=None)
    codec.check_option_args(old)                                              # a namespace without the key reads as no --chunk
    assert codec.STREAM_CHUNK == 16384


def test_stream_command_refuses_before_any_model(tmp_path, capsys):
    src = tmp_path / 'a.icf'
    src.write_bytes(_file()[0])
    for extra, why in ((['--recover'], '--recover does not go with stream'), (['--chunk', '0'], '--chunk 0 is not at least 1'),
                       (['--channels', '4'], '--channels does not go with stream')):
        assert codec.main(['stream', str(src), str(tmp_path / 'out')] + extra) == 2
        assert why in capsys.readouterr().err
    assert codec.main(['decompress', str(src), str(tmp_path / 'x.png'), '--chunk', '512']) == 2
    assert '--chunk belongs to stream' in capsys.readouterr().err
    assert not (tmp_path / 'out').exists()


# ---- the feed -----------------------------------------------------------------------------------------------------------------

class _NoModel(object):
    """the part of Codec that feed() asks before the first picture, without the model checks: no device"""

    def _recover_head(self, data):
        return codec.parse_recover(data)


def test_header_length_from_a_prefix():
    for ends in (ENDS, [8], list(range(1, 9))):
        data = _file(ends=ends)[0]
        head = codec.layer_prefix_bytes(data, 0)
        known = [n for n in range(len(data) + 1) if codec.stream_header_bytes(data[:n]) is not None]
        assert known == list(range(known[0], len(data) + 1)) and known[0] < head          # told by its front, long before it is whole
        assert all(codec.stream_header_bytes(data[:n]) == head for n in known)
        assert known[0] == 4 + 2 + 2 + len(HEAD['ae_name']) + 2 + len(HEAD['pc_name']) + 42


def test_feed_cut_headers():
    data = _file()[0]
    head = codec.layer_prefix_bytes(data, 0)
    for step in (1, 7, head - 1, head, head + 3, len(data)):
        dec = codec.StreamDecoder(_NoModel())
        for pos in range(0, len(data), step):
            n = min(pos + step, len(data))
            assert dec.feed(data[pos:n]) is (n >= head), (step, n)
            assert dec.bytes_fed == n
            assert dec.progress() == (tuple(codec.parse_recover(data[:n])[1]) if n >= head else ())
        assert dec.progress() == (len(ENDS),) * 4
    dec = codec.StreamDecoder(_NoModel())
    assert dec.feed(b'') is False and dec.feed(data[:3]) is False
    with pytest.raises(ValueError, match='no complete layer'):
        dec.image()
    assert dec.feed(data[3:head]) is True and dec.progress() == (0,) * 4
    with pytest.raises(ValueError, match='no complete layer'):                # the header alone: no picture yet, and nothing was launched
        dec.image()
    assert dec._session is None


def test_feed_damaged_headers():
    data = _file()[0]
    head = codec.layer_prefix_bytes(data, 0)
    for pos in (8, head - 20, head - 2):                                      # a name, the segment table, the header's CRC
        bad = bytearray(data)
        bad[pos] ^= 0x01
        dec = codec.StreamDecoder(_NoModel())
        assert dec.feed(bytes(bad[:head - 1])) is False                       # nothing can be said before the header's CRC is there
        with pytest.raises(ValueError, match='header damaged'):
            dec.feed(bytes(bad[head - 1:head]))
        with pytest.raises(ValueError, match='header damaged'):               # and it stays refused
            dec.feed(bytes(bad[head:]))
    front = 4 + 2 + 2 + len(HEAD['ae_name']) + 2 + len(HEAD['pc_name']) + 8 + 10 + 2 + 8 + 4
    for off, value, why in ((8, 0, 'layer count G = 0'), (8, 17, 'layer count G = 17'), (4, 5, '5 tiles do not cover'), (0, 0, 'tiles do not cover')):
        bad = bytearray(data)
        bad[front + off:front + off + 2] = struct.pack('<H', value)
        dec = codec.StreamDecoder(_NoModel())
        assert dec.feed(bytes(bad[:front + 9])) is False
        with pytest.raises(ValueError, match='header damaged: .*' + why):     # told as soon as the field is there: no waiting for a length that is wrong
            dec.feed(bytes(bad[front + 9:front + 10]))


def test_feed_wrong_magic_and_wrong_format():
    data, _, firsts = _file()
    for n in (1, 2, 4, 60):
        with pytest.raises(ValueError, match='header damaged: wrong magic'):
            codec.StreamDecoder(_NoModel()).feed((b'XCVF' + data[4:])[:n])
    dec = codec.StreamDecoder(_NoModel())
    assert dec.feed(b'IC') is False
    with pytest.raises(ValueError, match='wrong magic'):
        dec.feed(b'VX')
    args = [HEAD[k] for k in ('ae_name', 'pc_name', 'H', 'W', 'C', 'h', 'w', 'L')]
    tail = [HEAD[k] for k in ('resolution', 'fingerprint')]
    others = [codec.build_container(*(args + [0] + tail + [b'abc']))] + \
             [build(*(args + tail + [4, 4, firsts, [b'ab'] * 4]))
              for build in (codec.build_tiled_container, codec.build_checked_container, codec.build_wavefront_container)]
    for d in others:                                                          # recover's words, from the first six bytes on
        dec = codec.StreamDecoder(_NoModel())
        assert dec.feed(d[:5]) is False
        with pytest.raises(ValueError, match=r'--salvage.*decompress'):
            dec.feed(d[5:6])
        with pytest.raises(ValueError, match=r'--salvage.*decompress'):
            codec.StreamDecoder(_NoModel()).feed(d)
    for version in (0, 3, 7):
        with pytest.raises(ValueError, match='header damaged: format version {} is not the layered version 6'.format(version)):
            codec.StreamDecoder(_NoModel()).feed(data[:4] + struct.pack('<H', version) + data[6:40])


# ---- the workspace ------------------------------------------------------------------------------------------------------------

def test_workspace_size():
    from imgcomp_cvpr_amd import _lib
    resume = _lib.lib.ic_pc_decode_tiles_batch_layers_resume_workspace_bytes
    pertile = _lib.lib.ic_pc_decode_tiles_batch_layers_pertile_workspace_bytes
    align = lambda b: (b + 255) & ~255
    for args in ((32, 16, 16, 24, 1, 24, 4), (6, 4, 4, 4, 1, 24, 3), (8, 4, 3, 8, 2, 24, 16), (32, 16, 16, 1000, 7, 24, 1), (1, 1, 1, 1, 1, 24, 1)):
        a, b = int(resume(*args)), int(pertile(*args))
        assert a == b + 2 * align(4 * args[3]) and a > b > 0, args            # the per-tile entry's and two aligned int[ntiles] tables
        assert int(resume(*args)) == a                                        # a function of its seven arguments
    for args in ((32, 16, 16, 24, 1, 24, 0), (32, 16, 16, 24, 1, 24, 17), (32, 16, 16, 0, 1, 24, 4), (32, 16, 16, 24, 0, 24, 4), (0, 16, 16, 24, 1, 24, 4)):
        assert int(resume(*args)) == 0, args
    # monotone in the number of tiles and in the largest tile: a session's workspace for all tiles serves every smaller launch
    assert resume(32, 16, 16, 23, 1, 24, 4) <= resume(32, 16, 16, 24, 1, 24, 4) and resume(32, 15, 16, 24, 1, 24, 4) <= resume(32, 16, 16, 24, 1, 24, 4)
