"""The eight file formats side by side, on the host: the bytes every builder writes and what every reader says to every format, as
literals recorded from the commit before codec.FORMATS existed; what a Codec writes for every combination of its write options; and
the table itself against the constants it replaced."""
import itertools
import struct
import zlib

import pytest

from imgcomp_cvpr_amd import codec

VERSIONS = (1, 2, 4, 5, 6, 8, 10, 12)
# a 6 x 7 latent plane of a 45 x 56 image cut into 4 x 3 tiles: a 2 x 3 grid, all four tile shapes
HEAD = ('cvpr/low', 'cvpr/res_shallow', 45, 56, 5, 6, 7, 6, 1e9, 0xdeadbeef, 4, 3)      # names, H, W, C, h, w, L, resolution, fingerprint, th, tw
FIRSTS = [0, 1, 2, 3, 4, 5]
STREAMS = [b'\x12\x34', b'', b'\x80', b'\x01\x02\x03', b'\xff', b'\x10\x20']
BLOCK = 2                                                            # depth planes of 4, 4, 2, 2, 2, 1 blocks; tile 1 is its plane alone
DEPTH_STREAMS = [b'\x05\x00\x03\x01\x12\x34', b'\x00\x00\x00\x00', b'\x02\x05\x80', b'\x01\x00\x01\x02\x03', b'\x04\x04\xff', b'\x03\x10\x20']
LANES = 8                                                            # 32 bytes of states, then whole words; tile 1 is its states alone
RANS_STREAMS = [struct.pack('<8I', *([65536 + t] * 8)) + words
                for t, words in enumerate([b'\x12\x34', b'', b'\x80\x00', b'\x01\x02\x03\x04', b'\xff\xff', b'\x10\x20'])]
ENDS = [1, 3, 5]
SEGMENTS = [[bytes([16 * g + t]) * ((g + t) % 3) for t in range(6)] for g in range(3)]      # (some are empty)
PAYLOAD = b'\x01\x02\x03\x04\x05'


def build(version):
    if version == 1:
        return codec.build_container(*(HEAD[:8] + (3,) + HEAD[8:10] + (PAYLOAD,)))
    if version in (6, 8):
        builder = codec.build_layered_container if version == 6 else codec.build_front_layered_container
        return builder(*(HEAD + (FIRSTS, ENDS, SEGMENTS)))
    if version == 10:
        return codec.build_depth_container(*(HEAD + (BLOCK, FIRSTS, DEPTH_STREAMS)))
    if version == 12:
        return codec.build_rans_container(*(HEAD + (LANES, FIRSTS, RANS_STREAMS)))
    builder = {2: codec.build_tiled_container, 4: codec.build_checked_container, 5: codec.build_wavefront_container}[version]
    return builder(*(HEAD + (FIRSTS, STREAMS)))


FILES = {
    1: '4943564601000800637670722f6c6f771000637670722f7265735f7368616c6c6f772d0000003800000005000600000007000000060003000000000065cdcd41efbeadde0500000000000000010203040585e6e648',
    2: '4943564602000800637670722f6c6f771000637670722f7265735f7368616c6c6f772d000000380000000500060000000700000006000000000065cdcd41efbeadde04000300060000000000020000000100000000000200010000000300030000000400010000000500020000000900000000000000123480010203ff102013208d0c',
    4: '4943564604000800637670722f6c6f771000637670722f7265735f7368616c6c6f772d000000380000000500060000000700000006000000000065cdcd41efbeadde04000300060000000000020000009996991801000000000000000000020001000000ad6cba3f0300030000001d80bc55040001000000000000ff0500020000006620753009000000000000006fd14abf123480010203ff10205fb2ce68',
    5: '4943564605000800637670722f6c6f771000637670722f7265735f7368616c6c6f772d000000380000000500060000000700000006000000000065cdcd41efbeadde04000300060000000000020000009996991801000000000000000000020001000000ad6cba3f0300030000001d80bc55040001000000000000ff050002000000662075300900000000000000a8d72f5f123480010203ff10205fb2ce68',
    6: '4943564606000800637670722f6c6f771000637670722f7265735f7368616c6c6f772d000000380000000500060000000700000006000000000065cdcd41efbeadde040003000600000003000100030005000000010002000300040005000000000000000000010000001bdf05a5020000005111e19d000000000000000001000000942b6fd5020000003512c44c01000000e9ffb5cf020000001d11b07800000000000000000100000053aebc5602000000d711ad75000000000000000002000000951633ef00000000000000000100000069ae620702000000ec14175d000000000000000001000000ca3b069912000000000000009501e40801020204050510111113141420202223232539f9c651',
    8: '4943564608000800637670722f6c6f771000637670722f7265735f7368616c6c6f772d000000380000000500060000000700000006000000000065cdcd41efbeadde040003000600000003000100030005000000010002000300040005000000000000000000010000001bdf05a5020000005111e19d000000000000000001000000942b6fd5020000003512c44c01000000e9ffb5cf020000001d11b07800000000000000000100000053aebc5602000000d711ad75000000000000000002000000951633ef00000000000000000100000069ae620702000000ec14175d000000000000000001000000ca3b069912000000000000007148117801020204050510111113141420202223232539f9c651',
    10: '494356460a000800637670722f6c6f771000637670722f7265735f7368616c6c6f772d000000380000000500060000000700000006000000000065cdcd41efbeadde04000300020006000000000006000000af7138ab0100040000001cdf4421020003000000197a0a6c030005000000a287bf51040003000000475b26b1050003000000d255ab8c1800000000000000864211ff0500030112340000000002058001000102030404ff031020c09f17c2',
    12: '494356460c000800637670722f6c6f771000637670722f7265735f7368616c6c6f772d000000380000000500060000000700000006000000000065cdcd41efbeadde040003000800060000000000220000009ff4c74d0100200000006cb671cf02002200000039d05c8803002400000004f895cb0400220000005115603f05002200000052aafe4ecc00000000000000dedcd027000001000000010000000100000001000000010000000100000001000000010012340100010001000100010001000100010001000100010001000100010001000100020001000200010002000100020001000200010002000100020001000200010080000300010003000100030001000300010003000100030001000300010003000100010203040400010004000100040001000400010004000100040001000400010004000100ffff05000100050001000500010005000100050001000500010005000100050001001020fd9ed2f1',
}

TYPES = {1: codec.Container, 2: codec.TiledContainer, 4: codec.CheckedContainer, 5: codec.WavefrontContainer, 6: codec.LayeredContainer,
         8: codec.LayeredContainer, 10: codec.DepthContainer, 12: codec.RansContainer}


def _crcs(streams):
    return [zlib.crc32(b) & 0xffffffff for b in streams]


@pytest.mark.parametrize('version', VERSIONS)
def test_pinned_bytes(version):
    data = build(version)
    assert data == bytes.fromhex(FILES[version])
    c = codec.parse_container(data)
    assert type(c) is TYPES[version] and c.version == version
    assert (c.ae_name, c.pc_name, c.H, c.W, c.C, c.h, c.w, c.L, c.resolution, c.fingerprint) == HEAD[:10]
    if version == 1:
        assert c.first_sym == 3 and c.payload == PAYLOAD
        return
    assert (c.th, c.tw) == HEAD[10:] and c.first_syms == FIRSTS
    if version in (6, 8):
        assert c.layer_ends == ENDS and c.segments == SEGMENTS and c.segment_crcs == [_crcs(layer) for layer in SEGMENTS]
        assert c.streams == [[SEGMENTS[g][t] for g in range(3)] for t in range(6)]
        assert c.payload == b''.join(b for layer in SEGMENTS for b in layer)
        return
    streams = {10: DEPTH_STREAMS, 12: RANS_STREAMS}.get(version, STREAMS)
    assert c.streams == streams and c.payload == b''.join(streams)
    if version == 2:
        assert not hasattr(c, 'stream_crcs')
        return
    assert c.stream_crcs == _crcs(streams)
    if version == 10:
        assert c.depth_block == BLOCK
    if version == 12:
        assert c.lanes == LANES


def test_table():
    assert tuple(codec.FORMATS) == VERSIONS
    for version, row in codec.FORMATS.items():
        assert row.version == version and row.container is TYPES[version]
        assert type(codec.parse_container(bytes.fromhex(FILES[version]))) is row.container
        assert row.checked == any(f in row.container._fields for f in ('stream_crcs', 'segment_crcs'))
        assert row.layered == (row.container is codec.LayeredContainer)
        assert row.extra is None or row.container._fields[-1] == row.extra
    data = bytearray(bytes.fromhex(FILES[2]))
    for v in (3, 7, 9, 11, 13):
        data[4:6] = struct.pack('<H', v)
        with pytest.raises(ValueError) as e:
            codec.parse_container(bytes(data))
        assert str(e.value) == codec._unsupported(v)
    assert codec._TILED == (codec.TiledContainer, codec.CheckedContainer, codec.WavefrontContainer, codec.LayeredContainer,
                            codec.DepthContainer, codec.RansContainer)
    assert codec._LAYERED_VERSIONS == (6, 8) and codec._WITH_CRCS == (4, 5)


# ---- every reader against every format ------------------------------------------------------------------------------------------

READERS = (('salvage', codec.parse_salvage), ('partial', codec.parse_partial), ('recover', codec.parse_recover),
           ('stream', lambda d: codec.stream_header_bytes(d, fronts=False)), ('stream fronts', lambda d: codec.stream_header_bytes(d, fronts=True)),
           ('prefix', lambda d: codec.layer_prefix_bytes(d, 1)))

ACCEPTED = 'accepted'
NO_CRC = ('format version {v} has nothing to salvage with: one CRC over the whole file, none per tile (only version 4, written with --tile '
          '--checked, can be salvaged)')
NOT_SALVAGED = ('format version {v} (layered tiles) is not salvaged: salvage of layered files is out of scope; decompress --partial '
                '(Codec.decompress_partial) reads the complete layers of a cut file')
NO_PREFIX = ('header damaged: format version {v} is not the layered version 6: only a layered file (--tile --layers / --progressive) decodes '
             'from a prefix')
NOT_LAYERED = ('format version {v} is not the layered version 6: --recover reads layered files (--tile --layers / --progressive); a damaged '
               'format-4 / format-5 file is read with --salvage, an intact file of any format with decompress')
NO_FRONTS = ('format version {v} (front-layered tiles) is not streamed without --fronts (open_stream(fronts=True)), which continues a '
             'front-ordered decode; decompress --recover (Codec.recover) also reads what has arrived of such a file')
ONE_SENTENCE = ('format version {v} ({name}) is not read by {what}: a file to be salvaged is written with --tile --checked or --tile --wavefront '
                '(versions 4 and 5), a file to be read from a prefix, recovered or streamed with the layered formats --layers / --front-layers '
                '(versions 6 and 8); an intact file decodes with decompress')
NAMES = {10: 'depth-mapped tiles', 12: 'lane-parallel rANS tiles'}
# reader -> (the words it is named by in ONE_SENTENCE, the outcome per version of VERSIONS)
REFUSALS = {
    'salvage': ('--salvage', (NO_CRC, NO_CRC, ACCEPTED, ACCEPTED, NOT_SALVAGED, NOT_SALVAGED, ONE_SENTENCE, ONE_SENTENCE)),
    'partial': ('--partial / --recover / stream', (NO_PREFIX,) * 4 + (ACCEPTED, ACCEPTED, ONE_SENTENCE, ONE_SENTENCE)),
    'recover': ('--partial / --recover / stream', (NOT_LAYERED,) * 4 + (ACCEPTED, ACCEPTED, ONE_SENTENCE, ONE_SENTENCE)),
    'stream': ('--partial / --recover / stream', (NOT_LAYERED,) * 4 + (ACCEPTED, NO_FRONTS, ONE_SENTENCE, ONE_SENTENCE)),
    'stream fronts': ('--partial / --recover / stream', (NOT_LAYERED,) * 4 + (ACCEPTED, ACCEPTED, ONE_SENTENCE, ONE_SENTENCE)),
    'prefix': ('--partial / --recover / stream', (NO_PREFIX,) * 4 + (ACCEPTED, ACCEPTED, ONE_SENTENCE, ONE_SENTENCE)),
}


@pytest.mark.parametrize('version', VERSIONS)
@pytest.mark.parametrize('reader', [name for name, _ in READERS])
def test_refusal_matrix(reader, version):
    try:
        dict(READERS)[reader](bytes.fromhex(FILES[version]))
        outcome = 'accepted'
    except ValueError as e:
        outcome = str(e)
    what, outcomes = REFUSALS[reader]
    assert outcome == outcomes[VERSIONS.index(version)].format(v=version, name=NAMES.get(version), what=what)


# ---- what a Codec writes ----------------------------------------------------------------------------------------------------------

OPTIONS = (('checked', True), ('order', 'wavefront'), ('layers', [1, 3, 5]), ('front_layers', 'default'), ('depth_block', 4), ('rans', 'default'))
MODEL_REFUSALS = ('wavefront_refusal', 'layered_refusal', 'depth_refusal', 'rans_refusal')


def shell(tile, options, refused=None):
    """a Codec without a model: the attributes the write target is resolved from"""
    c = codec.Codec.__new__(codec.Codec)
    c.tile, c.checked, c.order, c.layers, c.front_layers, c.depth_block, c.rans, c.C = tile, False, 'raster', None, None, None, None, 5
    for name in MODEL_REFUSALS:
        setattr(c, name, '{}: no'.format(name) if name == refused else None)
    for name, value in options:
        setattr(c, name, value)
    return c


def target_cases():
    for n in (0, 1, 2):
        for options in itertools.combinations(OPTIONS, n):
            for tile in ((4, 3), None):
                yield ('+'.join(name for name, _ in options) or 'plain') + ('' if tile else ' untiled'), tile, options, None
    for refused in MODEL_REFUSALS:
        for options in [()] + [(o,) for o in OPTIONS]:
            yield ('+'.join(name for name, _ in options) or 'plain') + ' ' + refused, (4, 3), options, refused


TARGETS = {
    'plain': 2,
    'plain untiled': 1,
    'checked': 4,
    'checked untiled': 'checked=True needs a tile extent: the checksums of format 4 are per tile',
    'order': 5,
    'order untiled': "order='wavefront' needs a tile extent: format 5 is a tiled format",
    'layers': 6,
    'layers untiled': 'layers needs a tile extent: format 6 is a tiled format',
    'front_layers': 8,
    'front_layers untiled': 'front_layers needs a tile extent: format 8 is a tiled format',
    'depth_block': 10,
    'depth_block untiled': 'depth_block needs a tile extent: format 10 is a tiled format',
    'rans': 12,
    'rans untiled': 'rans needs a tile extent: format 12 is a tiled format',
    'checked+order': 5,
    'checked+order untiled': "order='wavefront' needs a tile extent: format 5 is a tiled format",
    'checked+layers': 6,
    'checked+layers untiled': 'layers needs a tile extent: format 6 is a tiled format',
    'checked+front_layers': 8,
    'checked+front_layers untiled': 'front_layers needs a tile extent: format 8 is a tiled format',
    'checked+depth_block': 10,
    'checked+depth_block untiled': 'depth_block needs a tile extent: format 10 is a tiled format',
    'checked+rans': 'rans does not go with checked=True: format 12 has its own CRC per tile, checked=True writes format 4',
    'checked+rans untiled': 'rans needs a tile extent: format 12 is a tiled format',
    'order+layers': "layers does not go with order='wavefront': a layer is no prefix of a wavefront-ordered stream",
    'order+layers untiled': 'layers needs a tile extent: format 6 is a tiled format',
    'order+front_layers': "front_layers does not go with order='wavefront': format 8 implies the order, order='wavefront' writes the unlayered format 5",
    'order+front_layers untiled': 'front_layers needs a tile extent: format 8 is a tiled format',
    'order+depth_block': "depth_block does not go with order='wavefront': format 10 implies the order, order='wavefront' writes format 5, which codes every position",
    'order+depth_block untiled': 'depth_block needs a tile extent: format 10 is a tiled format',
    'order+rans': "rans does not go with order='wavefront': format 12 implies the order, order='wavefront' writes format 5, one arithmetic coder per tile",
    'order+rans untiled': 'rans needs a tile extent: format 12 is a tiled format',
    'layers+front_layers': 'front_layers does not go with layers: the one cuts the wavefront order at fronts (format 8), the other the raster order at channel planes (format 6)',
    'layers+front_layers untiled': 'front_layers needs a tile extent: format 8 is a tiled format',
    'layers+depth_block': 'depth_block does not go with layers or front_layers: format 10 is one coder run per tile, the layered formats 6 and 8 cut a tile into several',
    'layers+depth_block untiled': 'depth_block needs a tile extent: format 10 is a tiled format',
    'layers+rans': 'rans does not go with layers or front_layers: format 12 is one interleaved stream per tile, the layered formats 6 and 8 cut a tile into several',
    'layers+rans untiled': 'rans needs a tile extent: format 12 is a tiled format',
    'front_layers+depth_block': 'depth_block does not go with layers or front_layers: format 10 is one coder run per tile, the layered formats 6 and 8 cut a tile into several',
    'front_layers+depth_block untiled': 'depth_block needs a tile extent: format 10 is a tiled format',
    'front_layers+rans': 'rans does not go with layers or front_layers: format 12 is one interleaved stream per tile, the layered formats 6 and 8 cut a tile into several',
    'front_layers+rans untiled': 'rans needs a tile extent: format 12 is a tiled format',
    'depth_block+rans': "rans does not go with depth_block: format 10 leaves positions out of an arithmetic coder's stream, format 12 codes every position with W rANS coders",
    'depth_block+rans untiled': 'rans needs a tile extent: format 12 is a tiled format',
    'plain wavefront_refusal': 2,
    'checked wavefront_refusal': 4,
    'order wavefront_refusal': 'wavefront_refusal: no',
    'layers wavefront_refusal': 6,
    'front_layers wavefront_refusal': 'wavefront_refusal: no',
    'depth_block wavefront_refusal': 10,
    'rans wavefront_refusal': 12,
    'plain layered_refusal': 2,
    'checked layered_refusal': 4,
    'order layered_refusal': 5,
    'layers layered_refusal': 'layered_refusal: no',
    'front_layers layered_refusal': 'layered_refusal: no',
    'depth_block layered_refusal': 10,
    'rans layered_refusal': 12,
    'plain depth_refusal': 2,
    'checked depth_refusal': 4,
    'order depth_refusal': 5,
    'layers depth_refusal': 6,
    'front_layers depth_refusal': 8,
    'depth_block depth_refusal': 'depth_refusal: no',
    'rans depth_refusal': 12,
    'plain rans_refusal': 2,
    'checked rans_refusal': 4,
    'order rans_refusal': 5,
    'layers rans_refusal': 6,
    'front_layers rans_refusal': 8,
    'depth_block rans_refusal': 10,
    'rans rans_refusal': 'rans_refusal: no',
}


@pytest.mark.parametrize('case', [c[0] for c in target_cases()])
def test_write_target_matrix(case):
    _, tile, options, refused = next(c for c in target_cases() if c[0] == case)
    try:
        outcome = shell(tile, options, refused).written_version()
    except ValueError as e:
        outcome = str(e)
    assert outcome == TARGETS[case]


def test_write_target_parameter():
    """the validated parameter that goes with the resolved row: the coders, the depth block, the layer ends"""
    for options, version, want in (((), 2, None), (OPTIONS[:1], 4, None), (OPTIONS[1:2], 5, None), (OPTIONS[2:3], 6, [1, 3, 5]),
                                   (OPTIONS[3:4], 8, codec.default_layer_ends(5)), (OPTIONS[4:5], 10, 4),
                                   (OPTIONS[5:], 12, codec.DEFAULT_RANS_LANES), ((('rans', 64),), 12, 64)):
        row, param = shell((4, 3), options)._target()
        assert row is codec.FORMATS[version] and param == want
