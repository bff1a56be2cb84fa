"""No device: tests/golden/codec_files.npz against today's host side.  The fixture holds files a past build wrote on the device and
the frequency tables it coded them with (tests/codec_golden_cases.py, tools/make_codec_golden.py).  Here: the synthetic weights
still give the recorded fingerprints; today's parser reads every recorded file to the expected header, geometry and segments, and
today's builders write the same bytes back; and, for the pairs whose tables are kept raw, the host coder over (symbols, tables)
reproduces every file byte for byte and the host decoder returns the symbols from every stream.  Every comparison is an equality.
tests/test_gpu_codec_golden.py holds the device to the same bytes."""
import numpy as np
import pytest

from imgcomp_cvpr_amd import codec
from tests import codec_golden_cases as G

VERSION_TYPE = {1: codec.Container, 2: codec.TiledContainer, 4: codec.CheckedContainer, 5: codec.WavefrontContainer,
                6: codec.LayeredContainer, 8: codec.LayeredContainer}
FILES = [(m, v, f) for m, v in G.PAIRS for f in G.formats_of(m)]


@pytest.fixture(scope='module')
def golden():
    return G.Golden()


@pytest.fixture(scope='module')
def parsed(golden):
    return {(m, v, f): codec.parse_container(golden.file(m, v, f)) for m, v, f in FILES}


def test_cases_cover_what_they_say():
    assert G.grid() == [(0, 0, 4, 8), (0, 8, 4, 1), (4, 0, 3, 8), (4, 8, 3, 1)]
    assert G.formats_of('plain') == G.formats_of('sharp') == G.FORMATS and G.formats_of('k64') == (1, 2, 4)
    assert len(FILES) == 2 * (6 + 6 + 3)
    assert ('sharp', 'iid') in G.RAW_TABLES and {m for m, _ in G.RAW_TABLES} == set(G.MODELS)
    assert codec.check_layer_ends(G.ENDS, G.SHAPE[0]) == list(G.ENDS)
    # every segment of the front-layered tiles holds symbols, on every tile extent
    for _, _, a, b in G.grid():
        cuts = codec.front_layer_cuts(G.SHAPE[0], a, b, G.ENDS)
        assert 1 < cuts[0] < cuts[1] < cuts[2] == G.SHAPE[0] * a * b


def test_fixture_is_small_and_complete(golden):
    import os
    assert os.path.getsize(G.PATH) <= G.MAX_BYTES
    assert golden.sharp == G.SHARP and golden.rocm
    for m, v in G.PAIRS:
        for what in ('logits', 'tables', 'tile_tables'):
            assert len(golden.digest(m, v, what)) == 64
        assert (golden.tables(m, v) is not None) == ((m, v) in G.RAW_TABLES) == (golden.tables(m, v, 'tile_tables') is not None)


def test_volumes_are_the_seeded_ones(golden):
    fill = codec.fill_symbol(G.centers(G.weights('plain')))
    iid, masked = G.volume('iid', fill), G.volume('masked', fill)
    assert iid.shape == G.SHAPE and iid.dtype == np.int64 and set(np.unique(iid)) == set(range(6))
    tail = (masked == fill)[::-1].cumprod(axis=0)[::-1].astype(bool)          # the run of fill symbols that ends at the last channel
    assert np.array_equal(masked[~tail], iid[~tail]) and 0.2 < (masked != iid).mean() < 0.6 and not tail.all(axis=0).any()
    for m in G.MODELS:
        assert np.array_equal(golden.symbols(m, 'iid'), iid) and np.array_equal(golden.symbols(m, 'masked'), masked)


@pytest.mark.parametrize('model', G.MODELS)
def test_synthetic_weights_give_the_recorded_fingerprint(golden, parsed, model):
    fp = G.fingerprint(G.weights(model))
    assert fp == golden.fingerprint(model)
    for (m, v, f), c in parsed.items():
        if m == model:
            assert c.fingerprint == fp, (m, v, f)
    assert len({golden.fingerprint(m) for m in G.MODELS}) == 3


@pytest.mark.parametrize('model,vol,fmt', FILES)
def test_golden_file_parses_and_rebuilds(golden, parsed, model, vol, fmt):
    data, c, sym = golden.file(model, vol, fmt), parsed[(model, vol, fmt)], golden.symbols(model, vol)
    C, h, w = G.SHAPE
    assert type(c) is VERSION_TYPE[fmt] and c.version == fmt
    assert (c.ae_name, c.pc_name, c.H, c.W, c.C, c.h, c.w, c.L, c.resolution) == (G.AE, G.PC_OF[model]) + G.IMAGE_HW + (C, h, w, 6, G.RESOLUTION)
    head = (c.ae_name, c.pc_name, c.H, c.W, c.C, c.h, c.w, c.L)
    if fmt == 1:
        assert c.first_sym == sym[0, 0, 0]
        assert codec.build_container(*(head + (c.first_sym, c.resolution, c.fingerprint, c.payload))) == data
        return
    assert (c.th, c.tw) == G.TILE and len(c.streams) == len(G.grid()) == 4
    assert c.first_syms == [int(sym[0, y0, x0]) for y0, x0, _, _ in G.grid()]
    tiled = head + (c.resolution, c.fingerprint, c.th, c.tw, c.first_syms)
    if fmt in (6, 8):
        assert c.layer_ends == list(G.ENDS) and len(c.segments) == 3 and all(len(layer) == 4 for layer in c.segments)
        assert c.streams == [[c.segments[g][t] for g in range(3)] for t in range(4)]
        build = codec.build_layered_container if fmt == 6 else codec.build_front_layered_container
        assert build(*(tiled + (c.layer_ends, c.segments))) == data
    else:
        build = {2: codec.build_tiled_container, 4: codec.build_checked_container, 5: codec.build_wavefront_container}[fmt]
        assert build(*(tiled + (c.streams,))) == data
        assert b''.join(c.streams) == c.payload


@pytest.mark.parametrize('model,vol', G.RAW_TABLES)
def test_host_coder_reproduces_the_files_from_the_tables(golden, parsed, model, vol):
    sym, tables, tile_tables = golden.symbols(model, vol), golden.tables(model, vol), golden.tables(model, vol, 'tile_tables')
    assert tables.shape == tile_tables.shape == (sym.size, 6)
    assert G.sha256(tables, '<i4') == golden.digest(model, vol, 'tables') and G.sha256(tile_tables, '<i4') == golden.digest(model, vol, 'tile_tables')
    assert 1 <= min(tables.min(), tile_tables.min()) and max(tables.max(), tile_tables.max()) <= G.RESOLUTION
    for fmt in G.formats_of(model):
        assert G.host_file(model, fmt, sym, tables, tile_tables, golden.fingerprint(model)) == golden.file(model, vol, fmt), \
            'format {}: the host coder over the pinned tables writes other bytes than the golden file holds'.format(fmt)
        back = G.host_decode_file(fmt, parsed[(model, vol, fmt)], tables, tile_tables)
        assert np.array_equal(back, sym), 'format {}: the host decoder over the pinned tables returns other symbols'.format(fmt)


@pytest.mark.parametrize('model,vol', [p for p in G.PAIRS if 6 in G.formats_of(p[0])])
@pytest.mark.parametrize('fmt', [6, 8])
def test_layer_prefixes_of_the_golden_bytes(golden, parsed, model, vol, fmt):
    data, c = golden.file(model, vol, fmt), parsed[(model, vol, fmt)]
    ends = [codec.layer_prefix_bytes(data, g) for g in range(4)]
    assert ends == [codec.layer_prefix_bytes(c, g) for g in range(4)] and ends[3] == len(data) - 4
    assert [b - a for a, b in zip(ends, ends[1:])] == [sum(len(s) for s in layer) for layer in c.segments]
    for g in range(4):
        # the prefix of g layers, one byte less, and the header of the prefix alone giving the same lengths
        p, complete, crc_ok = codec.parse_partial(data[:ends[g]])
        assert complete == g and not crc_ok and p.segments[:g] == c.segments[:g]
        assert all(s is None for layer in p.segments[g:] for s in layer)
        assert codec.layer_prefix_bytes(data[:ends[0]], g) == ends[g]
        if g:
            assert codec.parse_partial(data[:ends[g] - 1])[1] == g - 1
    assert codec.parse_partial(data)[1:] == (3, True)


def test_sharp_is_peaked_and_reaches_the_floor(golden):
    share, floor = G.sharp_shares(golden.tables('sharp', 'iid'))
    print('sharp/iid: {:.4f} of the positions hold a frequency >= {} * resolution, {} entries at the floor of 1'.format(share, G.PEAK, floor))
    assert share >= G.PEAK_SHARE and floor >= 1
    # plain, the model every other codec test runs on, reaches neither
    assert G.sharp_shares(golden.tables('plain', 'iid')) == (0.0, 0)
