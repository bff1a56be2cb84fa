"""-m gpu: a tile decode cut into chunks by max_workspace_bytes equals the same call in one launch, in every mode of
PredictionNetwork.decode_tiles_batch and for choose_tiles_batch.  Where the rows of a chunk begin -- in the tile table, the segment
table, the per-tile limits and the status words -- is host arithmetic that only a device run of more than one chunk checks.
Volumes (4, 3, 3) and (4, 2, 3) at tile 2 x 2: all four tile shapes, six tiles; streams by encode_tiles_batch, the synthetic model.
The budgets are what the mode's own size function gives for two and for four 2 x 2 tiles; the size functions do not grow below four
tiles, so the first makes launches of 3 and 3 tiles (3 and 2 where a tile is left out) and the second of 4 and 2 (4 and 1): two
different cuts, one inside volume 0 or behind it, one inside volume 1.  Every comparison is torch.equal."""
import numpy as np
import pytest
import torch

from tests.test_gpu_codec_decoder import _load

pytestmark = pytest.mark.gpu

SHAPES = [(4, 3, 3), (4, 2, 3)]
TH = TW = 2
ENDS = [2, 4]
TILE_LAYERS = [[2, 1, 0, 2], [1, 2]]
_SIZE = 'ic_pc_decode_tiles_batch{}_workspace_bytes'
# streams -> keywords of encode_tiles_batch
ENCODE = {'raster': {}, 'wavefront': {'order': 'wavefront'}, 'rans': {'order': 'rans'}, 'depth': {'order': 'wavefront', 'depth_block': 2},
          'layers': {'layer_ends': ENDS}, 'fronts': {'front_ends': ENDS}}
# mode -> (streams, keywords of decode_tiles_batch, the entry's workspace-size function, whether the call decodes everything)
MODES = {
    'plain': ('raster', {}, '', True),
    'plain_missing': ('raster', {}, '', False),
    'conceal': ('raster', {'conceal': True}, '', False),
    'preview': ('raster', {'channels': 2}, '', False),
    'wavefront': ('wavefront', {'order': 'wavefront'}, '', True),
    'wavefront_preview': ('wavefront', {'order': 'wavefront', 'channels': 3}, '', False),
    'rans': ('rans', {'order': 'rans'}, '', True),
    'rans_preview': ('rans', {'order': 'rans', 'channels': 2}, '', False),
    'depth': ('depth', {'order': 'wavefront', 'depth_block': 2}, '', True),
    'depth_preview': ('depth', {'order': 'wavefront', 'depth_block': 2, 'channels': 3}, '', False),
    'layers': ('layers', {'layer_ends': ENDS}, '_layers', True),
    'layers_preview': ('layers', {'layer_ends': ENDS, 'channels': 2}, '_layers', False),
    'layers_pertile': ('layers', {'layer_ends': ENDS, 'tile_layers': TILE_LAYERS}, '_layers_pertile', False),
    'fronts': ('fronts', {'front_ends': ENDS}, '_fronts', True),
    'fronts_preview': ('fronts', {'front_ends': ENDS, 'channels': 2}, '_fronts', False),
    'fronts_pertile': ('fronts', {'front_ends': ENDS, 'tile_layers': TILE_LAYERS}, '_fronts_pertile', False),
}
MISSING = ('plain_missing', 'conceal')           # volume 0's tile 2 has no stream


@pytest.fixture(scope='module')
def pred(cuda, configs, syn_weights):
    return _load(cuda, configs[0], configs[1], syn_weights, 1e9)


@pytest.fixture(scope='module')
def coded(pred):
    """the symbols, and per kind of stream what encode_tiles_batch gives for them"""
    syms = [np.random.RandomState(11 + n).randint(0, pred.pc.L, size=shape).astype(np.int64) for n, shape in enumerate(SHAPES)]
    return syms, {kind: pred.encode_tiles_batch(syms, TH, TW, **kw) for kind, kw in ENCODE.items()}


def _budget(pred, name, tiles, layered):
    from imgcomp_cvpr_amd import _lib
    tail = (len(ENDS),) if layered else ()
    return int(getattr(_lib.lib, _SIZE.format(name))(SHAPES[0][0], TH, TW, tiles, len(SHAPES), pred.pc._k, *tail))


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize('mode', list(MODES))
def test_chunked_decode_equals_one_launch(pred, coded, mode):
    kind, kw, size_name, full = MODES[mode]
    syms, streams = coded
    volumes = []
    for n, (tiles, shape) in enumerate(zip(streams[kind], SHAPES)):
        payloads = [None if mode in MISSING and (n, t) == (0, 2) else s for t, (s, _) in enumerate(tiles)]
        volumes.append((payloads, [f for _, f in tiles], shape))
    whole = pred.decode_tiles_batch(volumes, TH, TW, want='both', **kw)
    assert _budget(pred, size_name, 2, bool(size_name)) <= _budget(pred, size_name, 4, bool(size_name)) < _budget(pred, size_name, 5, bool(size_name))
    for tiles in (2, 4):
        cut = pred.decode_tiles_batch(volumes, TH, TW, want='both', max_workspace_bytes=_budget(pred, size_name, tiles, bool(size_name)), **kw)
        assert _same(cut, whole), (mode, tiles)
    if full:
        for (q, sym), want in zip(whole, syms):
            assert torch.equal(sym.cpu(), torch.as_tensor(want)), mode
            assert torch.equal(q, pred.centers.float()[sym]), mode


@pytest.mark.parametrize('lam', [0.05, [[0.0, 0.5, 1.0, 2.0], [0.25, 0.125]]], ids=['one lambda', 'per tile'])
def test_chunked_choice_equals_one_launch(pred, cuda, lam):
    zs = [torch.as_tensor(np.random.RandomState(3 + n).randn(*shape).astype(np.float32) * 1.5).to(cuda) for n, shape in enumerate(SHAPES)]
    whole = pred.choose_tiles_batch(zs, TH, TW, lam, want='both')
    for tiles in (2, 4):
        cut = pred.choose_tiles_batch(zs, TH, TW, lam, want='both', max_workspace_bytes=_budget(pred, '', tiles, False))
        assert _same(cut, whole), tiles
    for q, sym in whole:
        assert torch.equal(q, pred.centers.float()[sym])
