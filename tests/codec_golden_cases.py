"""Shared by tools/make_codec_golden.py, tests/test_cpu_codec_golden.py and tests/test_gpu_codec_golden.py: the models, symbol
volumes and container formats whose files and frequency tables tests/golden/codec_files.npz pins, the fixture's layout, and the
host-side reproduction of every file from (symbols, tables) alone.  numpy only: nothing here needs a device.

A file decodes only if the decoder derives, bit for bit, the integer tables the encoder coded with.  The fixture records them as a
past build of the kernels derived them (csrc/probclass.hip, csrc/pc_decode.hip, pc_table_row of csrc/pc_table.h) together with
the files that build wrote, so a change of the arithmetic shows as a difference to a committed byte, not only as a difference
between two paths of the same build.

Models (seed 1234, ae cvpr/low: C = 32, L = 6, resolution 1e9):
    plain   synthetic_weights(low, res_shallow): a Xavier last layer, near-uniform tables
    sharp   the same with the last context-model layer (filter and bias) times SHARP: the logits are exactly SHARP times plain's
            (a power of two commutes with every fp32 product and sum, and with the final ReLU), the tables peaked and
            context-dependent, as a trained model's
    k64     synthetic_weights(low, res_shallow_64): the 64-wide kernel instantiations; formats 5, 6 and 8 refuse that width
Volumes (32, 7, 9), int64, from np.random.RandomState only (the autoencoder's bits are no contract):
    iid     uniform over the L symbols
    masked  iid with every channel c >= c0(y, x) set to the fill symbol, c0 a seeded plane in 4 .. 32: what the importance map
            makes of a real volume
Formats: 1 untiled; 2, 4, 5 (wavefront), 6 (layers 8, 20, 32), 8 (front layers 8, 20, 32) with tile (4, 8), which cuts 7 x 9 into
4 x 8, 4 x 1, 3 x 8, 3 x 1: a full, a one-column and two ragged tiles."""
import hashlib
import os
from collections import OrderedDict

import numpy as np

from imgcomp_cvpr_amd import codec
from tests import codec_cases as cc

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'codec_files.npz')
MAX_BYTES = 256 * 1024                       # the fixture's size limit

SEED = 1234
RESOLUTION = 1e9
AE = 'cvpr/low'
PC_OF = OrderedDict([('plain', 'cvpr/res_shallow'), ('sharp', 'cvpr/res_shallow'), ('k64', 'cvpr/res_shallow_64')])
MODELS = tuple(PC_OF)
# the smallest power of two for which the recorded tables of sharp/iid have a symbol of frequency >= 0.9 * resolution at a tenth
# of the positions or more AND a frequency at the floor of 1 somewhere (sharp_shares; found by tools/make_codec_golden.py --find-sharp)
SHARP = 16.0
PEAK = 0.9
PEAK_SHARE = 0.1

SHAPE = (32, 7, 9)
VOLUMES = ('iid', 'masked')
VOLUME_SEED = 20241019
PAIRS = tuple((m, v) for m in MODELS for v in VOLUMES)
# the pairs whose tables the fixture holds raw; the others are pinned by their sha256 alone.  A pair's raw tables (the whole
# volume's and the tiles', 2016 x 6 int32 each) deflate to about 70 KB (plain, sharp) or 54 KB (k64): four pairs do not fit
# MAX_BYTES, so the three are sharp/iid and one volume of each other model
RAW_TABLES = (('sharp', 'iid'), ('plain', 'iid'), ('k64', 'iid'))

TILE = (4, 8)
ENDS = (8, 20, 32)
FORMATS = (1, 2, 4, 5, 6, 8)
K24_ONLY = (5, 6, 8)                         # the wavefront and the layered decoders cover the width k = 24
FACTOR = 8                                   # the autoencoder's subsampling factor (the generator checks Codec.factor)
IMAGE_HW = (50, 67)                          # ceil(50 / 8) = 7, ceil(67 / 8) = 9, neither a multiple of the factor
# Codec's attributes per format
CODEC_ARGS = {1: dict(tile=None, checked=False, order='raster', layers=None, front_layers=None),
              2: dict(tile=TILE, checked=False, order='raster', layers=None, front_layers=None),
              4: dict(tile=TILE, checked=True, order='raster', layers=None, front_layers=None),
              5: dict(tile=TILE, checked=False, order='wavefront', layers=None, front_layers=None),
              6: dict(tile=TILE, checked=False, order='raster', layers=list(ENDS), front_layers=None),
              8: dict(tile=TILE, checked=False, order='raster', layers=None, front_layers=list(ENDS))}

assert (IMAGE_HW[0] + FACTOR - 1) // FACTOR == SHAPE[1] and (IMAGE_HW[1] + FACTOR - 1) // FACTOR == SHAPE[2]


def formats_of(model):
    """the formats a model's width supports"""
    return tuple(f for f in FORMATS if PC_OF[model] == 'cvpr/res_shallow' or f not in K24_ONLY)


def configs(model):
    from imgcomp_cvpr_amd import config_parser as cp
    ae, _ = cp.parse(cp.builtin_config_path('ae_configs', *AE.split('/')))
    pc, _ = cp.parse(cp.builtin_config_path('pc_configs', *PC_OF[model].split('/')))
    return ae, pc


def weights(model):
    from imgcomp_cvpr_amd import weights as W
    w = W.synthetic_weights(*configs(model), seed=SEED)
    if model == 'sharp':
        for part in ('/weights', '/biases'):
            w[cc.LAST_LAYER + part] = w[cc.LAST_LAYER + part] * np.float32(SHARP)
    return w


def centers(model_weights):
    return model_weights['autoencoder/encoder/centers']


def fingerprint(model_weights):
    """Codec.fingerprint from the numpy weights"""
    return codec.model_fingerprint(centers(model_weights), {k: v for k, v in model_weights.items() if k.startswith('probclass3d/')})


def volume(name, fill):
    """the (32, 7, 9) int64 symbol volume `name`; fill = codec.fill_symbol(centres)"""
    C, h, w = SHAPE
    rs = np.random.RandomState(VOLUME_SEED)
    sym = rs.randint(0, 6, size=SHAPE).astype(np.int64)
    c0 = rs.randint(4, C + 1, size=(h, w))
    if name == 'iid':
        return sym
    assert name == 'masked'
    return np.where(np.arange(C)[:, None, None] >= c0[None], np.int64(fill), sym)


def grid():
    return codec.tile_grid(SHAPE[1], SHAPE[2], *TILE)


def tile_volumes(symbols):
    """the tiles of TILE as volumes of their own, in grid order"""
    return [np.ascontiguousarray(symbols[:, y0:y0 + a, x0:x0 + b]) for y0, x0, a, b in grid()]


def split_tile_tables(tile_tables):
    """the fixture's (C h w, L) tile tables -- every tile's own table rows, tiles back to back in grid order -> one array per tile"""
    counts = [SHAPE[0] * a * b for _, _, a, b in grid()]
    assert sum(counts) == len(tile_tables)
    return np.split(np.asarray(tile_tables), np.cumsum(counts)[:-1])


def sha256(array, dtype):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(array), dtype=dtype).tobytes()).hexdigest()


def sharp_shares(tables):
    """(share of the positions with a symbol of frequency >= PEAK * resolution, number of entries at the floor of 1)"""
    t = np.asarray(tables)
    return float((t.max(axis=1) >= PEAK * RESOLUTION).mean()), int((t == 1).sum())


def _segments(flat, tab, cuts):
    """the coder restarted at every cut: arithmetic_coding's coder over [max(1, n_{g-1}), n_g), index 0 being the uncoded first symbol"""
    return [cc.host_encode(flat[max(1, a):b], tab[max(1, a):b])[0] for a, b in zip([0] + list(cuts), cuts)]


def host_streams(fmt, symbols, tables, tile_tables):
    """what the file of format `fmt` holds per volume (format 1) or per tile, from the host coder over the given tables:
    format 1 -> (stream, first_sym); 2, 4, 5 -> [(stream, first_sym)]; 6, 8 -> [([segment per layer], first_sym)]"""
    if fmt == 1:
        flat = symbols.reshape(-1)
        return cc.host_encode(flat[1:], tables[1:])[0], int(flat[0])
    out = []
    for vol, tab in zip(tile_volumes(symbols), split_tile_tables(tile_tables)):
        C, a, b = vol.shape
        flat = vol.reshape(-1)
        if fmt in (5, 8):
            order = codec.wavefront_order(C, a, b)
            flat, tab = flat[order], tab[order]
        if fmt in (2, 4, 5):
            out.append((cc.host_encode(flat[1:], tab[1:])[0], int(flat[0])))
        else:
            cuts = [e * a * b for e in ENDS] if fmt == 6 else codec.front_layer_cuts(C, a, b, ENDS)
            out.append((_segments(flat, tab, cuts), int(flat[0])))
    return out


def host_file(model, fmt, symbols, tables, tile_tables, model_fingerprint):
    """the bytes of the file of format `fmt` from (symbols, tables) alone: host_streams through the container builder"""
    C, h, w = SHAPE
    head = (AE, PC_OF[model], IMAGE_HW[0], IMAGE_HW[1], C, h, w, 6)
    coded = host_streams(fmt, symbols, tables, tile_tables)
    if fmt == 1:
        return codec.build_container(*(head + (coded[1], RESOLUTION, model_fingerprint, coded[0])))
    tiled = head + (RESOLUTION, model_fingerprint) + TILE + ([f for _, f in coded],)
    if fmt in (6, 8):
        build = codec.build_layered_container if fmt == 6 else codec.build_front_layered_container
        return build(*(tiled + (list(ENDS), [[segs[g] for segs, _ in coded] for g in range(len(ENDS))])))
    build = {2: codec.build_tiled_container, 4: codec.build_checked_container, 5: codec.build_wavefront_container}[fmt]
    return build(*(tiled + ([b for b, _ in coded],)))


def host_decode_file(fmt, container, tables, tile_tables):
    """the host decoder over every stream of a parsed golden file with the given tables -> the (32, 7, 9) symbol volume"""
    C, h, w = SHAPE
    if fmt == 1:
        return np.array([container.first_sym] + cc.host_decode(container.payload, tables[1:]), np.int64).reshape(SHAPE)
    out = np.full(SHAPE, -1, np.int64)
    for t, ((y0, x0, a, b), tab) in enumerate(zip(grid(), split_tile_tables(tile_tables))):
        n = C * a * b
        order = codec.wavefront_order(C, a, b) if fmt in (5, 8) else np.arange(n)
        tab = tab[order]
        if fmt in (2, 4, 5):
            coded = cc.host_decode(container.streams[t], tab[1:])
        else:
            cuts = [e * a * b for e in ENDS] if fmt == 6 else codec.front_layer_cuts(C, a, b, ENDS)
            coded = []
            for g, (lo, hi) in enumerate(zip([0] + list(cuts), cuts)):
                coded += cc.host_decode(container.streams[t][g], tab[max(1, lo):hi])
        flat = np.empty(n, np.int64)
        flat[order] = [container.first_syms[t]] + coded
        out[:, y0:y0 + a, x0:x0 + b] = flat.reshape(C, a, b)
    return out


# ---- the fixture: a flat npz without pickles ------------------------------------------------------------------------------------

def key(model, vol, what):
    return '{}_{}_{}'.format(model, vol, what)


class Golden(object):
    """tests/golden/codec_files.npz, read: symbols as int64, files as bytes, tables as int64 (None where only the hash is kept)"""

    def __init__(self, path=PATH):
        with np.load(path, allow_pickle=False) as z:
            self.z = {k: z[k] for k in z.files}
        self.sharp = float(self.z['meta_sharp'])
        self.rocm = str(self.z['meta_rocm'])

    def fingerprint(self, model):
        return int(self.z['meta_fingerprint_' + model])

    def symbols(self, model, vol):
        return self.z['symbols_' + vol].astype(np.int64)              # (one volume for all models: stored once)

    def file(self, model, vol, fmt):
        return self.z[key(model, vol, 'f{}'.format(fmt))].tobytes()

    def digest(self, model, vol, what):
        """what: 'logits', 'tables' or 'tile_tables'"""
        return str(self.z[key(model, vol, what + '_sha256')])

    def tables(self, model, vol, what='tables'):
        a = self.z.get(key(model, vol, what))
        return None if a is None else a.astype(np.int64)


# ---- the device side, shared by the generator and tests/test_gpu_codec_golden.py (torch is imported where it is needed) --------

def load_codec(model, device):
    """the Codec of a model; its format is chosen per call by set_format"""
    ae_cfg, pc_cfg = configs(model)
    c = codec.Codec(ae_cfg, pc_cfg, weights(model), device)
    assert c.factor == FACTOR and (c.C, c.L) == (SHAPE[0], 6) and c.pred.freqs_resolution == RESOLUTION
    return c


def set_format(c, fmt):
    for name, value in CODEC_ARGS[fmt].items():
        setattr(c, name, value)
    return c


def device_logits(c, symbols):
    """pc.logits on the padded volume, as PredictionNetwork._tables computes what it feeds to ic_pc_logits_to_freqs_f32
    -> (1, C, h, w, L) float32 device tensor"""
    import torch
    vol = c.pred.pad_symbols_volume(symbols)
    sym = torch.as_tensor(np.ascontiguousarray(vol)).to(c.device).long()
    return c.pc.logits(c.pred.centers[sym][None].contiguous(), is_training=False)


def device_tables(c, symbols):
    """pred.get_all's tables of a volume coded as a whole -> (C h w, L) int64 numpy"""
    return c.pred.get_all(c.pred.pad_symbols_volume(symbols))[1]


def device_tile_tables(c, symbols):
    """every tile coded as a volume of its own: its tables, tiles back to back in grid order (split_tile_tables undoes it)"""
    return np.concatenate([device_tables(c, v) for v in tile_volumes(symbols)])


def device_file(c, fmt, symbols):
    import torch
    return set_format(c, fmt)._container(torch.as_tensor(symbols).to(c.device), *IMAGE_HW)
