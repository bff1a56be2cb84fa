"""What the tile coders of probclass.PredictionNetwork hand to the library, pinned without a device: the cases, a stub context
model and a recorder that stands in for probclass.lib.  tests/test_cpu_pc_launches.py runs every case against
tests/golden/pc_launches.json; tools/make_pc_launch_golden.py writes that file.

The recorder keeps, per library call, the entry's name, every number, whether a pointer is NULL, and the bytes behind every host
table read at the pointer it was given with the length the numbers imply (so a chunk's offset shows), short ones as hex and long
ones as a sha256.  It writes back status words from the case's script, in the order of the rows over all launches of the case (so
the offset of a chunk's status slice shows), a value per tile into symbols and q, and for the encoders a length and a byte pattern
over the whole capacity of every coder (so the slice that is cut out shows).  *_bytes / *_floats entries go to the real library,
which loads without a device."""
import ctypes
import hashlib
import itertools
import os
from collections import OrderedDict

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pc_launches.json')
MAX_BYTES = 256 * 1024

L = 6
CENTERS = [-1.8, -1.1, -0.4, 0.3, 1.0, 1.7]
SHAPES = [(4, 3, 3), (4, 2, 3)]              # at tile 2 x 2: all four tile shapes, six tiles
TH = TW = 2
ENDS = [2, 4]
MISSING = (0, 2)                             # the tile whose stream is None
TILE_LAYERS = [[2, 1, 0, 2], [1, 2]]


# ---- the stub model ---------------------------------------------------------------------------------------------------------------

class StubPc(object):
    def __init__(self, k=24):
        self._k, self.L = k, L
        self._tab = (ctypes.c_void_p * 1)()

    @classmethod
    def get_context_size(cls, config):
        return 9

    @classmethod
    def get_context_shape(cls, config):
        return 5, 9, 9

    def logits(self, q, is_training):
        import torch
        N, D, H, W = q.shape
        shape = (N, D - 4, H - 8, W - 8, L)
        return torch.arange(int(np.prod(shape)), dtype=torch.float32).view(shape)


def prediction_network(k=24):
    import torch
    from imgcomp_cvpr_amd import probclass
    return probclass.PredictionNetwork(StubPc(k), None, torch.tensor(CENTERS, dtype=torch.float32))


class _Stream(object):
    cuda_stream = 0

    def synchronize(self):
        pass


def substitutions(recorder):
    """[(object, attribute, value)]: the three replacements under which the coders run on the CPU"""
    import torch
    from imgcomp_cvpr_amd import _lib, probclass
    return [(probclass, 'lib', recorder), (torch.cuda, 'current_stream', lambda device=None: _Stream()),
            (_lib, 'require_cuda', lambda t, name='tensor': None)]


# ---- the recorder -----------------------------------------------------------------------------------------------------------------

def _addr(x):
    if x is None:
        return 0
    if isinstance(x, ctypes.c_void_p):
        return x.value or 0
    if isinstance(x, int):
        return x
    return ctypes.addressof(x)


def _blob(data):
    data = bytes(data)
    return 'h:' + data.hex() if len(data) <= 48 else 's:{}:{}'.format(hashlib.sha256(data).hexdigest()[:16], len(data))


_CHANNELS, _PER, _RESUME = ('int', 'int'), ('per tile', 'int'), ('per tile', 'per tile', 'int')
BATCH = OrderedDict([
    ('ic_pc_decode_tiles_batch_f32', ()),
    ('ic_pc_decode_tiles_batch_channels_f32', _CHANNELS),
    ('ic_pc_decode_tiles_batch_layers_f32', _CHANNELS + ('segs',)),
    ('ic_pc_decode_tiles_batch_fronts_f32', _CHANNELS + ('segs',)),
    ('ic_pc_decode_tiles_batch_layers_pertile_f32', _PER + ('segs',)),
    ('ic_pc_decode_tiles_batch_fronts_pertile_f32', _PER + ('segs',)),
    ('ic_pc_decode_tiles_batch_layers_resume_f32', _RESUME + ('segs',)),
    ('ic_pc_decode_tiles_batch_fronts_resume_f32', _RESUME + ('segs',)),
])


def _tables_of(name, a, args):
    """argument index -> number of bytes of the host table (or of the device input that is hashed) behind it"""
    if name in BATCH:
        tail = BATCH[name]
        out = {0: a[1], 2: a[3] * 40, 4: a[5] * 24}
        if tail and tail[-1] == 'segs':
            n = 19 + len(tail) - 1
            out[n], out[n + 2] = a[n + 1] * 4, a[3] * a[n + 1] * 16
        for i, what in enumerate(tail):
            if what == 'per tile':
                out[19 + i] = a[3] * 4
        return out
    if name == 'ic_pc_decode_tiles_f32':
        return {0: a[1], 2: a[3] * 40}
    if name in ('ic_pc_decode_f32', 'ic_pc_decode_channels_f32'):
        return {0: a[1]}
    if name == 'ic_pc_encode_f32':
        return {0: a[2] * a[3] * a[4] * 4, 1: a[2] * a[3] * 8}
    if name == 'ic_pc_encode_segments_f32':
        return {0: a[2] * a[3] * a[4] * 4, 1: a[2] * a[3] * 8, 6: max(a[7], 1) * 8}
    if name in ('ic_pc_conceal_tiles', 'ic_pc_conceal_tiles_channels'):
        return {2: a[3] * 40, 4: a[5] * 24, 6: ctypes.sizeof(args[6])}
    raise AttributeError(name)


class Recorder(object):
    def __init__(self):
        from imgcomp_cvpr_amd import _lib
        self._real, self._prototypes = _lib.lib, _lib.PROTOTYPES
        self.begin()

    def begin(self, script=()):
        self.calls, self.script, self.row = [], list(script), 0

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)
        if name.endswith(('_bytes', '_floats')):
            return getattr(self._real, name)
        if name not in self._prototypes:
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _status(self, n):
        words = [self.script[i] if i < len(self.script) else 0 for i in range(self.row, self.row + n)]
        self.row += n
        return words

    def _call(self, name, args):
        argtypes = self._prototypes[name][1]
        assert len(args) == len(argtypes), '{}: {} arguments for a prototype of {}'.format(name, len(args), len(argtypes))
        numbers = [None if t in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)) else (float(v) if t is ctypes.c_float else int(v))
                   for t, v in zip(argtypes, args)]
        tables = _tables_of(name, numbers, args)
        shown = []
        for i, (v, number) in enumerate(zip(args, numbers)):
            if number is not None:
                shown.append(repr(number))
            elif _addr(v) == 0:
                shown.append('0')
            elif i in tables:
                shown.append(_blob(ctypes.string_at(_addr(v), tables[i])))
            else:
                shown.append('p')
        self.calls.append(name + '|' + ','.join(shown))
        first = self.row
        if name in BATCH:
            self._write(args[13], ctypes.c_int32, self._status(numbers[3]))
            tiles = (_pc_tile() * numbers[3]).from_address(_addr(args[2]))
            volumes = (_pc_volume() * numbers[5]).from_address(_addr(args[4]))
            for i, t in enumerate(tiles):
                v = volumes[t.volume]
                for buf, ctype, off in ((args[11], ctypes.c_int64, v.symbols_off), (args[12], ctypes.c_float, v.q_off)):
                    if _addr(buf):
                        cells = np.ctypeslib.as_array((ctype * (numbers[14] * v.h * v.w)).from_address(_addr(buf) + off * ctypes.sizeof(ctype)))
                        cells.reshape(numbers[14], v.h, v.w)[:, t.y0:t.y0 + t.th, t.x0:t.x0 + t.tw] = 1 + first + i
        elif name == 'ic_pc_decode_tiles_f32':
            self._write(args[10], ctypes.c_int32, self._status(numbers[3]))
            C, h, w = numbers[11:14]
            cells = np.ctypeslib.as_array((ctypes.c_int64 * (C * h * w)).from_address(_addr(args[9]))).reshape(C, h, w)
            for i, t in enumerate((_pc_tile() * numbers[3]).from_address(_addr(args[2]))):
                cells[:, t.y0:t.y0 + t.th, t.x0:t.x0 + t.tw] = 1 + first + i
        elif name in ('ic_pc_decode_f32', 'ic_pc_decode_channels_f32'):
            self._write(args[9], ctypes.c_int32, self._status(1))
            n = numbers[10] * numbers[11] * numbers[12]
            self._write(args[8], ctypes.c_int64, [i % L for i in range(n)])
        elif name in ('ic_pc_encode_f32', 'ic_pc_encode_segments_f32'):
            at = 6 if name == 'ic_pc_encode_f32' else 8              # out, capacity, nbytes, status
            units = numbers[2] * (numbers[7] if name != 'ic_pc_encode_f32' and numbers[7] > 0 else 1)
            cap = numbers[at + 1]
            self._write(args[at + 3], ctypes.c_int32, self._status(units))
            self._write(args[at + 2], ctypes.c_int64, [min(cap, 3 + (first + u) % 5) for u in range(units)])
            self._write(args[at], ctypes.c_uint8, [(13 * i + 31 * (first + u)) & 0xff for u in range(units) for i in range(cap)])
        return 0

    @staticmethod
    def _write(pointer, ctype, values):
        if values:
            (ctype * len(values)).from_address(_addr(pointer))[:] = values


def _pc_tile():
    from imgcomp_cvpr_amd import _lib
    return _lib.PcTile


def _pc_volume():
    from imgcomp_cvpr_amd import _lib
    return _lib.PcVolume


# ---- what a call returned -----------------------------------------------------------------------------------------------------------

def shown(x):
    import torch
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    if isinstance(x, np.ndarray):
        return '{}{}:{}'.format(x.dtype, list(x.shape), _blob(np.ascontiguousarray(x).tobytes()))
    if isinstance(x, (bytes, bytearray)):
        return _blob(x)
    if isinstance(x, (list, tuple)):
        return [shown(v) for v in x]
    assert x is None or isinstance(x, (int, float, str)), type(x)
    return x


def run(recorder, fn, script=()):
    """-> {'calls': [...], 'result': ...} or {'calls': [...], 'raises': type, 'message': text}"""
    recorder.begin(script)
    try:
        result = fn()
    except Exception as e:
        return {'calls': recorder.calls, 'raises': type(e).__name__, 'message': str(e)}
    return {'calls': recorder.calls, 'result': shown(result)}


# ---- the cases ----------------------------------------------------------------------------------------------------------------------

_SIZE = 'ic_pc_decode_tiles_batch{}_workspace_bytes'
# mode -> (keywords of decode_tiles_batch, whether the streams are segment lists, the entry's workspace-size function)
DECODE_MODES = OrderedDict([
    ('plain', ({}, False, _SIZE.format(''))),
    ('flags', ({'flags': 2}, False, _SIZE.format(''))),
    ('wavefront', ({'order': 'wavefront'}, False, _SIZE.format(''))),
    ('preview', ({'channels': 2}, False, _SIZE.format(''))),
    ('wavefront_preview', ({'order': 'wavefront', 'channels': 3}, False, _SIZE.format(''))),
    ('conceal', ({'conceal': True}, False, _SIZE.format(''))),
    ('rans', ({'order': 'rans'}, False, _SIZE.format(''))),
    ('rans_lanes_preview', ({'order': 'rans', 'lanes': 8, 'channels': 2}, False, _SIZE.format(''))),
    ('depth', ({'order': 'wavefront', 'depth_block': 2}, False, _SIZE.format(''))),
    ('depth_preview', ({'order': 'wavefront', 'depth_block': 1, 'channels': 3}, False, _SIZE.format(''))),
    ('layers', ({'layer_ends': ENDS}, True, _SIZE.format('_layers'))),
    ('layers_preview', ({'layer_ends': ENDS, 'channels': 2}, True, _SIZE.format('_layers'))),
    ('layers_pertile', ({'layer_ends': ENDS, 'tile_layers': TILE_LAYERS}, True, _SIZE.format('_layers_pertile'))),
    ('fronts', ({'front_ends': ENDS}, True, _SIZE.format('_fronts'))),
    ('fronts_preview', ({'front_ends': ENDS, 'channels': 2}, True, _SIZE.format('_fronts'))),
    ('fronts_pertile', ({'front_ends': ENDS, 'tile_layers': TILE_LAYERS}, True, _SIZE.format('_fronts_pertile'))),
])
# mode -> further status scripts, one word per listed tile (five: the sixth is MISSING) in the order of the launches
DECODE_SCRIPTS = {
    'depth': [[0, 2, 0, 0, 0], [0, 0, 0, 0, 3]],
    'rans': [[0, 0, 4, 0, 0], [0, 5, 0, 0, 0], [0, 0, 0, 0, 6]],
    'rans_lanes_preview': [[4, 0, 0, 0, 0]],
    'conceal': [[0, 1, 0, 0, 3], [1, 1, 1, 1, 1]],
    'layers_pertile': [[1, 0, 0, 0, 1], [0, 0, 2, 0, 0]],
    'fronts_pertile': [[1, 0, 0, 0, 1], [0, 0, 2, 0, 0]],
}
ONE_FAILS = [0, 0, 0, 1, 0]
ENCODE_MODES = OrderedDict([
    ('raster', {}), ('wavefront', {'order': 'wavefront'}), ('layers', {'layer_ends': ENDS}), ('fronts', {'front_ends': ENDS}),
    ('depth', {'order': 'wavefront', 'depth_block': 2}), ('rans', {'order': 'rans', 'lanes': 8}),
])


def grid_count(shape):
    return -(-shape[1] // TH) * -(-shape[2] // TW)


def decode_volumes(segments, shapes=SHAPES, missing=MISSING):
    """[(streams, first_syms, shape)] of arbitrary bytes: a stream per tile, or len(ENDS) segments per tile"""
    volumes, i = [], 0
    for n, shape in enumerate(shapes):
        streams, firsts = [], []
        for t in range(grid_count(shape)):
            i += 1
            stream = [bytes([16 * i + g]) * (2 + i + g) for g in range(len(ENDS))] if segments else bytes([i]) * (3 + i)
            streams.append(None if (n, t) == missing else stream)
            firsts.append(i % L)
        volumes.append((streams, firsts, shape))
    return volumes


def budget(which, size_name, layered):
    """max_workspace_bytes by the entry's own size function: None -> the default, 'two' / 'four' -> what so many 2 x 2 tiles need,
    'below' -> one byte less than the first tile needs alone.  The size functions do not grow below four tiles, so of the five listed
    tiles 'two' makes launches of 3 and 2 (cut between the volumes) and 'four' of 4 and 1 (cut inside volume 1)."""
    from imgcomp_cvpr_amd import _lib
    if which is None:
        return {}
    size = getattr(_lib.lib, size_name)
    tail = (len(ENDS),) if layered else ()
    C = SHAPES[0][0]
    if which == 'below':
        return {'max_workspace_bytes': int(size(C, TH, TW, 1, len(SHAPES), 24, *tail)) - 1}
    return {'max_workspace_bytes': int(size(C, TH, TW, {'two': 2, 'four': 4}[which], len(SHAPES), 24, *tail))}


def symbols(shape, seed):
    return np.random.RandomState(seed).randint(0, L, size=shape).astype(np.int64)


def cases():
    """name -> (function of (pred, pred17) that makes the call, status script)"""
    import torch
    out = OrderedDict()
    for mode, (kw, segments, size_name) in DECODE_MODES.items():
        for want, which in itertools.product(('q', 'symbols', 'both'), (None, 'two', 'four', 'below')):
            if which == 'four' and want != 'both':
                continue
            def call(pred, pred17, kw=kw, segments=segments, size_name=size_name, want=want, which=which):
                return pred.decode_tiles_batch(decode_volumes(segments), TH, TW, want=want, **dict(kw, **budget(which, size_name, segments)))
            out['decode/{}/{}/{}'.format(mode, want, which or 'unlimited')] = (call, ())
        for which, script in itertools.product((None, 'two', 'four'), [ONE_FAILS] + DECODE_SCRIPTS.get(mode, [])):
            def call(pred, pred17, kw=kw, segments=segments, size_name=size_name, which=which):
                return pred.decode_tiles_batch(decode_volumes(segments), TH, TW, want='both', **dict(kw, **budget(which, size_name, segments)))
            out['decode/{}/status {}/{}'.format(mode, ''.join(str(s) for s in script), which or 'unlimited')] = (call, script)

    def empty(pred, pred17):
        return [pred.decode_tiles_batch([], TH, TW), pred.decode_tiles_batch([], TH, TW, conceal=True),
                pred.decode_tiles_batch([], TH, TW, layer_ends=ENDS, tile_layers=[]), pred.choose_tiles_batch([], TH, TW, 0.5)]
    out['decode/no volumes'] = (empty, ())
    listing = [('plain channels', {}, False, [((), (), (3, 2, 2))]),
               ('plain counts', {}, False, [(decode_volumes(False)[0][0][:3], decode_volumes(False)[0][1], SHAPES[0])]),
               ('pertile rows', {'layer_ends': ENDS, 'tile_layers': TILE_LAYERS[:1]}, True, []),
               ('pertile entries', {'layer_ends': ENDS, 'tile_layers': [[1, 1], [1, 1]]}, True, []),
               ('pertile range', {'front_ends': ENDS, 'tile_layers': [[2, 1, 0, 3], [1, 2]]}, True, []),
               ('pertile segments', {'front_ends': ENDS, 'tile_layers': [[2, 1, 1, 2], [1, 2]]}, True, []),
               ('layers segments', {'layer_ends': ENDS}, False, []),
               ('bad want', {}, False, [])]
    for name, kw, segments, extra in listing:
        def call(pred, pred17, name=name, kw=kw, segments=segments, extra=extra):
            return pred.decode_tiles_batch(decode_volumes(segments) + extra, TH, TW, want='colour' if name == 'bad want' else 'q', **kw)
        out['decode/listing/' + name] = (call, ())

    for kind in ('layer_ends', 'front_ends'):
        def session(pred, pred17, kind=kind):
            results = []
            for refused in (lambda: pred.open_layers(SHAPES, TH, TW), lambda: pred.open_layers(SHAPES, TH, TW, ENDS, front_ends=ENDS),
                            lambda: pred.open_layers(SHAPES, TH, TW, max_workspace_bytes=1000, **{kind: ENDS}),
                            lambda: pred17.open_layers(SHAPES, TH, TW, **{kind: ENDS})):
                try:
                    refused()
                except ValueError as e:
                    results.append(str(e))
            s = pred.open_layers(SHAPES, TH, TW, **{kind: ENDS})
            volumes = decode_volumes(True)
            for want, layers in (('q', [[1, 1, 0, 1], [1, 1]]), ('symbols', [[2, 2, 0, 2], [2, 2]]), ('both', [[1, 2, 0, 2], [2, 2]]),
                                 ('both', [[2, 2, 0, 2], [2, 2]]), ('q', [[2, 0, 0, 2], [2, 2]]), ('q', [[2, 0, 0, 2], [2, 2]])):
                results.append(s.advance(volumes if want != 'symbols' else [v[:2] for v in volumes], layers, want=want))
                results.append([s.entry, s.fronts, s.launches, [list(d) for d in s.done], [[list(p) if p else p for p in row] for row in s.place],
                                s.shapes, [list(g) for g in s.grids], int(s.ws.numel()), list(s.sym.shape), list(s.q.shape)])
            for layers in ([[3, 0, 0, 2], [2, 2]], [[2, 0, 1, 2], [2, 2]], [[2, 0, 0, 2]]):
                try:
                    s.advance(volumes, layers)
                except ValueError as e:
                    results.append(str(e))
            return results
        out['session/' + kind] = (session, [0] * 15 + [0, 1, 0, 0, 0])

    zs = [torch.as_tensor(np.random.RandomState(7 + n).randn(*shape).astype(np.float32)) for n, shape in enumerate(SHAPES)]
    lams = OrderedDict([('float', 0.01), ('per tile', [[0.0, 0.5, 1.0, 2.0], [0.25, 0.125]])])
    for (lname, lam), which, script, want in itertools.product(lams.items(), (None, 'two', 'four', 'below'), ((), [0, 0, 0, 0, 1, 0]), ('symbols', 'both')):
        if (which == 'below' or want == 'both') and script:
            continue

        def choose(pred, pred17, lam=lam, which=which, want=want):
            return pred.choose_tiles_batch(zs, TH, TW, lam, want=want, **budget(which, _SIZE.format(''), False))
        out['choose/{}/{}/{}/{}'.format(lname, want, which or 'unlimited', 'status 1' if script else 'ok')] = (choose, script)

    def choose_refused(pred, pred17):
        results = []
        for refused in (lambda: pred17.choose_tiles_batch(zs, TH, TW, 0.5), lambda: pred.choose_tiles_batch(zs, TH, TW, 0.5, want='z'),
                        lambda: pred.choose_tiles_batch(zs, TH, TW, [[0.5] * 4]), lambda: pred.choose_tiles_batch([zs[0], zs[1][:3]], TH, TW, 0.5),
                        lambda: pred.choose_tiles_batch([zs[0].double()], TH, TW, 0.5)):
            try:
                refused()
            except ValueError as e:
                results.append(str(e))
        return results
    out['choose/refusals'] = (choose_refused, ())

    for mode, kw in ENCODE_MODES.items():
        units = 4 * (len(ENDS) if mode in ('layers', 'fronts') else 1)
        for status in (0, 1, 2, 3):
            def encode(pred, pred17, kw=kw):
                return pred.encode_tiles_batch([symbols(SHAPES[0], 1)], TH, TW, **kw)
            out['encode/{}/status {}'.format(mode, status)] = (encode, [0] * (units - 1) + [status])

    def encode_two(pred, pred17):
        return [pred.encode_tiles_batch([symbols(s, 2 + n) for n, s in enumerate(SHAPES)], TH, TW, **kw) for kw in ENCODE_MODES.values()]
    out['encode/two volumes'] = (encode_two, ())

    def encode_stream(pred, pred17):
        sym, results = symbols((3,) + SHAPES[0], 5), []
        for kw in ({}, {'capacity': 40}, {'order': 'wavefront', 'capacity': 40}, {'seg_ends': [9, 36]}, {'order': 'rans'},
                   {'order': 'wavefront', 'depth_block': 2}, {'order': 'rans', 'seg_ends': [36]}, {'lanes': 8}, {'order': 'spiral'},
                   {'depth_block': 2}, {'order': 'wavefront', 'seg_ends': [36]}, {'seg_ends': [36, 9]}):
            try:
                results.append(pred.encode_stream(sym, **kw))
                results.append(pred.encode_stream(sym[0], **kw))
            except ValueError as e:
                results.append(str(e))
        results.append(pred.encode_stream(symbols((1, 1, 1), 6), order='rans'))
        return results
    out['encode/stream'] = (encode_stream, ())

    single = decode_volumes(False, SHAPES[:1], None)[0]
    tiles_calls = OrderedDict([
        ('direct', lambda p, p17: p.decode_tiles(single[0], single[1], SHAPES[0], TH, TW)),
        ('direct flags', lambda p, p17: p.decode_tiles(single[0], single[1], SHAPES[0], TH, TW, flags=1)),
        ('direct k 17', lambda p, p17: p17.decode_tiles(single[0], single[1], SHAPES[0], TH, TW)),
        ('channels', lambda p, p17: p.decode_tiles(single[0], single[1], SHAPES[0], TH, TW, channels=2)),
        ('rans', lambda p, p17: p.decode_tiles(single[0], single[1], SHAPES[0], TH, TW, order='rans', lanes=32)),
        ('wavefront', lambda p, p17: p.decode_tiles(single[0], single[1], SHAPES[0], TH, TW, order='wavefront')),
        ('counts', lambda p, p17: p.decode_tiles(single[0][:2], single[1], SHAPES[0], TH, TW)),
        ('channels k 17', lambda p, p17: p17.decode_tiles(single[0], single[1], SHAPES[0], TH, TW, channels=2)),
    ])
    for name, call in tiles_calls.items():
        for script in ((), [0, 0, 1, 0]):
            out['tiles/{}/{}'.format(name, 'status 1' if script else 'ok')] = (call, script)
    for name, kw in (('plain', {}), ('channels', {'channels': 2}), ('on device', {'on_device': True, 'flags': 3})):
        for script in ((), [1]):
            def stream(pred, pred17, kw=kw):
                return pred.decode_stream(b'\x01\x02\x03\x04\x05', SHAPES[0], 4, **kw)
            out['stream/{}/{}'.format(name, 'status 1' if script else 'ok')] = (stream, script)
    out['stream/empty'] = (lambda p, p17: p.decode_stream(b'', SHAPES[1], 0), ())
    out['stream/channels k 17'] = (lambda p, p17: p17.decode_stream(b'\x01', SHAPES[1], 0, channels=1), ())
    return out


# ---- the refusal grid -----------------------------------------------------------------------------------------------------------------

GRID = OrderedDict([
    ('conceal', (False, True)), ('order', ('raster', 'wavefront', 'rans', 'spiral')), ('channels', (None, 2)), ('layer_ends', (None, ENDS)),
    ('tile_layers', (None, [[1]])), ('front_ends', (None, ENDS)), ('depth_block', (None, 2)), ('lanes', (None, 16)), ('flags', (0, 1)),
    ('k', (24, 17)),
])


def refusal_grid(pred, pred17):
    """decode_tiles_batch of one tile under the full product of GRID -> (messages, [index into messages per combination]); 'ok' for
    a call that went through"""
    messages, codes = ['ok'], []
    for combination in itertools.product(*GRID.values()):
        kw = dict(zip(GRID, combination))
        p = pred if kw.pop('k') == 24 else pred17
        segments = kw['layer_ends'] is not None or kw['front_ends'] is not None
        try:
            p.decode_tiles_batch(decode_volumes(segments, [(4, 2, 2)], None), TH, TW, **kw)
            message = 'ok'
        except ValueError as e:
            message = str(e)
        if message not in messages:
            messages.append(message)
        codes.append(messages.index(message))
    return messages, codes


def record_all(recorder):
    """everything the golden file holds, from the coders as they are"""
    pred, pred17 = prediction_network(24), prediction_network(17)
    out = OrderedDict()
    out['cases'] = OrderedDict((name, run(recorder, lambda: call(pred, pred17), script)) for name, (call, script) in cases().items())
    recorder.begin()
    messages, codes = refusal_grid(pred, pred17)
    out['grid'] = {'axes': OrderedDict((k, [shown(v) for v in vs]) for k, vs in GRID.items()), 'messages': messages,
                   'codes': ' '.join(str(c) for c in codes)}
    return out
