"""-m gpu: rate-aware symbol choice at encode (IC_PC_DECODE_RDO on ic_pc_decode_tiles_batch_channels_f32, Codec.compress(rdo=...)).
The sweep raw through the C ABI against the rule of tests/rdo_rule.py in its teacher-forced form -- every chosen symbol equals the
rule on (z, the row of pred.get_all over the final symbols of its tile), which by induction over T is the sequential rule -- and
against the product's host statement codec.rdo_choose; then whole files.  Every device buffer comes from tests.fenced.fenced(), the
workspace has exactly the queried size and is handed over dirty (0xFF, then 0x00; the outputs must be bit-identical), every
comparison is an equality."""
import ctypes
import json

import numpy as np
import pytest
import torch

from tests import rdo_rule as rule
from tests.fenced import OUT_FENCE, IN_FENCE, check_fences, fenced, poison, snapshot, unchanged
from tests.test_gpu_codec_decoder import _load, _model

pytestmark = pytest.mark.gpu

LAM = 0.05             # key units (squared distance) per bit: a fraction of the squared centre spacing


@pytest.fixture(scope='module')
def pred(cuda, configs, syn_weights):
    return _load(cuda, configs[0], configs[1], syn_weights, 1e9)


def _centres(model):
    return model.centers.detach().contiguous().float().cpu().numpy()


def _z(model, shape, seed):
    """values over the centres' range and beyond, and on every midpoint between neighbouring centres and 1 ulp to either side"""
    c = np.sort(_centres(model))
    rs = np.random.RandomState(seed)
    z = rs.uniform(c[0] - 0.7, c[-1] + 0.7, size=shape).astype(np.float32)
    mids = ((c[:-1].astype(np.float64) + c[1:]) / 2).astype(np.float32)
    special = np.concatenate([mids, np.nextafter(mids, np.float32(np.inf)), np.nextafter(mids, np.float32(-np.inf)), c])
    flat = z.reshape(-1)
    where = rs.permutation(flat.size)[:min(flat.size // 2, 4 * special.size)]
    flat[where] = special[rs.randint(0, special.size, size=where.size)]
    return z


def _raw_rdo(cuda, model, zs, th, tw, lams, want_syms=True, want_q=True, flags=None, K=None, mangle=None, caller_model=None, raw_lambda=False):
    """the entry with IC_PC_DECODE_RDO (or `flags`) on fenced buffers.  zs: [(C, h, w) float32 numpy]; lams: per volume a lambda or
    one per tile.  The records lie 8-aligned in one buffer between NaN fences, the gaps NaN too.  Two runs over a workspace of
    0xFF, then 0x00: bit-identical outputs.  mangle(rows) may damage the tile table.  raw_lambda: lams hold the records' Lambda
    itself, any f64, one per tile.  -> (rc, [symbols], [q], status list)"""
    from imgcomp_cvpr_amd import _lib, codec
    model = caller_model or model
    flags = _lib.PC_DECODE_RDO if flags is None else flags
    rows, parts, pos = [], [], 0
    for n, z in enumerate(zs):
        C, h, w = z.shape
        grid = codec.tile_grid(h, w, th, tw)
        for (y0, x0, a, b), lm in zip(grid, lams[n] if raw_lambda else codec.rdo_tile_lambdas(lams[n], len(grid))):
            rec = rule.record(lm if raw_lambda else rule.lambda_q(lm), z[:, y0:y0 + a, x0:x0 + b])
            assert len(rec) == rule.record_bytes(C, a, b) == codec.rdo_record_bytes(C, a, b)
            assert rec == codec.rdo_record(lm if raw_lambda else codec.rdo_lambda_q(lm), z[:, y0:y0 + a, x0:x0 + b])
            rows.append([y0, x0, a, b, pos, len(rec), -7, n])                  # first_sym is ignored on input
            pad = (-len(rec)) % 8
            parts.append(rec + b'\xff' * pad)
            pos += len(rec) + pad
    if mangle:
        mangle(rows)
    shapes = [z.shape for z in zs]
    C = shapes[0][0]
    table = _lib.tile_table(rows)
    vtable, offs, total = _lib.packed_volume_table(shapes)
    data = fenced(torch.frombuffer(bytearray(b''.join(parts)), dtype=torch.uint8), torch.uint8, cuda, IN_FENCE, 'records')
    need = int(_lib.lib.ic_pc_decode_tiles_batch_workspace_bytes(C, max(r[2] for r in rows), max(r[3] for r in rows), len(rows), len(zs),
                                                                 model.pc._k))
    centers = fenced(model.centers.contiguous().float(), torch.float32, cuda, IN_FENCE, 'centres')
    runs = []
    for byte in (0xFF, 0x00):
        sym = fenced((total,), torch.int64, cuda, OUT_FENCE, 'symbols') if want_syms else None
        q = fenced((total,), torch.float32, cuda, OUT_FENCE, 'q') if want_q else None
        status = fenced((len(rows),), torch.int32, cuda, OUT_FENCE, 'status')
        ws = poison(fenced((need,), torch.uint8, cuda, OUT_FENCE, 'workspace'), byte)
        before = snapshot(sym, q, status, ws)
        rc = _lib.lib.ic_pc_decode_tiles_batch_channels_f32(
            _lib.ptr(data), pos, table, len(rows), vtable, len(zs), model.pc._tab, _lib.ptr(centers), model.pc._k, model.pc.L,
            model.freqs_resolution, _lib.ptr(sym), _lib.ptr(q), _lib.ptr(status), C, _lib.ptr(ws), need, int(flags),
            _lib.current_stream(cuda), C if K is None else int(K), 0)
        torch.cuda.synchronize()
        check_fences(data, centers, sym, q, status, ws)
        if rc != 0:
            unchanged(before, sym, q, status, ws)                            # a refused call wrote nothing
            return rc, None, None, None
        runs.append((None if sym is None else sym.clone(), None if q is None else q.clone(), status.tolist()))
    (s0, q0, st0), (s1, q1, st1) = runs
    assert st0 == st1 and (s0 is None or torch.equal(s0, s1)) and (q0 is None or torch.equal(q0.view(torch.int32), q1.view(torch.int32))), \
        'the outputs depend on what the workspace held'
    cut = lambda buf: [buf[o:o + c * h * w].view(c, h, w) for (c, h, w), o in zip(shapes, offs)]
    if want_syms and want_q:
        for s, qq in zip(cut(s0), cut(q0)):
            assert int(s.min()) >= 0 and int(s.max()) < model.pc.L
            assert torch.equal(qq, model.centers.contiguous().float()[s]), 'q is not centers[symbols], bit for bit'
    return rc, [s.cpu().numpy() for s in cut(s0)] if want_syms else None, cut(q0) if want_q else None, st0


def _device_hard(cuda, model, z):
    """the quantiser's symbols of z (ic_quantize_f32)"""
    from imgcomp_cvpr_amd import _lib
    dz = fenced(z, torch.float32, cuda, IN_FENCE, 'z')
    centers = fenced(model.centers.contiguous().float(), torch.float32, cuda, IN_FENCE, 'centres')
    out = fenced(z.shape, torch.int64, cuda, OUT_FENCE, 'quantiser symbols')
    rc = _lib.lib.ic_quantize_f32(_lib.ptr(dz), _lib.ptr(centers), model.pc.L, 1.0, None, None, _lib.ptr(out), z.size, _lib.current_stream(cuda))
    torch.cuda.synchronize()
    assert rc == 0
    check_fences(dz, centers, out)
    return out.cpu().numpy()


def _holds(model, sym, z, th, tw, lams, rows_of=None):
    """every symbol of every tile is the rule's -- tests/rdo_rule.py and codec.rdo_choose -- on (z, the row of get_all over the
    tile's final symbols); the first position is the quantiser's symbol"""
    from imgcomp_cvpr_amd import codec
    cen = _centres(model)
    C, h, w = sym.shape
    grid = codec.tile_grid(h, w, th, tw)
    changed = 0
    for (y0, x0, a, b), lm in zip(grid, codec.rdo_tile_lambdas(lams, len(grid))):
        ts, tz = sym[:, y0:y0 + a, x0:x0 + b], z[:, y0:y0 + a, x0:x0 + b]
        rows = model.get_all(model.pad_symbols_volume(ts))[1].reshape(C, a, b, -1) if rows_of is None else rows_of(C, a, b)
        lq = rule.lambda_q(lm)
        assert lq == codec.rdo_lambda_q(lm)
        bad, status = rule.sweep_holds(ts, tz, cen, lq, rows)
        assert bad == [] and status == 0, ((y0, x0), lm, bad[:5])
        for c, y, x in ((0, 0, 0), (C - 1, a - 1, b - 1), (C // 2, a // 2, b // 2)):
            rated = (c, y, x) != (0, 0, 0)
            assert codec.rdo_choose(tz[c, y, x], rows[c, y, x], cen, lq, rated) == (int(ts[c, y, x]), 0)
        assert int(ts[0, 0, 0]) == rule.hard(tz[0, 0, 0], cen)
        changed += int(sum(int(ts[c, y, x]) != rule.hard(tz[c, y, x], cen) for c in range(C) for y in range(a) for x in range(b)))
    return changed


EXTENTS = {
    '1x1x1': ([(1, 1, 1)], 1, 1),
    'Cx1x1': ([(8, 1, 1)], 1, 1),
    '5x7 cut by 4x4': ([(4, 5, 7)], 4, 4),
    '16x16x16': ([(16, 16, 16)], 16, 16),
    'two volumes': ([(4, 5, 7), (4, 9, 6)], 4, 4),
}


@pytest.mark.parametrize('name', sorted(EXTENTS))
def test_the_sweep_is_the_rule(cuda, pred, name):
    shapes, th, tw = EXTENTS[name]
    zs = [_z(pred, s, 10 + i + len(name)) for i, s in enumerate(shapes)]
    lams = [LAM] * len(zs)
    rc, syms, qs, status = _raw_rdo(cuda, pred, zs, th, tw, lams)
    assert rc == 0 and status == [0] * len(status), (rc, status)
    changed = sum(_holds(pred, s, z, th, tw, LAM) for s, z in zip(syms, zs))
    print('{}: {} of {} symbols differ from the quantiser\'s at lambda {}'.format(name, changed, sum(z.size for z in zs), LAM))
    if name == '16x16x16':
        assert changed > 0, 'lambda {} moves no symbol: the test shows nothing'.format(LAM)
    # lambda = 0: the quantiser everywhere, midpoints +- 1 ulp included
    rc, hard, _, status = _raw_rdo(cuda, pred, zs, th, tw, [0.0] * len(zs))
    assert rc == 0 and status == [0] * len(status)
    for s, z in zip(hard, zs):
        assert np.array_equal(s, _device_hard(cuda, pred, z))
    # symbols alone, q alone: the same values
    rc, s_only, none, _ = _raw_rdo(cuda, pred, zs, th, tw, lams, want_q=False)
    assert rc == 0 and none is None and all(np.array_equal(a, b) for a, b in zip(s_only, syms))
    rc, none, q_only, _ = _raw_rdo(cuda, pred, zs, th, tw, lams, want_syms=False)
    assert rc == 0 and none is None and all(torch.equal(a, b) for a, b in zip(q_only, qs))
    # the surface function gathers the same records on the device
    both = pred.choose_tiles_batch([fenced(z, torch.float32, cuda, IN_FENCE, 'z') for z in zs], th, tw, LAM, want='both')
    assert all(np.array_equal(b[1].cpu().numpy(), s) and torch.equal(b[0], q) for b, s, q in zip(both, syms, qs))


def test_lambda_per_tile(cuda, pred):
    from imgcomp_cvpr_amd import codec
    z = _z(pred, (4, 9, 10), 3)
    n = len(codec.tile_grid(9, 10, 4, 4))
    lams = [0.0, 0.3, 0.01, 0.1, 1.0, 0.0, 0.05, 0.2, 3.0][:n]
    assert len(lams) == n
    rc, syms, _, status = _raw_rdo(cuda, pred, [z], 4, 4, [lams])
    assert rc == 0 and status == [0] * n
    _holds(pred, syms[0], z, 4, 4, lams)
    uniform = _raw_rdo(cuda, pred, [z], 4, 4, [0.3])[1][0]
    y0, x0, a, b = codec.tile_grid(9, 10, 4, 4)[1]
    assert np.array_equal(uniform[:, y0:y0 + a, x0:x0 + b], syms[0][:, y0:y0 + a, x0:x0 + b])       # the tile whose lambda is 0.3
    assert not np.array_equal(uniform, syms[0])
    got = pred.choose_tiles_batch([fenced(z, torch.float32, cuda, IN_FENCE, 'z')], 4, 4, [lams])[0]
    assert np.array_equal(got.cpu().numpy(), syms[0])
    with pytest.raises(ValueError, match='lambdas for'):
        pred.choose_tiles_batch([fenced(z, torch.float32, cuda, IN_FENCE, 'z')], 4, 4, [lams[:-1]])


HARD = {
    'L = 6, floor rows': [0.0, 20.0, 20.0, 20.0, 20.0, 20.0],
    'L = 6, one large entry': [30.0, 0.0, 0.0, 0.0, 0.0, 0.0],
    'L = 2': [0.0, 3.0],
    'L = 16': [float(j % 5) for j in range(16)],
}


@pytest.mark.parametrize('name', sorted(HARD))
def test_hard_tables(cuda, name):
    """a constant table: the rule needs no network.  A very large lambda takes the first most frequent symbol everywhere but at
    the first position"""
    model, table = _model(cuda, HARD[name])
    shape = (4, 5, 7)
    z = _z(model, shape, len(name))
    const = lambda C, a, b: np.broadcast_to(np.asarray(table, np.int64), (C, a, b, len(table)))
    for lam in (0.0, LAM, 0.5):
        rc, syms, _, status = _raw_rdo(cuda, model, [z], 5, 7, [lam])
        assert rc == 0 and status == [0]
        changed = _holds(model, syms[0], z, 5, 7, lam, rows_of=const)
        print('{}: table {}, lambda {}: {} of {} symbols differ from the quantiser\'s'.format(name, table, lam, changed, z.size))
        assert (changed == 0) == (lam == 0.0 or len(set(table)) == 1)
    zf = np.clip(z, -10.0, 10.0)
    rc, syms, _, status = _raw_rdo(cuda, model, [zf], 5, 7, [1e30])
    assert rc == 0 and status == [0]
    want = np.full(shape, int(np.argmax(table)), np.int64)
    want[0, 0, 0] = rule.hard(zf[0, 0, 0], _centres(model))
    assert np.array_equal(syms[0], want)


def _first_min(costs):
    best, sym = float('inf'), 0
    for j, v in enumerate(costs):
        if v < best:
            best, sym = v, j
    return sym


def _near_ties(table, centres, seed, tries=400, reach=300):
    """(z, Lambda) at which the rule's cost -- one rounded multiply, one rounded add -- and a fused multiply-add, which rounds
    k + Lambda R once, decide differently: for random z the Lambda that ties the nearest centre with the cheapest symbol is solved
    for and stepped `reach` ulps to either side.  Host arithmetic only: Python floats for the two roundings, exact fractions
    rounded once for the fused form."""
    from fractions import Fraction
    R = rule.rates(table)
    cheap = _first_min(R)
    rs = np.random.RandomState(seed)
    out = []
    for z in rs.uniform(float(centres.min()) - 0.5, float(centres.max()) + 0.5, size=tries).astype(np.float32):
        k = [float(rule.key(z, c)) for c in centres]
        near = _first_min(k)
        if near == cheap or R[near] == R[cheap]:
            continue
        lam = np.float64((k[cheap] - k[near]) / (R[near] - R[cheap]))
        for _ in range(reach):
            lam = np.nextafter(lam, -np.inf)
        for _ in range(2 * reach):
            lq = float(lam)
            costs = [k[j] + lq * R[j] for j in range(len(k))]
            two, low = _first_min(costs), sorted(costs)
            # (a fused cost lies within an ulp of the two-rounding cost: only a gap of a few ulps can turn the decision)
            if low[1] - low[0] <= 4 * float(np.spacing(low[1])):
                fused = _first_min([float(Fraction(k[j]) + Fraction(lq) * R[j]) for j in range(len(k))])
                if two != fused:
                    out.append((z, lq, two, fused))
            lam = np.nextafter(lam, np.inf)
    return out


@pytest.mark.parametrize('name', ['L = 2', 'L = 6, one large entry'])
def test_the_cost_is_two_roundings_not_a_fused_multiply_add(cuda, name):
    """Lambda is the caller's f64: at a near-tie one rounding of k + Lambda R and two roundings pick different symbols.  A constant
    table fixes R, z fixes k; every (z, Lambda) found, and Lambda one ulp to either side, is a tile of one launch: a raw position 0
    and the position in question"""
    model, table = _model(cuda, HARD[name])
    cen = _centres(model)
    cases = _near_ties(table, cen, seed=len(name))
    print('{}: {} (z, Lambda) where a fused cost decides differently, e.g. {}'.format(name, len(cases), cases[:2]))
    assert len(cases) >= 1, 'the search found no near-tie: the test shows nothing'
    tiles = [(z, lq) for z, lam, _, _ in cases[:40] for lq in (float(np.nextafter(lam, -np.inf)), lam, float(np.nextafter(lam, np.inf)))]
    zvol = np.zeros((1, 1, 2 * len(tiles)), np.float32)
    zvol[0, 0, 1::2] = [z for z, _ in tiles]
    rc, syms, _, status = _raw_rdo(cuda, model, [zvol], 1, 2, [[lq for _, lq in tiles]], raw_lambda=True)
    assert rc == 0 and status == [0] * len(tiles)
    got = syms[0][0, 0, 1::2].tolist()
    want = [rule.choose(z, table, cen, lq)[0] for z, lq in tiles]
    assert got == want, [(t, g, w) for t, g, w in zip(tiles, got, want) if g != w][:5]
    from imgcomp_cvpr_amd import codec
    assert want == [codec.rdo_choose(z, table, cen, lq)[0] for z, lq in tiles]
    # and these are positions where it matters: the fused form's symbols are others
    assert [want[3 * i + 1] for i in range(len(cases[:40]))] == [two for _, _, two, _ in cases[:40]]
    assert all(two != fused for _, _, two, fused in cases)


def test_a_total_over_the_limit_is_status_1_and_decided_without_rates(cuda):
    """the resolution at which a constant row's total is just above 2^30 + 2, found on the device as the rANS tests find it, and
    the nearest one below at which it is within"""
    from tests.test_gpu_codec_decoder import _device_tables
    from tests.util import dev
    bias, shape = [0.0, 1.0, 2.0, 3.0, 2.0, 1.0], (4, 5, 7)
    found = {}
    for res in (1.0737418e9 + 64.0 * k for k in range(-40, 41)):
        res = float(np.float32(res))
        total = int(_device_tables(dev(np.asarray(bias, np.float32)[None], cuda), res)[0].sum())
        found.setdefault(total > rule.MAX_TOTAL, (res, total))
    assert True in found and False in found, found
    over, table = _model(cuda, bias, resolution=found[True][0])
    assert sum(table) > rule.MAX_TOTAL
    z = _z(over, shape, 2)
    rc, syms, _, status = _raw_rdo(cuda, over, [z], 5, 7, [0.5])
    assert rc == 0 and status == [1]
    assert np.array_equal(syms[0], _device_hard(cuda, over, z))              # all R_j = 0: the quantiser's symbols
    bad, st = rule.sweep_holds(syms[0], z, _centres(over), rule.lambda_q(0.5), np.broadcast_to(np.asarray(table, np.int64), shape + (6,)))
    assert bad == [] and st == 1
    with pytest.raises(ValueError, match='total is too large'):
        over.choose_tiles_batch([fenced(z, torch.float32, cuda, IN_FENCE, 'z')], 5, 7, 0.5)
    within, table = _model(cuda, bias, resolution=found[False][0])
    rc, syms, _, status = _raw_rdo(cuda, within, [z], 5, 7, [0.5])
    assert rc == 0 and status == [0] and not np.array_equal(syms[0], _device_hard(cuda, within, z))
    _holds(within, syms[0], z, 5, 7, 0.5, rows_of=lambda C, a, b: np.broadcast_to(np.asarray(table, np.int64), (C, a, b, 6)))


def test_refusals_write_nothing(cuda, pred, configs):
    from imgcomp_cvpr_amd import _lib, config_parser as cp, weights as Wt
    shape = (4, 5, 7)
    z = _z(pred, shape, 1)
    R, WF = _lib.PC_DECODE_RDO, _lib.PC_DECODE_WAVEFRONT
    assert _raw_rdo(cuda, pred, [z], 5, 7, [LAM])[0] == 0
    for flags in (R | WF, R | _lib.PC_DECODE_RANS(8), R | _lib.PC_DECODE_DEPTH(2), R | WF | _lib.PC_DECODE_DEPTH(2), R | _lib.PC_DECODE_RECOMPUTE,
                  R | _lib.PC_DECODE_PER_LAYER, R | 0x2000000):
        assert _raw_rdo(cuda, pred, [z], 5, 7, [LAM], flags=flags)[0] == -2, hex(flags)
    for K in (1, 3):
        assert _raw_rdo(cuda, pred, [z], 5, 7, [LAM], K=K)[0] == -2, K        # channels < C
    pc64, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow_64'))
    pred64 = _load(cuda, configs[0], pc64, Wt.synthetic_weights(configs[0], pc64), 1e9)
    assert _raw_rdo(cuda, pred, [z], 5, 7, [LAM], caller_model=pred64)[0] == -2
    with pytest.raises(ValueError, match='k = 24, this one has k = 64'):
        pred64.choose_tiles_batch([fenced(z, torch.float32, cuda, IN_FENCE, 'z')], 5, 7, LAM)

    # a record of wrong length, a misaligned offset: IC_ERR_ARG
    def longer(rows):
        rows[1][5] += 4

    def shorter(rows):
        rows[0][5] -= 4

    def misaligned(rows):
        rows[1][4] += 4
        rows[1][5] -= 0

    for mangle in (longer, shorter, misaligned):
        assert _raw_rdo(cuda, pred, [z, z], 5, 7, [LAM, LAM], mangle=mangle)[0] == -1, mangle.__name__

    # the other entries, each with arguments it would otherwise serve
    lib, ptr = _lib.lib, _lib.ptr
    C, h, w = shape
    rec = rule.record(rule.lambda_q(LAM), z)
    tiles = [(0, 0, h, w, 0, len(rec), 0, 0)]
    table, nt, pos = _lib.tile_table(tiles), 1, len(rec)
    vtable, _, total = _lib.packed_volume_table([shape])
    data = fenced(torch.frombuffer(bytearray(rec), dtype=torch.uint8), torch.uint8, cuda, IN_FENCE, 'record')
    centers = fenced(pred.centers.contiguous().float(), torch.float32, cuda, IN_FENCE, 'centres')
    ends = (ctypes.c_int * 1)(C)
    segs = _lib.seg_table([(0, pos)])
    limits, zeros = (ctypes.c_int * nt)(C), (ctypes.c_int * nt)(0)
    k, Lm, res, tab, stream = pred.pc._k, pred.pc.L, pred.freqs_resolution, pred.pc._tab, _lib.current_stream(cuda)
    fill = pred.conceal_fallback()

    def refused(name, need, call):
        out = fenced((total,), torch.int64, cuda, OUT_FENCE, name + ' symbols')
        q = fenced((total,), torch.float32, cuda, OUT_FENCE, name + ' q')
        status = fenced((nt,), torch.int32, cuda, OUT_FENCE, name + ' status')
        ws = poison(fenced((int(need),), torch.uint8, cuda, OUT_FENCE, name + ' workspace'), 0xFF)
        before = snapshot(out, q, status, ws)
        for flags in (R, R | WF):
            rc = call(out, q, status, ws, int(need), flags)
            torch.cuda.synchronize()
            assert rc == -2, (name, hex(flags), rc)
            check_fences(data, centers, out, q, status, ws)
            unchanged(before, out, q, status, ws)

    batch = lambda out, q, status, ws, need, flags: (ptr(data), pos, table, nt, vtable, 1, tab, ptr(centers), k, Lm, res, ptr(out), ptr(q),
                                                      ptr(status), C, ptr(ws), need, flags, stream)
    refused('ic_pc_decode_f32', lib.ic_pc_decode_workspace_bytes(C, h, w, k),
            lambda out, q, status, ws, need, flags: lib.ic_pc_decode_f32(ptr(data), pos, 0, tab, ptr(centers), k, Lm, res, ptr(out), ptr(status),
                                                                         C, h, w, ptr(ws), need, flags, stream))
    refused('ic_pc_decode_channels_f32', lib.ic_pc_decode_workspace_bytes(C, h, w, k),
            lambda out, q, status, ws, need, flags: lib.ic_pc_decode_channels_f32(ptr(data), pos, 0, tab, ptr(centers), k, Lm, res, ptr(out),
                                                                                  ptr(status), C, h, w, ptr(ws), need, flags, stream, C, fill))
    refused('ic_pc_decode_tiles_f32', lib.ic_pc_decode_tiles_workspace_bytes(C, h, w, nt, k),
            lambda out, q, status, ws, need, flags: lib.ic_pc_decode_tiles_f32(ptr(data), pos, table, nt, tab, ptr(centers), k, Lm, res, ptr(out),
                                                                               ptr(status), C, h, w, ptr(ws), need, flags, stream))
    refused('ic_pc_decode_tiles_batch_f32', lib.ic_pc_decode_tiles_batch_workspace_bytes(C, h, w, nt, 1, k),
            lambda *a: lib.ic_pc_decode_tiles_batch_f32(*batch(*a)))
    for kind in ('layers', 'fronts'):
        need = getattr(lib, 'ic_pc_decode_tiles_batch_{}_workspace_bytes'.format(kind))(C, h, w, nt, 1, k, 1)
        refused(kind, need, lambda *a: getattr(lib, 'ic_pc_decode_tiles_batch_{}_f32'.format(kind))(*(batch(*a) + (C, fill, ends, 1, segs))))
        need = getattr(lib, 'ic_pc_decode_tiles_batch_{}_pertile_workspace_bytes'.format(kind))(C, h, w, nt, 1, k, 1)
        refused(kind + ' pertile', need,
                lambda *a: getattr(lib, 'ic_pc_decode_tiles_batch_{}_pertile_f32'.format(kind))(*(batch(*a) + (limits, fill, ends, 1, segs))))
        need = getattr(lib, 'ic_pc_decode_tiles_batch_{}_resume_workspace_bytes'.format(kind))(C, h, w, nt, 1, k, 1)
        refused(kind + ' resume', need,
                lambda *a: getattr(lib, 'ic_pc_decode_tiles_batch_{}_resume_f32'.format(kind))(*(batch(*a) + (zeros, limits, fill, ends, 1, segs))))


# ---- files ------------------------------------------------------------------------------------------------------------------------------

H_IMG, W_IMG = 64, 96
FORMATS = (1, 2, 5, 6, 8, 10, 12)


def _image(H, W_, seed=9):
    from imgcomp_cvpr_amd import weights as Wt
    return np.ascontiguousarray(Wt.synthetic_image((1, 3, H, W_), 'natural', seed=seed)[0].transpose(1, 2, 0))


@pytest.fixture(scope='module')
def cdc(cuda, configs, syn_weights):
    from imgcomp_cvpr_amd import codec
    return codec.Codec(configs[0], configs[1], syn_weights, cuda)


def _as(c, version, fn):
    """run fn() with the Codec writing the given format, tiles of 4 x 4 cells (--tile 32)"""
    c.tile = None if version == 1 else (4, 4)
    c.checked, c.order = False, 'wavefront' if version == 5 else 'raster'
    c.layers = 'default' if version == 6 else None
    c.front_layers = 'default' if version == 8 else None
    c.depth_block = 2 if version == 10 else None
    c.rans = 'default' if version == 12 else None
    try:
        assert c.written_version() == version
        return fn()
    finally:
        c.tile, c.checked, c.order, c.layers, c.front_layers, c.depth_block, c.rans = None, False, 'raster', None, None, None, None


@pytest.fixture(scope='module')
def picture():
    return _image(H_IMG, W_IMG, seed=5)


@pytest.mark.parametrize('version', FORMATS)
def test_files_of_every_format(cdc, picture, version):
    def body():
        assert cdc.compress(picture, rdo=0) == cdc.compress(picture) == cdc.compress(picture, rdo=0.0)
        sym, enc, (H, W) = cdc.choose_symbols(picture, LAM)
        assert (H, W) == (H_IMG, W_IMG) and sym.shape == enc.symbols[0].shape
        data = cdc.compress(picture, rdo=LAM)
        got, c = cdc.decode_symbols(data)
        assert c.version == version and np.array_equal(got, sym.cpu().numpy())
        assert np.array_equal(cdc.decompress(data), cdc._image(sym.cpu().numpy(), c))
        counted = cdc.compress_counting(picture, LAM)
        assert counted == (data, int((sym != enc.symbols[0]).sum()), sym.numel()) and counted[1] > 0
        # the sweep ran over this format's coded volumes: each is the rule on its own tables
        z = enc.z[0].cpu().numpy()
        th, tw = (z.shape[1], z.shape[2]) if version == 1 else (4, 4)
        if version in (1, 2):
            _holds(cdc.pred, got, z, th, tw, LAM)
        return data
    data = _as(cdc, version, body)
    print('format {}: {} bytes with lambda {}, {} without'.format(version, len(data), LAM, len(_as(cdc, version, lambda: cdc.compress(picture)))))


def test_cap_rois_many_and_rd(cdc, picture, tmp_path):
    from imgcomp_cvpr_amd import codec

    def body():
        # with a cap and with rois the sweep runs over the capped z
        for kw in (dict(cap=3.0), dict(rois=[(16, 8, 32, 24)], background=2.0)):
            enc, _, _ = cdc.encode_symbols_capped(picture, **kw)
            sym, enc2, _ = cdc.choose_symbols(picture, LAM, **kw)
            assert torch.equal(enc.z, enc2.z) and torch.equal(enc.symbols, enc2.symbols)
            _holds(cdc.pred, sym.cpu().numpy(), enc.z[0].cpu().numpy(), 4, 4, LAM)
            assert cdc.decode_symbols(cdc.compress(picture, rdo=LAM, **kw))[0].tolist() == sym.cpu().numpy().tolist()
            assert cdc.compress(picture, rdo=0, **kw) == cdc.compress(picture, **kw)
        # compress_many element by element
        other = _image(40, 56, seed=3)
        n = len(codec.tile_grid(8, 12, 4, 4))
        per_tile = [0.02 * i for i in range(n)]
        many = cdc.compress_many([picture, other, picture, picture], caps=[None, 2.5, None, None], rdos=[LAM, 0.2, None, per_tile])
        assert many == [cdc.compress(picture, rdo=LAM), cdc.compress(other, cap=2.5, rdo=0.2), cdc.compress(picture),
                        cdc.compress(picture, rdo=per_tile)]
        assert len(set(many)) == 4
        # the rows of the table are measure(...) in every field, doubles compared by ==
        lams = [0.0, 0.01, LAM, 0.5]
        rows = cdc.rdo_curve(picture, lams)
        assert [lm for lm, _ in rows] == lams
        for lm, m in rows:
            assert m == cdc.measure(picture, cdc.compress(picture, rdo=lm)), lm
        return rows
    rows = _as(cdc, 5, body)
    print('\n'.join('lambda {:g}: {} bytes, PSNR {:.3f}'.format(lm, m.bytes, m.psnr) for lm, m in rows))
    with pytest.raises(ValueError, match='0 <= lambda < inf'):
        cdc.compress(picture, rdo=-1.0)
    with pytest.raises(ValueError, match='0 <= lambda < inf'):
        cdc.compress(picture, rdo=float('nan'))


def test_rd_command_rows(cdc, picture, tmp_path, cuda):
    """rd --rdo-levels: the JSON rows equal measure(img, compress(img, rdo=lambda)), the codec built as the command builds it"""
    from PIL import Image
    from imgcomp_cvpr_amd import codec, weights as Wt
    src, out = str(tmp_path / 'in.png'), str(tmp_path / 'rd.json')
    Image.fromarray(picture).save(src)
    assert codec.main(['rd', src, out, '--tile', '32', '--wavefront', '--rdo-levels', '0,0.05,0.5', '--device', str(cuda)]) == 0
    table = json.load(open(out))
    assert table['format'] == 5 and [r['rdo'] for r in table['rows']] == [0.0, 0.05, 0.5]
    c2 = codec.Codec(*_cli_configs(), Wt.synthetic_weights(*_cli_configs(), seed=1234), cuda, tile=(4, 4), order='wavefront')
    for r in table['rows']:
        m = c2.measure(picture, c2.compress(picture, rdo=r['rdo']))
        assert dict(m._asdict(), rdo=r['rdo']) == r


def _cli_configs():
    from imgcomp_cvpr_amd import config_parser as cp
    ae, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    return ae, pc


def test_a_model_of_another_width_is_refused_when_asked(cuda, configs, picture):
    from imgcomp_cvpr_amd import codec, config_parser as cp, weights as Wt
    pc64, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow_64'))
    c64 = codec.Codec(configs[0], pc64, Wt.synthetic_weights(configs[0], pc64), cuda)
    assert 'k = 24, this one has k = 64' in c64.rdo_refusal
    small = picture[:32, :32]
    assert c64.compress(small) == c64.compress(small, rdo=None)               # raised only when rdo is asked for
    for call in (lambda: c64.compress(small, rdo=0.0), lambda: c64.choose_symbols(small, 0.1), lambda: c64.compress_many([small], rdos=[0.1]),
                 lambda: c64.rdo_curve(small, [0.1])):
        with pytest.raises(ValueError, match='rate-aware symbol choice.*k = 24, this one has k = 64'):
            call()
