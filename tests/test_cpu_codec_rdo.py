"""Rate-aware symbol choice at encode, host side: the integer log2, the rule of one position (tests/rdo_rule.py against the product's
statement in codec.py), the two forms of a sweep on a toy causal table function, the record and its checks, the option and refusal
sentences, the header's macro.  No device."""
import argparse
import math
import os
import re
import struct

import numpy as np
import pytest

from imgcomp_cvpr_amd import _lib, codec
from tests import rdo_rule as rule

EDGES = (1, 2, 3, 4, 5, 7, 8, 1000, 65535, 65536, 65537, (1 << 30) + 2, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 1)


def test_ilog2_q16():
    assert rule.ilog2_q16(3) == codec.ilog2_q16(3) == 103872
    for e in range(32):
        assert rule.ilog2_q16(1 << e) == codec.ilog2_q16(1 << e) == e << 16       # exact on powers of two
    rs = np.random.RandomState(0)
    values = list(EDGES) + [int(v) for v in rs.randint(1, 1 << 32, size=3000, dtype=np.int64)] + \
        [int(v) for v in rs.randint(1, 1 << 12, size=500)]
    for v in values:
        r = rule.ilog2_q16(v)
        assert r == codec.ilog2_q16(v), v
        assert 0.0 <= math.log2(v) - r / 65536.0 + 1e-12 and abs(math.log2(v) - r / 65536.0) <= 2.0 ** -16, (v, r)
    prev = 0
    for v in range(1, 200001):                                                # monotone
        r = codec.ilog2_q16(v)
        assert r >= prev, v
        prev = r
    for bad in (0, -1, 1 << 32):
        with pytest.raises(ValueError, match='outside 1 .. 2\\^32 - 1'):
            codec.ilog2_q16(bad)


def test_lambda_q():
    for lam in (0, 0.0, 1e-3, 0.05, 1.0, 3, 1e30, np.float32(0.25), np.float64(2.0)):
        assert codec.rdo_lambda_q(lam) == rule.lambda_q(lam) == float(lam) * 1e7 / 65536.0
    for bad in (-1e-9, float('inf'), float('nan'), None, 'x', True, [0.1]):
        with pytest.raises(ValueError, match='0 <= lambda < inf'):
            codec.rdo_lambda_q(bad)


CENTRES = np.array([-1.7, -0.9, -0.1, 0.4, 1.1, 1.9], np.float32)


def _midpoint_values(c):
    mids = ((c[:-1].astype(np.float64) + c[1:]) / 2).astype(np.float32)
    return np.concatenate([mids, np.nextafter(mids, np.float32(np.inf)), np.nextafter(mids, np.float32(-np.inf)), c,
                           np.array([-5.0, 5.0, 0.0, -0.0, 1e20, -1e20, np.inf, -np.inf], np.float32)])


def test_lambda_zero_is_the_quantiser():
    """the first argmin of k_j whatever the row, also at the midpoints +- 1 ulp, at +-inf (every key inf: symbol 0) and at NaN"""
    rs = np.random.RandomState(1)
    zs = np.concatenate([_midpoint_values(CENTRES), rs.uniform(-3, 3, size=300).astype(np.float32), np.array([np.nan], np.float32)])
    rows = [[1, 1, 1, 1, 1, 1], [1, 10 ** 9, 5, 7, 1, 3], [10 ** 8] * 6]                 # (totals within 2^30 + 2)
    for z in zs:
        keys = [float(rule.key(z, c)) for c in CENTRES]
        want = 0
        for j in range(1, 6):
            if keys[j] < keys[want]:
                want = j
        assert rule.hard(z, CENTRES) == want
        for row in rows:
            for rated in (True, False):
                assert rule.choose(z, row, CENTRES, 0.0, rated) == (want, 0), (z, row)
                assert codec.rdo_choose(z, row, CENTRES, 0.0, rated) == (want, 0), (z, row)
    # unsorted centres and a tie between two equal centres: the first wins
    c2 = np.array([0.5, -0.5, 0.5, 2.0], np.float32)
    assert rule.choose(0.4, [1, 1, 1, 1], c2, 0.0) == codec.rdo_choose(0.4, [1, 1, 1, 1], c2, 0.0) == (0, 0)


def test_large_lambda_takes_the_first_most_frequent():
    rs = np.random.RandomState(2)
    lq = rule.lambda_q(1e30)
    for row in ([5, 900, 900, 3, 1, 1], [7, 7, 7, 7, 7, 7], [1, 2, 3, 4, 5, 10 ** 9], [10 ** 9, 1, 1, 1, 1, 1]):
        want = row.index(max(row))
        for z in rs.uniform(-3, 3, size=50).astype(np.float32):
            assert rule.choose(z, row, CENTRES, lq) == codec.rdo_choose(z, row, CENTRES, lq) == (want, 0)
            # the first position has no rate: the quantiser's symbol whatever lambda
            assert rule.choose(z, row, CENTRES, lq, rated=False) == codec.rdo_choose(z, row, CENTRES, lq, rated=False) == (rule.hard(z, CENTRES), 0)


def test_rule_and_statement_agree_and_a_nan_never_wins():
    rs = np.random.RandomState(3)
    for trial in range(400):
        L = int(rs.randint(1, 17))
        c = np.sort(rs.uniform(-2, 2, size=L).astype(np.float32))
        row = [int(v) for v in np.maximum(1, (rs.dirichlet(np.ones(L) * 0.3) * 1e9).astype(np.int64))]
        z = np.float32(rs.uniform(-2.5, 2.5))
        lq = rule.lambda_q(float(10.0 ** rs.uniform(-4, 1)))
        assert rule.choose(z, row, c, lq) == codec.rdo_choose(z, row, c, lq), (trial, z, row, lq)
    # a total above 2^30 + 2: status 1, decided without rates
    big = [1 << 29, 1 << 29, 3, 1, 1, 1]
    assert sum(big) > rule.MAX_TOTAL == codec.RANS_MAX_TOTAL
    for z in (-1.0, 0.3, 1.5):
        assert rule.choose(z, big, CENTRES, 5.0) == codec.rdo_choose(z, big, CENTRES, 5.0) == (rule.hard(z, CENTRES), 1)
    ok = [1 << 29, (1 << 29) - 2, 1, 1, 1, 1]
    assert sum(ok) == rule.MAX_TOTAL and rule.choose(0.3, ok, CENTRES, 5.0)[1] == 0 and codec.rdo_choose(0.3, ok, CENTRES, 5.0)[1] == 0
    # NaN costs: a NaN centre's key is NaN and never wins; all NaN (z NaN): symbol 0
    cn = np.array([np.nan, 0.0, 1.0], np.float32)
    for lq in (0.0, 3.0):
        assert rule.choose(0.9, [5, 5, 5], cn, lq) == codec.rdo_choose(0.9, [5, 5, 5], cn, lq) == (2, 0)
        assert rule.choose(np.nan, [5, 5, 5], cn, lq) == codec.rdo_choose(np.nan, [5, 5, 5], cn, lq) == (0, 0)
    # every key infinite: no cost is below inf, symbol 0
    assert rule.choose(np.float32(1e30), [1, 5, 5], [0.0, 1.0, 2.0], 3.0) == codec.rdo_choose(np.float32(1e30), [1, 5, 5], [0.0, 1.0, 2.0], 3.0) == (0, 0)


def _toy_rows(sym, pos, L):
    """a causal table function: the row of a position from the decided symbols of smaller T in its neighbourhood"""
    C, th, tw = sym.shape
    c, y, x = pos
    T = x + 2 * y + 4 * c
    acc = np.zeros(L, np.int64)
    for dc, dy, dx in ((0, 0, -1), (0, -1, 0), (0, -1, 1), (-1, 0, 0), (-1, 0, 1), (-1, 1, 0), (0, 0, -2)):
        cc, yy, xx = c + dc, y + dy, x + dx
        if 0 <= cc < C and 0 <= yy < th and 0 <= xx < tw:
            assert xx + 2 * yy + 4 * cc < T and sym[cc, yy, xx] >= 0, 'the toy function looked at an undecided position'
            acc[sym[cc, yy, xx]] += 3
            acc[(sym[cc, yy, xx] + 1) % L] += 1
    e = np.exp(acc.astype(np.float64) - acc.max())
    return [max(1, int(v)) for v in e / e.sum() * 1e9]


@pytest.mark.parametrize('shape', [(1, 1, 1), (3, 1, 1), (2, 3, 5), (4, 5, 7)])
def test_the_two_forms_of_a_sweep_agree(shape):
    rs = np.random.RandomState(sum(shape))
    L = len(CENTRES)
    z = rs.uniform(-2.2, 2.2, size=shape).astype(np.float32)
    order = rule.order(*shape)
    assert [t for t, _, _, _ in order] == sorted(t for t, _, _, _ in order) and order[0][1:] == (0, 0, 0)
    for lam in (0.0, 0.05, 0.5):
        lq = rule.lambda_q(lam)
        sym, status = rule.sweep_sequential(z, CENTRES, lq, lambda s, p: _toy_rows(s, p, L))
        assert status == 0 and sym.min() >= 0
        rows = np.zeros(shape + (L,), np.int64)
        for c in range(shape[0]):
            for y in range(shape[1]):
                for x in range(shape[2]):
                    rows[c, y, x] = _toy_rows(sym, (c, y, x), L)
        assert rule.sweep_holds(sym, z, CENTRES, lq, rows) == ([], 0)
        # the product's statement of the rule in both forms: the same sweep, and it holds on it
        sym2, status2 = rule.sweep_sequential(z, CENTRES, lq, lambda s, p: _toy_rows(s, p, L), choose=codec.rdo_choose)
        assert status2 == 0 and np.array_equal(sym2, sym)
        assert rule.sweep_holds(sym, z, CENTRES, lq, rows, choose=codec.rdo_choose) == ([], 0)
        if lam == 0.0:
            assert all(sym[c, y, x] == rule.hard(z[c, y, x], CENTRES) for _, c, y, x in order)
        elif z.size > 1:
            # the teacher-forced form is a test: it finds a symbol that is not the rule's
            other = sym.copy()
            other[-1, -1, -1] = (other[-1, -1, -1] + 1) % L
            assert rule.sweep_holds(other, z, CENTRES, lq, rows)[0] == [tuple(v - 1 for v in shape)]


def test_record():
    z = np.arange(24, dtype=np.float32).reshape(2, 3, 4) / 7
    lq = codec.rdo_lambda_q(0.05)
    rec = codec.rdo_record(lq, z)
    assert rec == rule.record(lq, z) and len(rec) == codec.rdo_record_bytes(2, 3, 4) == rule.record_bytes(2, 3, 4) == 8 + 4 * 24
    assert struct.unpack('<d', rec[:8])[0] == lq
    assert np.array_equal(np.frombuffer(rec[8:], '<f4').reshape(2, 3, 4), z)              # (c, y, x) order
    assert codec.rdo_record(lq, np.asfortranarray(z)) == rec
    with pytest.raises(ValueError, match='a \\(C, th, tw\\) array'):
        codec.rdo_record(lq, z[0])
    codec.check_rdo_record(0, 104, 2, 3, 4)
    codec.check_rdo_record(1 << 20, 104, 2, 3, 4)
    for off, nbytes, why in ((4, 104, 'not a multiple of 8'), (1, 104, 'not a multiple of 8'), (0, 100, 'expected 104'), (8, 108, 'expected 104')):
        with pytest.raises(ValueError, match=why):
            codec.check_rdo_record(off, nbytes, 2, 3, 4)
    assert codec.rdo_tile_lambdas(0.1, 3) == [0.1] * 3 and codec.rdo_tile_lambdas([0, 1, 2.5], 3) == [0.0, 1.0, 2.5]
    assert codec.rdo_tile_lambdas(np.float32(0.5), 2) == [0.5, 0.5] and codec.rdo_tile_lambdas(np.array([0.5, 1.0]), 2) == [0.5, 1.0]
    for bad, why in (([0.1, 0.2], '2 lambdas for 3 tiles'), ([0.1, -1, 0.2], '0 <= lambda < inf'), ('0.1', '0 <= lambda < inf')):
        with pytest.raises(ValueError, match=why):
            codec.rdo_tile_lambdas(bad, 3)


def _flags(command, **kw):
    base = dict(command=command, tile=None, checked=False, wavefront=False, salvage=False, channels=None, layers=None, progressive=False,
                front_layers=None, front_progressive=False, partial=False, recover=False, chunk=None, batch=8, depth=False, depth_block=None,
                rans=False, lanes=None, rdo=None, rdo_levels=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_option_sentences():
    for command in ('compress', 'compress-dir'):
        for kw in (dict(), dict(tile=128), dict(tile=128, rans=True), dict(tile=128, wavefront=True), dict(tile=128, depth=True),
                   dict(tile=128, progressive=True), dict(cap=3.0)):
            codec.check_option_args(_flags(command, rdo=0.05, **kw))
            codec.check_option_args(_flags(command, rdo=0.0, **kw))
    codec.check_option_args(_flags('compress', rdo=0.1, roi=['0,0,16,16'], background=1.0))
    codec.check_option_args(_flags('rd', rdo_levels='0,0.01,0.1'))
    codec.check_option_args(_flags('rd', tile=128, rans=True, rdo_levels='0.5'))
    for flags, why in ((_flags('transcode', rdo=0.1), '--rdo does not go with transcode: .* a file has no z'),
                       (_flags('transcode-dir', rdo=0.1), '--rdo does not go with transcode-dir'),
                       (_flags('decompress', rdo=0.1), '--rdo belongs to compress / compress-dir'),
                       (_flags('measure', rdo=0.1), '--rdo belongs to compress'),
                       (_flags('rd', rdo=0.1), '--rdo belongs to compress'),
                       (_flags('compress', rdo=0.1, max_bytes=1000), '--rdo does not go with --max-bytes: a search over lambda'),
                       (_flags('compress-dir', rdo=0.1, bpp=0.5), '--rdo does not go with --bpp'),
                       (_flags('compress', rdo=0.1, min_psnr=30.0), '--rdo does not go with --min-psnr'),
                       (_flags('compress', rdo=0.1, min_ms_ssim=0.9), '--rdo does not go with --min-ms-ssim'),
                       (_flags('compress', rdo=-0.1), '0 <= lambda < inf'),
                       (_flags('compress', rdo=float('inf')), '0 <= lambda < inf'),
                       (_flags('compress', rdo=float('nan')), '0 <= lambda < inf'),
                       (_flags('compress', rdo_levels='0,1'), '--rdo-levels belongs to rd'),
                       (_flags('rd', rdo_levels='0,1', levels=8), '--rdo-levels does not go with --levels or --roi'),
                       (_flags('rd', rdo_levels='0,1', roi=['0,0,16,16']), '--rdo-levels does not go with --levels or --roi'),
                       (_flags('rd', rdo_levels='0,x'), 'not a comma-separated list of numbers'),
                       (_flags('rd', rdo_levels='0,-1'), 'every lambda is a number with 0 <= lambda < inf'),
                       (_flags('rd', rdo_levels='inf'), 'every lambda is a number with 0 <= lambda < inf')):
        with pytest.raises(ValueError, match=why):
            codec.check_option_args(flags)
    assert codec.parse_rdo_levels_arg('0,0.01,1e-1') == [0.0, 0.01, 0.1]
    old = argparse.Namespace(command='compress', tile=128, checked=False, wavefront=True, salvage=False, channels=None)
    codec.check_option_args(old)                                              # a namespace without the keys reads as no option
    assert codec._rdo_note(0.05, 12, 3456) == ", lambda 0.05: 12 of 3456 symbols differ from the quantiser's"
    assert codec._rd_line(0.5, codec.Measure(100, 0.5, 1.0, 40.0, 0.99), 'lambda').startswith('lambda 0.5: 100 bytes')
    assert codec._rd_line(4, codec.Measure(100, 0.5, 1.0, 40.0, 0.99)).startswith('level 4: 100 bytes')


def test_header_macro_and_flag_layout():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'imgcomp_hip.h')).read()
    m = re.search(r'#define\s+IC_PC_DECODE_RDO\s+(0x[0-9a-fA-F]+)', text)
    assert m and int(m.group(1), 16) == _lib.PC_DECODE_RDO == 1 << 24
    # a bit of its own above the rANS field, clear of every other decoder flag
    others = _lib.PC_DECODE_PER_LAYER | _lib.PC_DECODE_RECOMPUTE | _lib.PC_DECODE_WAVEFRONT | _lib.PC_DECODE_DEPTH(0xff) | _lib.PC_DECODE_RANS(0xff)
    assert _lib.PC_DECODE_RDO & others == 0 and _lib.PC_DECODE_RDO > _lib.PC_DECODE_RANS(0xff)
    assert re.search(r'#define\s+IC_ABI_VERSION\s+2\b', text)
    assert not any('rdo' in name for name in _lib.PROTOTYPES)                # no new entry: a flag on an existing one
