"""The decode side of the codec, the parts that need no GPU: a word-level model of the device range-decoder step
(pc_dec_symbol_wave with pc_udiv, csrc/pc_decode.hip) against arithmetic_coding's ArithmeticDecoder, symbol for symbol -- on
streams the host encoder wrote (golden sequence, random tables up to the coder's limit, pending runs, frequency-1 symbols) and on
byte strings no encoder wrote.  Every comparison is an equality."""
import os

import numpy as np
import pytest

from imgcomp_cvpr_amd import arithmetic_coding as ac
from tests import codec_cases as cc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GARBAGE_SYMBOLS = 400            # symbols decoded from every byte string that no encoder wrote


def _cases():
    """[(name, symbols, freq rows)]: the sequences test_cpu_codec.py codes, and the constant tables the GPU tests construct"""
    out = []
    g = np.load(os.path.join(GOLD, 'arithcoding.npz'))
    out.append(('golden', g['symbols'].astype(np.int64), g['freqs'].astype(np.int64)))
    rs = np.random.RandomState(11)                               # drawn as test_model_random_tables draws them
    for L, conc in ((2, 1.0), (6, 0.05), (6, 5.0), (16, 0.3)):
        p = rs.dirichlet([conc] * L, size=1500)
        freqs = np.maximum((p * 1e9).astype(np.int64), 1)
        out.append(('dirichlet L={} conc={}'.format(L, conc), np.array([rs.choice(L, p=r) for r in p]), freqs))
        out.append(('dirichlet L={} conc={}, uniform symbols'.format(L, conc), rs.randint(L, size=len(p)), freqs))
    for i in range(20):                                          # free integer tables: totals up to the limit, frequency 1
        L = int(rs.randint(2, 17))
        n = 200
        totals = rs.randint(L, (1 << 30) + 3, size=n)
        cuts = np.sort(np.stack([rs.randint(1, t, size=L - 1) if t > L else np.arange(1, L) for t in totals]), axis=1)
        bounds = np.concatenate([np.zeros((n, 1), np.int64), cuts, totals[:, None]], axis=1)
        out.append(('integer tables {}'.format(i), rs.randint(L, size=n), np.maximum(np.diff(bounds, axis=1), 1)))
    logits, symbols = cc.pending_run_logits()
    out.append(('pending run', symbols, cc.softmax_tables(logits)))
    logits, symbols = cc.worst_case_logits(300)
    out.append(('worst case', symbols, cc.softmax_tables(logits)))
    # one row at every position, as constant_table_weights gives them
    rs = np.random.RandomState(12)
    for name, row in (('floor 1', [1] + [200000000] * 5), ('floor 1 at the top', [200000000] * 5 + [1]),
                      ('L=3 exact', [333333344] * 3), ('skewed L=6', cc.softmax_tables(np.array([[0, 1, 2, 3, 2, 1]]))[0].tolist()),
                      ('total = MAX_TOTAL', [1 << 30, 1, 1]), ('uniform L=16', [62500000] * 16),
                      ('3 live of 16', [333333344] * 3 + [1] * 13)):
        n = 400
        p = np.array(row, np.float64) / sum(row)
        symbols = np.where(rs.rand(n) < 0.7, rs.choice(len(row), size=n, p=p), rs.randint(len(row), size=n))
        out.append(('constant ' + name, symbols, [row] * n))
    return out


CASES = _cases()


def _both(data, rows, what):
    want = cc.host_decode(data, rows)
    got, status = cc.model_decode(data, rows)
    assert status == 0 and got == want, '{}: first difference at symbol {}'.format(
        what, next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want))))
    return want


def test_model_udiv_is_exact():
    """pc_udiv's precondition (n < 2^63, d < 2^34, n / d < 2^34: model_udiv asserts it on every call) holds for the three
    divisions of the decoder step -- ((code - low + 1) * total - 1) / r, cum_lo * r / total, cum_hi * r / total, with r in
    [2^30 + 1, 2^32] after renormalisation and total in [L, 2^30 + 2] -- and on them the corrected double quotient is //."""
    rs = np.random.RandomState(6)
    totals = [2, 3, 6, 16, 1000000000, 1000000005, (1 << 30) + 1, (1 << 30) + 2] + rs.randint(2, (1 << 30) + 3, size=600).tolist()
    ranges = [(1 << 30) + 1, (1 << 30) + 2, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 1, 1 << 32]
    checked, corrected = 0, [0]

    def check(n, d):
        assert n < (1 << 63) and d < (1 << 34) and n // d < (1 << 34)
        assert cc.model_udiv(n, d) == n // d, (n, d)
        raw = int(float(n) / float(d))
        assert abs(raw - n // d) <= 1                               # what one correction step can repair
        corrected[0] += raw != n // d
        return 1

    for total in totals:
        for r in ranges + rs.randint((1 << 30) + 1, (1 << 32) + 1, size=3).tolist():
            for cum in (0, 1, total - 1, total, int(rs.randint(0, total + 1))):
                checked += check(cum * r, total)
            for off in (0, r - 1, int(rs.randint(0, r))):           # off = code - low
                checked += check((off + 1) * total - 1, r)
    for _ in range(5000):                                           # free triples
        total, r = int(rs.randint(2, (1 << 30) + 3)), int(rs.randint((1 << 30) + 1, (1 << 32) + 1))
        checked += check(int(rs.randint(0, total + 1)) * r, total) + check((int(rs.randint(0, r)) + 1) * total - 1, r)
    print('pc_udiv model: {} quotients equal to //, {} of them only after the correction step'.format(checked, corrected[0]))
    assert corrected[0] > 0                                         # the operands reach the case the correction step is for


@pytest.mark.parametrize('name,symbols,rows', CASES, ids=[c[0] for c in CASES])
def test_model_decodes_what_the_host_encoder_wrote(name, symbols, rows):
    stream, _ = cc.host_encode(symbols, rows)
    if name == 'golden':
        assert stream == np.load(os.path.join(GOLD, 'arithcoding.npz'))['stream'].tobytes()
    assert _both(stream, rows, name) == [int(s) for s in symbols]


def test_model_pending_run_on_one_table():
    """straddle_symbols: a pending run longer than 64 on ONE table (what constant_table_weights can give the device decoders),
    decoded back by both.  (The peaked L = 8 table grows its run more slowly: it only has to grow.)"""
    for table, steps, floor in (([333333344] * 3, 60, 64), (cc.softmax_tables(np.array([[0, 1, 2, 3, 2, 1]]))[0].tolist(), 60, 64),
                                (cc.softmax_tables(np.array([[5, 0, 0, 0, 0, 0, 0, 0]]))[0].tolist(), 60, 0)):
        for prefix in ((), (0,), (0, 1, 0), (1, 0, 2, 0, 1, 1)):
            run, pending = cc.straddle_symbols(table, steps, prefix)
            print('table {}, {} leading symbols: pending {} after {} steps'.format(table, len(prefix), pending, steps))
            assert pending > floor, (table, prefix, pending)
            symbols = list(prefix) + run + np.random.RandomState(3).randint(len(table), size=30).tolist()
            stream, host_pending = cc.host_encode(symbols, [table] * len(symbols))
            assert host_pending >= pending                          # (the tail may add to the run before it releases it)
            assert _both(stream, [table] * len(symbols), 'straddle') == symbols
    assert cc.straddle_symbols([333333344] * 3, 60)[1] > 64         # fp32(1 / 3) * 1e9: the same row on every implementation
    # a cumulative boundary exactly at half the total: no symbol contains 2^31 at the first step
    for table in ([500000000] * 2, [166666672] * 6, [62500000] * 16):
        with pytest.raises(AssertionError, match='no symbol straddles'):
            cc.straddle_symbols(table, 60)


def test_model_and_host_agree_on_arbitrary_bytes():
    """bytes that no encoder wrote: the host decoder never refuses them (zeros past the end), the model returns its symbols"""
    compared = 0
    for i, (name, symbols, rows) in enumerate(CASES):
        valid, _ = cc.host_encode(symbols, rows)
        rows = rows[:GARBAGE_SYMBOLS]
        for what, data in cc.garbage_strings(valid, seed=100 + i):
            _both(data, rows, '{}, {}'.format(name, what))
            compared += 1
    print('{} byte strings x {} tables: model == host decoder'.format(compared // len(CASES), len(CASES)))
    assert compared >= 20 * len(CASES)


def test_model_status():
    at = [[1 << 30, 1, 1]] * 50
    over = [[1 << 30, 1, 1, 1]] * 50
    assert sum(at[0]) == ac.MAX_TOTAL and sum(over[0]) == ac.MAX_TOTAL + 1
    symbols = [0] * 20 + [1, 0, 2] * 10
    stream, _ = cc.host_encode(symbols, at)
    assert cc.model_decode(stream, at) == (symbols, 0)
    assert cc.model_decode(stream, over) == ([], 1)
    assert cc.model_decode(stream, at[:7] + over) == (symbols[:7], 1)      # the symbols before the refused table stand
    with pytest.raises(ValueError, match='total is too large'):
        cc.host_decode(stream, over)
    # fp32 softmax at resolution 2^30 gives exactly these rows: bias [40, 0, 0] is at the limit, [40, 0, 0, 0] one over
    assert cc.softmax_tables(np.array([[40, 0, 0]]), 2.0 ** 30)[0].tolist() == at[0]
    assert cc.softmax_tables(np.array([[40, 0, 0, 0]]), 2.0 ** 30)[0].tolist() == over[0]
    assert cc.model_encode([0], [1], [ac.MAX_TOTAL + 1])[1] == 1
