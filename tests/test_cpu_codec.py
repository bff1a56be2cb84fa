"""Codec, the parts that need no GPU: the container, the capacity bound, and a word-level model of the device range encoder
(clz renormalisation, 64-bit reservoir, pending runs longer than the reservoir) against arithmetic_coding's coder, byte for byte."""
import os
import struct
import zlib

import numpy as np
import pytest

from tests import codec_cases as cc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _fields(payload=b'\x12\x34\x56\x80'):
    return dict(ae_name='cvpr/low', pc_name='cvpr/res_shallow', H=61, W=93, C=32, h=8, w=12, L=6, first_sym=3,
                resolution=1e9, fingerprint=0xdeadbeef, payload=payload)


def test_container_round_trip():
    from imgcomp_cvpr_amd import codec
    f = _fields()
    data = codec.build_container(**f)
    c = codec.parse_container(data)
    assert c.version == codec.FORMAT_VERSION
    for k, v in f.items():
        assert getattr(c, k) == v, k
    assert data[:4] == b'ICVF' and struct.unpack('<I', data[-4:])[0] == zlib.crc32(data[:-4])
    # an empty payload and empty names are legal containers
    e = codec.parse_container(codec.build_container(**dict(f, payload=b'', ae_name='', pc_name='')))
    assert e.payload == b'' and e.ae_name == ''


def test_container_refuses_damage():
    from imgcomp_cvpr_amd import codec
    data = codec.build_container(**_fields(payload=bytes(range(200))))
    head = len(data) - 4 - 200
    for pos, word in ((0, 'magic'), (4, 'version'), (10, 'CRC'), (head - 3, 'CRC'), (head + 17, 'CRC'), (len(data) - 2, 'CRC')):
        bad = bytearray(data)
        bad[pos] ^= 0x40
        with pytest.raises(ValueError, match=word):
            codec.parse_container(bytes(bad))
    for n in (0, 3, 20, head - 1, head, head + 100, len(data) - 1):
        with pytest.raises(ValueError, match='truncated|CRC'):
            codec.parse_container(data[:n])
    with pytest.raises(ValueError, match='truncated|CRC'):
        codec.parse_container(data + b'\x00')
    # lengths that lie, under a CRC that is right: still refused, by the bounds of the bytes that are there
    f = _fields()
    good = codec.build_container(**f)
    body = bytearray(good[:-4])
    off = len(body) - len(f['payload']) - 8
    body[off:off + 8] = struct.pack('<Q', 1 << 40)
    with pytest.raises(ValueError, match='payload length'):
        codec.parse_container(bytes(body) + struct.pack('<I', zlib.crc32(bytes(body))))
    body = bytearray(good[:-4])
    body[6:8] = struct.pack('<H', 60000)
    with pytest.raises(ValueError, match='truncated'):
        codec.parse_container(bytes(body) + struct.pack('<I', zlib.crc32(bytes(body))))


def test_fingerprint_and_model_checks(configs, syn_weights):
    """check_container needs no device: a Codec shell with the model's numbers."""
    from imgcomp_cvpr_amd import codec, weights as W
    ae_cfg, pc_cfg = configs

    def fp(wts):
        return codec.model_fingerprint(wts['autoencoder/encoder/centers'], {k: v for k, v in wts.items() if k.startswith('probclass3d/')})

    a, b = fp(syn_weights), fp(W.synthetic_weights(ae_cfg, pc_cfg, seed=99))
    assert a == fp(W.synthetic_weights(ae_cfg, pc_cfg)) and a != b
    assert codec.config_name(ae_cfg) == 'cvpr/low' and codec.config_name(pc_cfg) == 'cvpr/res_shallow'

    class _Pred(object):
        freqs_resolution = 1e9
    shell = codec.Codec.__new__(codec.Codec)
    shell.ae_name, shell.pc_name, shell.fingerprint, shell.C, shell.L, shell.factor, shell.pred = 'cvpr/low', 'cvpr/res_shallow', a, 32, 6, 8, _Pred()
    good = dict(_fields(), fingerprint=a)
    shell.check_container(codec.parse_container(codec.build_container(**good)))
    for change, word in ((dict(fingerprint=b), 'fingerprint'), (dict(ae_name='cvpr/hi'), 'config'), (dict(pc_name='x'), 'config'),
                         (dict(C=16), 'C = 16'), (dict(L=12), 'L = 12'), (dict(h=9), 'symbol volume'), (dict(w=1 << 20), 'symbol volume'),
                         (dict(H=0), 'image size'), (dict(first_sym=6), 'first symbol'), (dict(resolution=2e9), 'resolution')):
        with pytest.raises(ValueError, match=word):
            shell.check_container(codec.parse_container(codec.build_container(**dict(good, **change))))
    # a short payload with a large volume is legitimate (a confident table codes far below a bit per symbol): only the header's
    # own image size bounds the volume
    shell.check_container(codec.parse_container(codec.build_container(**dict(good, H=4096, W=4096, h=512, w=512, payload=b'\x80'))))


def test_encode_capacity_bytes():
    from imgcomp_cvpr_amd import _lib
    cap = _lib.lib.ic_pc_encode_capacity_bytes
    assert cap(1) == 20 and cap(120) == 496 and cap(196608) == 4 * 196608 + 16
    assert cap(0) == 0 and cap(-5) == 0
    assert cap(1 << 40) == 4 * (1 << 40) + 16                   # 64-bit arithmetic


def _assert_model_equals_host(symbols, freqs, what):
    host, host_pending = cc.host_encode(symbols, freqs)
    got, status, model_pending = cc.model_encode(*cc.triples(symbols, freqs))
    assert status == 0 and got == host, '{}: the model wrote {} bytes, the host coder {}'.format(what, len(got), len(host))
    assert model_pending == host_pending
    return host, host_pending


def test_model_reciprocal_division_is_exact():
    rs = np.random.RandomState(5)
    tot = [1, 2, 3, 6, 1000000005, (1 << 30) + 1, (1 << 30) + 2] + rs.randint(1, (1 << 30) + 3, size=3000).tolist()
    for d in tot:
        for r in (1 << 32, (1 << 32) - 1, (1 << 30) + 2, int(rs.randint(1 << 30, 1 << 32))):
            for c in (0, 1, d - 1, d, int(rs.randint(0, d + 1))):
                assert cc.model_div(c * r, d) == c * r // d


def test_model_golden_sequence():
    g = np.load(os.path.join(GOLD, 'arithcoding.npz'))
    host, _ = _assert_model_equals_host(g['symbols'], g['freqs'], 'golden')
    assert host == g['stream'].tobytes()                           # ... which is the reference coder's stream
    assert cc.model_encode([], [], []) == (b'\x80', 0, 0)          # count == 1: nothing coded, the finishing bit alone


def test_model_random_tables():
    rs = np.random.RandomState(11)
    for L, conc in ((2, 1.0), (6, 0.05), (6, 5.0), (16, 0.3)):
        p = rs.dirichlet([conc] * L, size=1500)
        freqs = np.maximum((p * 1e9).astype(np.int64), 1)
        syms = np.array([rs.choice(L, p=r) for r in p])
        _assert_model_equals_host(syms, freqs, 'dirichlet L={}'.format(L))
        _assert_model_equals_host(rs.randint(L, size=len(p)), freqs, 'uniform symbols L={}'.format(L))   # improbable symbols too
    # free integer tables: every total up to the coder's limit, symbols of frequency 1
    for _ in range(20):
        L = int(rs.randint(2, 17))
        n = 200
        totals = rs.randint(L, (1 << 30) + 3, size=n)
        cuts = np.sort(np.stack([rs.randint(1, t, size=L - 1) if t > L else np.arange(1, L) for t in totals]), axis=1)
        bounds = np.concatenate([np.zeros((n, 1), np.int64), cuts, totals[:, None]], axis=1)
        freqs = np.maximum(np.diff(bounds, axis=1), 1)
        _assert_model_equals_host(rs.randint(L, size=n), freqs, 'integer tables')


def test_model_pending_run_longer_than_reservoir():
    logits, symbols = cc.pending_run_logits()
    freqs = cc.softmax_tables(logits)
    host, host_pending = _assert_model_equals_host(symbols, freqs, 'pending run')
    assert host_pending > 64, host_pending                          # the run really outgrew the 64-bit reservoir ...
    assert b'\xff' * 20 in host or b'\x00' * 20 in host             # ... and left as whole bytes
    # the run released at every reservoir fill level: 0..7 bits already waiting
    for lead in range(8):
        pre = np.zeros((lead, cc.PENDING_L), np.float32)
        l2 = np.concatenate([pre, logits[:60], logits[-10:]])
        s2 = np.concatenate([np.zeros(lead, np.int64), symbols[:60], symbols[-10:]])
        assert _assert_model_equals_host(s2, cc.softmax_tables(l2), 'pending run after {} symbols'.format(lead))[1] > 64


def test_model_worst_case_and_capacity():
    from imgcomp_cvpr_amd import _lib
    n = 300
    freqs = np.tile(np.array([[1, (1 << 30) + 1]], np.int64), (n, 1))       # total 2^30 + 2, the symbol of frequency 1
    host, _ = _assert_model_equals_host(np.zeros(n, np.int64), freqs, 'worst case')
    top, _ = _assert_model_equals_host(np.ones(n, np.int64), freqs[:, ::-1], 'worst case, frequency 1 at the top of the table')
    # A step commits n + m bits with 2^(n + m) <= (range after renormalisation) / (width of the symbol) <= 2^32 / 1: never more than
    # 4 bytes per symbol, which is what ic_pc_encode_capacity_bytes reserves.  Measured here: 30.0 bits per symbol with the symbol at
    # the top of the table, 30.5 at the bottom (widths 3, 2, 3, 2, ... of the full range: 30 and 31 bits in turn).
    for stream in (host, top):
        assert 30.0 <= 8.0 * len(stream) / n <= 32.0, 8.0 * len(stream) / n
        assert len(stream) <= 4 * n + 1 <= _lib.lib.ic_pc_encode_capacity_bytes(n + 1)
    logits, symbols = cc.worst_case_logits(n)
    sm = cc.softmax_tables(logits)
    assert sm[0].tolist() == [1, 1000000000]
    host2, _ = _assert_model_equals_host(symbols, sm, 'worst case through softmax')
    assert 29.0 <= 8.0 * len(host2) / n <= 32.0, 8.0 * len(host2) / n
    # capacity one byte short: status 2, nothing beyond the capacity; a total above the limit: status 1
    tr = cc.triples(np.zeros(n, np.int64), freqs)
    got, status, _ = cc.model_encode(*tr, capacity=len(host) - 1)
    assert status == 2 and len(got) <= len(host) - 1 and host.startswith(got)
    assert cc.model_encode(*tr, capacity=len(host))[:2] == (host, 0)
    assert cc.model_encode([0], [1], [(1 << 30) + 3])[1] == 1
