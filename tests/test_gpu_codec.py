"""-m gpu: the device range encoder (ic_pc_encode_f32) through the C ABI and through PredictionNetwork.encode_stream, and the codec
built on it (imgcomp_cvpr_amd.codec).  Every comparison is an equality: the device stream is the host coder's stream byte for byte,
and the host coder's is the reference coder's (tests/golden/arithcoding.npz, tests/test_cpu_host.py)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from tests import codec_cases as cc
from tests.util import dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5


def _device_tables(logits_t, resolution):
    """the tables the parent path codes with: ic_pc_logits_to_freqs_f32 on the same logits -> (n, L) int64 numpy"""
    from imgcomp_cvpr_amd import _lib
    n, L = logits_t.shape
    freqs = torch.empty((n, L), dtype=torch.int64, device=logits_t.device)
    _lib.check(_lib.lib.ic_pc_logits_to_freqs_f32(_lib.ptr(logits_t), n, L, resolution, _lib.ptr(freqs), None,
                                                  _lib.current_stream(logits_t.device)))
    return freqs.cpu().numpy()


def _raw_encode(cuda, logits, symbols, resolution=1e9, capacity=None, slack=64):
    """logits (N, count, L), symbols (N, count) numpy -> ([bytes], nbytes, status) from ONE launch.  The kernel is told `capacity`;
    the allocation behind it is `slack` bytes longer per volume and pre-filled with a guard value that must survive."""
    from imgcomp_cvpr_amd import _lib
    lg = dev(logits, cuda)
    sy = dev(symbols, cuda, torch.int64)
    N, count, L = lg.shape
    cap = int(_lib.lib.ic_pc_encode_capacity_bytes(count)) if capacity is None else int(capacity)
    # N volumes of `cap` bytes back to back, as the ABI lays them out, then the guard zone
    out = torch.full((N * cap + slack,), GUARD, dtype=torch.uint8, device=cuda)
    nbytes = torch.full((N,), -1, dtype=torch.int64, device=cuda)
    status = torch.full((N,), -1, dtype=torch.int32, device=cuda)
    _lib.check(_lib.lib.ic_pc_encode_f32(_lib.ptr(lg), _lib.ptr(sy), N, count, L, resolution, _lib.ptr(out), cap,
                                         _lib.ptr(nbytes), _lib.ptr(status), _lib.current_stream(cuda)), 'ic_pc_encode_f32')
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    nb, st = nbytes.tolist(), status.tolist()
    assert (o[N * cap:] == GUARD).all(), 'bytes behind the buffer were written'
    streams = []
    for n in range(N):
        assert 0 <= nb[n] <= cap
        vol = o[n * cap:(n + 1) * cap]
        assert (vol[nb[n]:] == GUARD).all(), 'bytes beyond nbytes were written'
        streams.append(vol[:nb[n]].tobytes())
    return streams, nb, st


def _host_stream(cuda, logits, symbols, resolution=1e9):
    """one volume: the parent's statement, encode_sequence(symbols[1:], freqs[1:]) over the device's own tables"""
    freqs = _device_tables(dev(logits, cuda), resolution)
    return cc.host_encode(symbols[1:], freqs[1:])


@pytest.fixture(scope='module')
def nets(cuda, configs, syn_weights):
    from imgcomp_cvpr_amd import autoencoder, probclass
    ae_cfg, pc_cfg = configs
    ae = autoencoder.get_network_cls(ae_cfg)(ae_cfg).load_weights(syn_weights, cuda)
    pc = probclass.get_network_cls(pc_cfg)(pc_cfg, num_centers=ae_cfg.num_centers).load_weights(syn_weights, cuda)
    pred = probclass.PredictionNetwork(pc, pc_cfg, ae.get_centers_variable())
    return ae, pc, pred


def _parent_file(pred, sym, tmp_path):
    """bit_counter._encode's file for a (C,h,w) symbol volume -> (bytes, first_sym, theoretical bits)"""
    from imgcomp_cvpr_amd import bit_counter
    fd, path = tempfile.mkstemp(dir=str(tmp_path))
    nbits, first, theory = bit_counter._encode(fd, pred.pad_symbols_volume(sym), sym, pred)
    data = open(path, 'rb').read()
    assert nbits == 8 * len(data)
    return data, first, theory


def _kodak_symbols(cuda, ae):
    from imgcomp_cvpr_amd import weights as W
    x = dev(W.synthetic_image((1, 3, 512, 768), 'natural', seed=4), cuda)      # the volume of test_cfg4_real_bpp_full_kodak_volume
    return ae.encode(x, False).symbols[0].cpu().numpy()


@pytest.mark.parametrize('case', ['random120', 'enc64x96', 'kodak'])
def test_encode_stream_equals_parent_file(cuda, nets, tmp_path, case):
    from imgcomp_cvpr_amd import weights as W
    ae, pc, pred = nets
    if case == 'random120':
        sym = np.random.RandomState(7).randint(0, 6, size=(3, 5, 8)).astype(np.int64)
    elif case == 'enc64x96':
        sym = ae.encode(dev(W.synthetic_image((1, 3, 64, 96), 'natural', seed=2), cuda), False).symbols[0].cpu().numpy()
        assert sym.size == 3072
    else:
        sym = _kodak_symbols(cuda, ae)
        assert sym.size == 196608
    want, first, _ = _parent_file(pred, sym, tmp_path)
    got, got_first = pred.encode_stream(sym)
    print('{}: {} symbols, {} bytes from the device, {} from the host coder'.format(case, sym.size, len(got), len(want)))
    assert got_first == first == int(sym.reshape(-1)[0])
    assert got == want, 'device stream differs from bit_counter._encode\'s file'
    # the C ABI on the logits of the public path, with the guard bytes checked
    q = ae.get_centers_variable()[torch.as_tensor(pred.pad_symbols_volume(sym)).to(cuda).long()][None].contiguous()
    logits = pc.logits(q, is_training=False).reshape(1, sym.size, pc.L).cpu().numpy()
    streams, nb, st = _raw_encode(cuda, logits, sym.reshape(1, -1))
    assert st == [0] and streams[0] == want
    # ... and back: the device decoder returns the symbols from the device encoder's stream
    if case != 'kodak':                                  # the full volume's decode is test_bit_count_device_encode's
        assert np.array_equal(pred.decode_stream(got, sym.shape, got_first), sym)


def test_count_one(cuda, nets):
    _, _, pred = nets
    streams, nb, st = _raw_encode(cuda, np.zeros((2, 1, 6), np.float32), np.array([[3], [0]]))
    assert streams == [b'\x80', b'\x80'] and nb == [1, 1] and st == [0, 0]
    assert pred.encode_stream(np.array([[[4]]])) == (b'\x80', 4)
    assert pred.decode_stream(b'\x80', (1, 1, 1), 4).tolist() == [[[4]]]


def test_pending_run_longer_than_reservoir(cuda):
    logits, symbols = cc.pending_run_logits()
    logits = np.concatenate([np.zeros((1, cc.PENDING_L), np.float32), logits])           # position 0 is not coded
    symbols = np.concatenate([[0], symbols])
    want, pending = _host_stream(cuda, logits, symbols)
    print('pending run: the host coder\'s _pending reached {} on the device\'s tables'.format(pending))
    assert pending > 64, pending
    streams, _, st = _raw_encode(cuda, logits[None], symbols[None])
    assert st == [0] and streams[0] == want
    for lead in (1, 3, 6):                                                    # other fill levels of the reservoir at the release
        l2 = np.concatenate([np.zeros((1 + lead, cc.PENDING_L), np.float32), logits[1:61], logits[-10:]])
        s2 = np.concatenate([np.zeros(1 + lead, np.int64), symbols[1:61], symbols[-10:]])
        want2, p2 = _host_stream(cuda, l2, s2)
        assert p2 > 64
        assert _raw_encode(cuda, l2[None], s2[None])[0][0] == want2


def test_worst_case_cost(cuda):
    logits, symbols = cc.worst_case_logits(400)
    want, _ = _host_stream(cuda, logits, symbols)
    streams, nb, st = _raw_encode(cuda, logits[None], symbols[None])
    print('worst case through softmax: {:.3f} bits per symbol'.format(8.0 * nb[0] / 399))
    assert st == [0] and streams[0] == want
    assert 29.0 <= 8.0 * nb[0] / 399 <= 32.0


@pytest.mark.parametrize('L', [2, 6, 11, 16])
def test_other_numbers_of_centres(cuda, L):
    rs = np.random.RandomState(L)
    n = 1000
    logits = (rs.randn(n, L) * rs.choice([0.5, 3.0, 12.0], size=(n, 1))).astype(np.float32)
    symbols = rs.randint(0, L, size=n)
    want, _ = _host_stream(cuda, logits, symbols)
    streams, _, st = _raw_encode(cuda, logits[None], symbols[None])
    assert st == [0] and streams[0] == want


def test_three_volumes_in_one_launch(cuda, nets):
    ae, pc, pred = nets
    rs = np.random.RandomState(21)
    n, L = 700, 6
    logits = (rs.randn(3, n, L) * np.array([1.0, 4.0, 10.0])[:, None, None]).astype(np.float32)
    symbols = rs.randint(0, L, size=(3, n))
    singles = [_raw_encode(cuda, logits[i:i + 1], symbols[i:i + 1])[0][0] for i in range(3)]
    streams, nb, st = _raw_encode(cuda, logits, symbols)
    assert st == [0, 0, 0] and streams == singles and len(set(singles)) == 3
    assert singles == [_host_stream(cuda, logits[i], symbols[i])[0] for i in range(3)]
    # the public batched form
    sym = rs.randint(0, 6, size=(3, 4, 6, 7))
    batch = pred.encode_stream(sym)
    assert batch == [pred.encode_stream(sym[i]) for i in range(3)]
    for (stream, first), s in zip(batch, sym):
        assert np.array_equal(pred.decode_stream(stream, s.shape, first), s)


def test_capacity_too_small_sets_status_2(cuda):
    rs = np.random.RandomState(33)
    n, L = 500, 6
    logits = (rs.randn(2, n, L) * 3).astype(np.float32)
    symbols = rs.randint(0, L, size=(2, n))
    full, nb, st = _raw_encode(cuda, logits, symbols)
    assert st == [0, 0]
    # exactly enough is enough; one byte short is status 2 and the byte behind the buffer keeps its guard value (_raw_encode
    # asserts that for every byte at or beyond the capacity it passed: they lie inside a larger allocation)
    exact, nb2, st2 = _raw_encode(cuda, logits[:1], symbols[:1], capacity=nb[0])
    assert st2 == [0] and exact[0] == full[0]
    cut, nb3, st3 = _raw_encode(cuda, logits[:1], symbols[:1], capacity=nb[0] - 1)
    assert st3 == [2] and nb3[0] <= nb[0] - 1 and full[0].startswith(cut[0])
    cap = min(nb) - 1
    cut, nb4, st4 = _raw_encode(cuda, logits, symbols, capacity=cap)                  # a volume must not spill into its neighbour
    assert st4 == [2, 2] and all(full[i].startswith(cut[i]) for i in range(2))
    assert _raw_encode(cuda, logits[:1], symbols[:1], capacity=0)[1:] == ([0], [2])
    # the long pending run against a small buffer: its whole-byte store is bounded like every other
    lg, sy = cc.pending_run_logits()
    lg, sy = np.concatenate([np.zeros((1, cc.PENDING_L), np.float32), lg]), np.concatenate([[0], sy])
    whole = _raw_encode(cuda, lg[None], sy[None])[0][0]
    for cap in (1, 8, 20, len(whole) - 1):
        cut, _, st5 = _raw_encode(cuda, lg[None], sy[None], capacity=cap)
        assert st5 == [2] and whole.startswith(cut[0])


def test_table_total_too_large_sets_status_1(cuda, nets):
    _, _, pred = nets
    rs = np.random.RandomState(4)
    logits = rs.randn(1, 50, 6).astype(np.float32)
    symbols = rs.randint(0, 6, size=(1, 50))
    assert _raw_encode(cuda, logits, symbols, resolution=1e9)[2] == [0]
    assert _raw_encode(cuda, logits, symbols, resolution=2e9)[2] == [1]         # totals ~ 2e9 > 2^30 + 2
    bad = symbols.copy()
    bad[0, 17] = 6
    assert _raw_encode(cuda, logits, bad)[2] == [3]                             # a symbol outside [0, L) is refused, not coded
    from imgcomp_cvpr_amd import probclass
    hot = probclass.PredictionNetwork(pred.pc, pred.config, pred.centers, freqs_resolution=2e9)
    with pytest.raises(ValueError, match='total is too large'):
        hot.encode_stream(rs.randint(0, 6, size=(2, 4, 4)))


def test_bit_count_device_encode(cuda, nets):
    """encode_decode_to_file_ctx with the device encoder: the same count as with the host coder, all three run-time checks kept
    (|coded - theoretical| < 50 bits, file size, decoded symbols) -- on the full Kodak volume."""
    from imgcomp_cvpr_amd import bit_counter, probclass
    ae, pc, pred = nets
    sym = _kodak_symbols(cuda, ae)
    host_bits = bit_counter.encode_decode_to_file_ctx(sym, pred, syms_format='CHW')
    dev_bits = bit_counter.encode_decode_to_file_ctx(sym, pred, syms_format='CHW', device_encode=True)
    assert dev_bits == host_bits
    checker = probclass.ProbclassNetworkTesting(pc, ae)
    small = sym[:4, :10, :12]
    assert (bit_counter.encode_decode_to_file_ctx(small, pred, syms_format='CHW', device_encode=True,
                                                  theoretical_bit_cost=checker.get_total_bit_cost)
            == bit_counter.encode_decode_to_file_ctx(small, pred, syms_format='CHW'))
    with pytest.raises(AssertionError, match='Theoretical'):
        bit_counter.encode_decode_to_file_ctx(small, pred, syms_format='CHW', device_encode=True, theoretical_bit_cost=1e6)


@pytest.mark.parametrize('shape', [(512, 768), (61, 93)])
def test_codec_round_trip(cuda, configs, syn_weights, shape):
    from imgcomp_cvpr_amd import bit_counter, codec, val, weights as W
    ae_cfg, pc_cfg = configs
    H, W_ = shape
    img = np.ascontiguousarray(W.synthetic_image((1, 3, H, W_), 'natural', seed=9)[0].transpose(1, 2, 0))
    c = codec.Codec(ae_cfg, pc_cfg, syn_weights, cuda)
    data = c.compress(img)
    out = c.decompress(data)
    assert out.shape == img.shape and out.dtype == np.uint8
    # against the pieces, run by hand as val.py runs them
    padded, undo = val.add_padding(img, c.factor)
    x = torch.as_tensor(np.ascontiguousarray(padded.transpose(2, 0, 1))[None]).to(cuda).float()
    enc = c.ae.encode(x, is_training=False)
    sym, head = c.decode_symbols(data)
    assert np.array_equal(sym, enc.symbols[0].cpu().numpy())
    assert (head.H, head.W, head.C, head.h, head.w, head.L) == (H, W_, 32, padded.shape[0] // 8, padded.shape[1] // 8, 6)
    x_out = c.ae.decode(enc.qhard, is_training=False).to(torch.uint8)[0].cpu().numpy().transpose(1, 2, 0)
    assert np.array_equal(out, undo(x_out)), 'pixels differ from ae.decode(enc.qhard)'
    nbits = bit_counter.encode_decode_to_file_ctx(enc.symbols[0].cpu().numpy(), c.pred, syms_format='CHW')
    assert 8 * len(head.payload) == nbits
    # the host encoder writes the same file
    c.device_encode = False
    assert c.compress(img) == data
    # a damaged or foreign file is refused before anything is decoded
    bad = bytearray(data)
    bad[len(bad) // 2] ^= 1
    with pytest.raises(ValueError, match='CRC'):
        c.decompress(bytes(bad))
    other = codec.Codec(ae_cfg, pc_cfg, W.synthetic_weights(ae_cfg, pc_cfg, seed=77), cuda)
    with pytest.raises(ValueError, match='fingerprint'):
        other.decompress(data)


def _cli(args, timeout):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    return subprocess.run([sys.executable, '-m', 'imgcomp_cvpr_amd.codec'] + args, cwd=ROOT, env=env, timeout=timeout,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


def test_cli_in_fresh_processes(cuda, configs, syn_weights, tmp_path):
    from PIL import Image
    from imgcomp_cvpr_amd import codec, weights as W
    ae_cfg, pc_cfg = configs
    img = np.ascontiguousarray(W.synthetic_image((1, 3, 77, 120), 'natural', seed=12)[0].transpose(1, 2, 0))
    src, icf, png = str(tmp_path / 'in.png'), str(tmp_path / 'out.icf'), str(tmp_path / 'back.png')
    Image.fromarray(img).save(src)
    r = _cli(['compress', src, icf], 600)
    assert r.returncode == 0, r.stderr
    print(r.stdout.strip())
    assert 'bpp' in r.stdout
    r = _cli(['decompress', icf, png], 600)
    assert r.returncode == 0, r.stderr
    c = codec.Codec(ae_cfg, pc_cfg, syn_weights, cuda)
    data = open(icf, 'rb').read()
    assert data == c.compress(img)
    assert np.array_equal(np.asarray(Image.open(png)), c.decompress(data))
    # written with one seed of synthetic weights, refused under another
    r = _cli(['decompress', icf, str(tmp_path / 'no.png'), '--synthetic_seed', '4321'], 600)
    assert r.returncode != 0 and 'fingerprint' in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(str(tmp_path / 'no.png'))
