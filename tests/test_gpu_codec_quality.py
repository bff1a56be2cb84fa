"""-m gpu: the quality axis of the codec -- Codec.measure, rd_curve, compress_to_quality, transcode_to_quality and their commands.
Every comparison between two ways of getting a number is an equality of doubles: a row of the table against measure of the real file,
the search's result against the table and against real compress / measure calls.  The only tolerances are those of the device metrics
against the host's NumPy code (1e-4 dB, 1e-6, as test_device_metrics_match_numpy holds them).  No figure is pinned: the targets are
derived from the curve of the same run, which under the synthetic weights is narrow and NOT monotone in the level."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = {'untiled': {}, 'tile64': dict(tile=(8, 8)), 'fronts': dict(tile=(8, 8), front_layers='default')}
SIZES = {'64x96': (64, 96, 9), '40x56': (40, 56, 2)}
ROIS = [(10, 20, 30, 16)]


def _picture(h, w, seed):
    from imgcomp_cvpr_amd import weights as W_
    return np.ascontiguousarray(np.transpose(W_.synthetic_image((1, 3, h, w), 'natural', seed=seed)[0], (1, 2, 0)))


def _set(c, tile=None, layers=None, front_layers=None):
    c.tile, c.layers, c.front_layers, c.checked, c.order = tile, layers, front_layers, False, 'raster'
    return c


@pytest.fixture(scope='module')
def cdc(cuda, configs, syn_weights):
    from imgcomp_cvpr_amd import codec
    c = codec.Codec(configs[0], configs[1], syn_weights, cuda)
    assert (c.C, c.L) == (32, 6)
    yield c
    _set(c)


@pytest.fixture(scope='module')
def pics():
    return {name: _picture(*hws) for name, hws in SIZES.items()}


@pytest.fixture(scope='module')
def img(pics):
    return pics['64x96']


def _device_values(cuda, a_hwc, b_hwc):
    """metrics.val_metrics_device on two uploaded HWC uint8 pictures -> the six doubles"""
    from imgcomp_cvpr_amd import metrics
    up = lambda p: torch.as_tensor(np.ascontiguousarray(np.transpose(p, (2, 0, 1)))[None]).to(cuda)
    scales, mse = metrics.val_metrics_device(up(a_hwc), up(b_hwc))
    return scales.tolist() + [float(mse)]


# ---- measure ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('size', sorted(SIZES))
@pytest.mark.parametrize('fmt', sorted(FORMATS))
def test_measure(cuda, cdc, pics, fmt, size):
    from imgcomp_cvpr_amd import codec, metrics
    c, pic = _set(cdc, **FORMATS[fmt]), pics[size]
    H, W = pic.shape[:2]
    data = c.compress(pic)
    dec = c.decompress(data)
    m = c.measure(pic, data)
    six = _device_values(cuda, pic, dec)
    assert m == codec.measure_from_values(six, len(data), H * W)             # bit for bit: mse, and psnr / ms_ssim as functions of the six
    assert m.mse == six[5] and m.bytes == len(data) and m.bpp == 8.0 * len(data) / (H * W)
    assert m.psnr == metrics.psnr_from_mse(six[5]) and m.ms_ssim == metrics.msssim_from_scale_values(six[:5])
    nchw = lambda p: np.transpose(p, (2, 0, 1))[None]
    host_psnr, host_msssim = float(metrics.psnr_uint8(pic, dec)), float(metrics.msssim_nchw_uint8(nchw(pic), nchw(dec)))
    print('{} {}: {} | host psnr {} ms-ssim {}'.format(fmt, size, m, host_psnr, host_msssim))
    assert abs(m.psnr - host_psnr) <= 1e-4 and abs(m.ms_ssim - host_msssim) <= 1e-6
    # a preview is measured as the preview
    m4 = c.measure(pic, data, channels=4)
    assert m4 == codec.measure_from_values(_device_values(cuda, pic, c.decompress(data, channels=4)), len(data), H * W)
    assert m4.mse != m.mse
    # a rectangle: the metrics of the two crops, the bytes the file's; clipped as a region of interest is
    for rect, (x0, y0, x1, y1) in (((10, 20, 30, 16), (10, 20, 40, 36)), ((-5, -5, 30, 40), (0, 0, 25, 35)), ((W - 20, H - 17, 99, 99), (W - 20, H - 17, W, H))):
        mr = c.measure(pic, data, rect=rect)
        assert mr == codec.measure_from_values(_device_values(cuda, pic[y0:y1, x0:x1], dec[y0:y1, x0:x1]), len(data), H * W), rect
        assert mr.mse != m.mse and (mr.bytes, mr.bpp) == (m.bytes, m.bpp)
    assert c.measure(pic, data, rect=(0, 0, W, H)) == m
    _set(cdc)


def test_measure_refusals(cdc, img):
    c = _set(cdc, tile=(8, 8))
    data = c.compress(img)
    damaged = bytearray(data)
    damaged[len(data) // 2] ^= 0x10
    for bad in (bytes(damaged), data[:-7], b'', data[:4] + b'\x03\x00' + data[6:]):
        with pytest.raises(ValueError) as want:
            c.decompress(bad)
        with pytest.raises(ValueError) as got:
            c.measure(img, bad)
        assert str(got.value) == str(want.value)
    with pytest.raises(ValueError) as e:
        c.measure(img[:-3], data)
    assert '61 x 96' in str(e.value) and '64 x 96' in str(e.value)
    with pytest.raises(ValueError, match='at least 16'):
        c.measure(img, data, rect=(0, 0, 15, 40))
    with pytest.raises(ValueError, match='does not intersect'):
        c.measure(img, data, rect=(200, 0, 20, 20))
    with pytest.raises(ValueError, match='channels'):
        c.measure(img, data, channels=0)
    _set(cdc)


# ---- rd_curve -----------------------------------------------------------------------------------------------------------------------

def _rows_are_measures(c, pic, rows, rois=None):
    for level, m in rows:
        data = c.compress(pic, rois=rois, background=level) if rois else c.compress(pic, cap=level)
        assert m == c.measure(pic, data), (level, m)


@pytest.mark.parametrize('fmt', sorted(FORMATS))
def test_rd_curve(cdc, pics, fmt):
    from imgcomp_cvpr_amd import codec
    c, pic = _set(cdc, **FORMATS[fmt]), pics['64x96']
    rows = c.rd_curve(pic)
    assert [lv for lv, _ in rows] == codec.rd_levels(c.C) and len(rows) == 17
    _rows_are_measures(c, pic, rows)
    psnrs = sorted(set(m.psnr for _, m in rows))
    print('{}: {} distinct PSNR values of 17: {} .. {}'.format(fmt, len(psnrs), psnrs[0], psnrs[-1]))
    assert len(psnrs) >= 3, 'fixture too flat: the 17 levels show {} distinct PSNR values'.format(len(psnrs))
    assert rows[-1][1] == c.measure(pic, c.compress(pic))                    # level C is the file without a cap
    assert len(set(m.bytes for _, m in rows)) >= 3                           # the bytes are those of real files
    _set(cdc)


@pytest.mark.parametrize('fmt,size', [('untiled', '40x56'), ('tile64', '64x96'), ('fronts', '40x56')])
def test_rd_curve_explicit_levels_and_rois(cdc, pics, fmt, size):
    c, pic = _set(cdc, **FORMATS[fmt]), pics[size]
    levels = [0, 2.5, 7, 31.875, float('inf')]
    rows = c.rd_curve(pic, levels=levels)
    assert [lv for lv, _ in rows] == levels
    _rows_are_measures(c, pic, rows)
    with_rois = c.rd_curve(pic, levels=levels[:3], rois=ROIS)
    _rows_are_measures(c, pic, with_rois, rois=ROIS)
    assert [m for _, m in with_rois] != [m for _, m in rows[:3]]
    for bad in ([], [2, 1], [-1]):
        with pytest.raises(ValueError):
            c.rd_curve(pic, levels=bad)
    _set(cdc)


def test_rd_curve_under_forced_f2x2(cuda, configs, syn_weights, img):
    """a Codec whose 3 x 3 layers may not run F(4x4): the table is still that Codec's own measure of its own files"""
    from imgcomp_cvpr_amd import codec, _lib
    c2 = codec.Codec(configs[0], configs[1], syn_weights, cuda, plan_flags=_lib.CONV3_NO_WINO4)
    rows = c2.rd_curve(img, levels=[0, 3.25, 16, 32])
    _rows_are_measures(c2, img, rows)


# ---- compress_to_quality --------------------------------------------------------------------------------------------------------------

PROBE_BOUND = 1 + 2 + 8


@pytest.fixture(scope='module')
def table(cdc, img):
    """the 257-level curve of the 64 x 96 picture, untiled: computed once"""
    from imgcomp_cvpr_amd import codec
    rows = _set(cdc).rd_curve(img, levels=codec.rd_levels(cdc.C, 256))
    assert [np.float32(lv) for lv, _ in rows] == list(codec.cap_levels(cdc.C))
    return rows


@pytest.mark.parametrize('metric', ['psnr', 'ms_ssim'])
def test_compress_to_quality(cdc, img, table, metric):
    from imgcomp_cvpr_amd import codec
    c = _set(cdc)
    curve = [getattr(m, metric) for _, m in table]
    if metric == 'ms_ssim':
        assert all(math.isfinite(v) for v in curve), 'the MS-SSIM curve has a nan: no target can be derived from it'
    low, top = min(curve), curve[256]
    print('{}: level 0 {}, uncapped {}, min {} max {}, {} distinct'.format(metric, curve[0], top, low, max(curve), len(set(curve))))
    for target in (top, 0.5 * (curve[0] + top), low - 1.0 if metric == 'psnr' else 0.5 * low):
        data, level, m, probes = c.compress_to_quality(img, **{metric: target})
        k = [lv for lv, _ in table].index(level)
        print('  target {} -> level {} after {} probes: {}'.format(target, level, probes, m))
        assert m == table[k][1]
        assert getattr(m, metric) >= target and (k == 0 or not curve[k - 1] >= target)
        assert data == c.compress(img, cap=level) and m == c.measure(img, data)
        assert 1 <= probes <= PROBE_BOUND
        if target < low:
            assert (level, probes) == (0.0, 1)
    above = max(curve) + (1.0 if metric == 'psnr' else 0.5 * (1.0 - max(curve)))
    with pytest.raises(ValueError) as e:
        c.compress_to_quality(img, **{metric: above})
    assert 'without a cap reaches {:g}'.format(top) in str(e.value), str(e.value)
    for kw in (dict(), dict(psnr=30, ms_ssim=0.5), dict(ms_ssim=2)):
        with pytest.raises(ValueError):
            c.compress_to_quality(img, **kw)


def test_compress_to_quality_with_rois(cdc, img):
    from imgcomp_cvpr_amd import codec
    c = _set(cdc, tile=(8, 8))
    levels = codec.cap_levels(c.C)
    at = lambda lv: c.measure(img, c.compress(img, rois=ROIS, background=lv))
    m0, mC = at(0), at(c.C)
    target = 0.5 * (m0.psnr + mC.psnr)
    data, level, m, probes = c.compress_to_quality(img, psnr=target, rois=ROIS)
    k = int(np.nonzero(levels == np.float32(level))[0][0])
    print('rois: level 0 {}, uncapped {}, target {} -> level {} after {} probes: {}'.format(m0.psnr, mC.psnr, target, level, probes, m))
    assert data == c.compress(img, rois=ROIS, background=level) and m == c.measure(img, data) == at(level)
    assert m.psnr >= target and (k == 0 or not at(levels[k - 1]).psnr >= target)
    assert 1 <= probes <= PROBE_BOUND
    assert data != c.compress(img, cap=level) or level >= c.C                  # the rectangles stayed uncapped
    _set(cdc)


# ---- transcode_to_quality -------------------------------------------------------------------------------------------------------------

def test_transcode_to_quality(cdc, img, monkeypatch):
    c = _set(cdc, tile=(8, 8))
    source = c.compress(img)
    ref = c.decompress(source)
    _set(c, **FORMATS['fronts'])                                                 # the target format: another one than the source's
    curve = [c.measure(ref, c.transcode(source, cap=K)) for K in range(c.C + 1)]
    assert curve[c.C].psnr == float('inf') and curve[c.C].ms_ssim == 1.0 and curve[c.C].mse == 0.0
    finite = sorted(m.psnr for m in curve if math.isfinite(m.psnr))
    assert len(set(finite)) >= 3, 'fixture too flat'
    print('transcode: psnr per level {}'.format([m.psnr for m in curve]))

    def refuse(*args, **kw):
        raise AssertionError('a transcode to a quality ran the encoder')

    for ae in [c.ae] + [ae for _, ae in c._lanes(c.IN_FLIGHT)]:
        for name in ('encode', 'encode_capped', 'requantize'):
            monkeypatch.setattr(ae, name, refuse)
    with pytest.raises(AssertionError):
        c.compress(img)
    bound = 1 + 2 + int(math.ceil(math.log2(c.C)))
    for kw in (dict(psnr=finite[len(finite) // 2]), dict(psnr=finite[0] - 1.0), dict(ms_ssim=sorted(m.ms_ssim for m in curve if math.isfinite(m.ms_ssim))[c.C // 4])):
        (name, target), = kw.items()
        out, K, m, probes = c.transcode_to_quality(source, **kw)
        print('  {} >= {} -> K {} after {} probes: {}'.format(name, target, K, probes, m))
        assert out == c.transcode(source, cap=K) and m == curve[K] == c.measure(ref, out)
        assert getattr(m, name) >= target and (K == 0 or not getattr(curve[K - 1], name) >= target)
        assert 1 <= probes <= bound
    with pytest.raises(ValueError):
        c.transcode_to_quality(source)
    with pytest.raises(ValueError, match='CRC'):
        c.transcode_to_quality(source[:-1] + bytes([source[-1] ^ 1]), psnr=20)
    _set(cdc)


def test_transcode_to_an_infinite_psnr_keeps_every_channel(cuda, cdc):
    """only the picture itself is within inf dB of itself.  The source is written from a random symbol volume: the synthetic encoder's
    own files leave the top channels empty, so their levels below C are the same file and K = C could not be told from them"""
    c = _set(cdc, tile=(8, 8))
    H, W = 64, 96
    sym = torch.as_tensor(np.random.RandomState(7).randint(0, c.L, (c.C, H // 8, W // 8))).to(cuda)
    source = c._container(sym, H, W)
    out, K, m, probes = c.transcode_to_quality(source, psnr=float('inf'))
    assert K == c.C and out == c.transcode(source) == source
    assert (m.mse, m.psnr, m.ms_ssim, m.bytes) == (0.0, float('inf'), 1.0, len(out)) and probes == 3
    assert c.transcode_to_quality(source, psnr=0.0)[1::2] == (0, 1)            # 0 dB: any picture reaches it, level 0 after one probe
    _set(cdc)


# ---- the command line -----------------------------------------------------------------------------------------------------------------

def _cli(args, timeout=300):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    return subprocess.run([sys.executable, '-m', 'imgcomp_cvpr_amd.codec'] + args, cwd=ROOT, env=env, timeout=timeout,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


@pytest.fixture(scope='module')
def cli_case(cdc, pics, tmp_path_factory):
    """a picture on disk and a PSNR target halfway between its level 0 and its file without a cap, --tile 64"""
    from PIL import Image
    d = tmp_path_factory.mktemp('quality_cli')
    pic = pics['40x56']
    png = str(d / 'in.png')
    Image.fromarray(pic).save(png)
    c = _set(cdc, tile=(8, 8))
    target = 0.5 * (c.measure(pic, c.compress(pic, cap=0)).psnr + c.measure(pic, c.compress(pic)).psnr)
    _set(cdc)
    return d, pic, png, target


def test_cli_compress_to_a_psnr_and_measure(cdc, cli_case):
    from imgcomp_cvpr_amd import codec
    d, pic, png, target = cli_case
    icf = str(d / 'q.icf')
    c = _set(cdc, tile=(8, 8))
    data, level, m, probes = c.compress_to_quality(pic, psnr=target)
    r = _cli(['compress', png, icf, '--tile', '64', '--min-psnr', repr(target)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(icf, 'rb').read() == data
    assert r.stdout.strip() == codec._compress_line(icf, data, pic.shape[0] * pic.shape[1]) + codec._quality_note(level, m, probes), r.stdout
    r = _cli(['measure', png, icf, '--region', '8,8,32,24'])
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip() == codec._measure_line(icf, c.measure(pic, data, rect=(8, 8, 32, 24)), rect=(8, 8, 40, 32)), r.stdout
    r = _cli(['compress', png, icf, '--min-psnr', '30', '--cap', '4'])
    assert r.returncode == 2 and '--min-psnr does not go with --cap' in r.stderr
    _set(cdc)


def test_cli_rd(cdc, cli_case):
    from imgcomp_cvpr_amd import codec
    d, pic, png, _ = cli_case
    out = str(d / 'rd.json')
    c = _set(cdc, tile=(8, 8))
    rows = c.rd_curve(pic, levels=codec.rd_levels(c.C, 4))
    r = _cli(['rd', png, out, '--tile', '64', '--levels', '4'])
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.splitlines() == [codec._rd_line(level, m) for level, m in rows], r.stdout
    with open(out) as f:
        got = json.load(f)
    assert [(row['level'], codec.Measure(**{k: row[k] for k in codec.Measure._fields})) for row in got['rows']] == rows
    assert (got['format'], got['tile'], got['H'], got['W'], got['ae_config'], got['pc_config']) == (2, [64, 64], 40, 56, c.ae_name, c.pc_name)
    assert got == codec.rd_table(c, rows, png, 40, 56)
    _set(cdc)


def test_cli_transcode_to_a_psnr(cdc, cli_case):
    from imgcomp_cvpr_amd import codec
    d, pic, png, _ = cli_case
    src, dst = str(d / 'src.icf'), str(d / 'dst.icf')
    c = _set(cdc)
    source = c.compress(pic)
    with open(src, 'wb') as f:
        f.write(source)
    ref = c.decompress(source)
    _set(c, tile=(8, 8))
    finite = sorted(p for p in (c.measure(ref, c.transcode(source, cap=K)).psnr for K in range(0, c.C + 1, 4)) if math.isfinite(p))
    target = finite[len(finite) // 2]
    out, K, m, probes = c.transcode_to_quality(source, psnr=target)
    r = _cli(['transcode', src, dst, '--tile', '64', '--min-psnr', repr(target)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(dst, 'rb').read() == out
    assert r.stdout.strip() == codec._transcode_line(dst, source, out) + codec._quality_note(K, m, probes), r.stdout
    _set(cdc)


def test_cli_compress_dir_to_a_psnr(cdc, pics, tmp_path):
    """one target for the directory, a search per file: the smaller of the pictures' midpoints between level 0 and no cap, which
    every picture reaches at level 0 or without a cap"""
    from PIL import Image
    from imgcomp_cvpr_amd import codec
    src, dst = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    for name, pic in pics.items():
        Image.fromarray(pic).save(str(src / (name + '.png')))
    c = _set(cdc)
    target = min(0.5 * (c.measure(pic, c.compress(pic, cap=0)).psnr + c.measure(pic, c.compress(pic)).psnr) for pic in pics.values())
    r = _cli(['compress-dir', str(src), str(dst), '--min-psnr', repr(target)])
    assert r.returncode == 0, r.stderr[-2000:]
    for name, pic in pics.items():
        path = str(dst / (name + '.icf'))
        data, level, m, probes = c.compress_to_quality(pic, psnr=target)
        assert open(path, 'rb').read() == data, name
        assert codec._compress_line(path, data, pic.shape[0] * pic.shape[1]) + codec._quality_note(level, m, probes) in r.stdout.splitlines(), r.stdout
    r = _cli(['compress-dir', str(src), str(dst), '--min-psnr', repr(target), '--roi', '0,0,8,8'])
    assert r.returncode == 2 and '--roi belongs to compress' in r.stderr
