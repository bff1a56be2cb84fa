"""no GPU: the host side of the quality axis -- codec.quality_search on every kind of predicate, the refusals of the new options on
bare namespaces, the argument checks of measure / rd / the quality targets, and how a Measure follows from the six device values."""
import argparse
import math

import numpy as np
import pytest

from imgcomp_cvpr_amd import codec, metrics


# ---- quality_search -----------------------------------------------------------------------------------------------------------

def _bound(steps):
    return 1 + 2 + int(math.ceil(math.log2(steps)))


def _run(table):
    """quality_search over a list of booleans -> (k, probes), with its contract and its promises checked against the list"""
    steps, calls = len(table) - 1, []

    def meets(k):
        assert 0 <= k <= steps
        calls.append(k)
        return table[k]

    k, probes = codec.quality_search(meets, steps)
    assert probes == len(calls) == len(set(calls)), 'a call was repeated: {}'.format(calls)
    assert probes <= _bound(steps), (probes, steps)
    assert table[k] and k in calls
    assert k == 0 or (not table[k - 1] and k - 1 in calls), 'the level below was not established by a call'
    return k, probes


@pytest.mark.parametrize('steps', [1, 2, 3, 32, 33, 256])
def test_monotone_predicates(steps):
    for first in range(steps + 1):
        k, _ = _run([i >= first for i in range(steps + 1)])
        assert k == first


def test_all_true_only_top_true_and_the_bound_reached():
    assert _run([True] * 257) == (0, 1)
    assert _run([False] * 256 + [True]) == (256, 3)              # 0, the top, the one below it: an adjacent pair already
    assert _run([False] + [True] * 256) == (1, _bound(256))      # the bound is reached: the whole bisection behind the three
    assert _run([True, True]) == (0, 1) and _run([False, True]) == (1, 2)


def test_non_monotone_shape_of_the_synthetic_weights():
    """true, false, false, true ..: level 0 is better than the levels behind it.  With the target met at 0 that is the answer; with
    0 just under the target the search still ends on a pair (false, true) whatever lies between"""
    assert _run([True, False, False] + [True] * 30) == (0, 1)
    table = [False, True, False, False] + [True] * 29
    k, _ = _run(table)
    assert k in (1, 4)
    rs = np.random.RandomState(3)
    for _ in range(200):
        steps = int(rs.randint(1, 80))
        _run([bool(b) for b in rs.rand(steps) < 0.5] + [True])


def test_refusal_when_the_top_level_fails():
    calls = []

    def meets(k):
        calls.append(k)
        return k == 3

    with pytest.raises(ValueError, match='no level meets the target'):
        codec.quality_search(meets, 32)
    assert calls == [0, 32]
    with pytest.raises(ValueError, match='at least 1'):
        codec.quality_search(lambda k: True, 0)

    def broken(k):
        raise ValueError('the probe itself')

    with pytest.raises(ValueError, match='the probe itself'):
        codec.quality_search(broken, 8)


def _recorded_curve():
    """257 PSNR values of the shape the synthetic weights give: a narrow band, not monotone, flat at the top"""
    rs = np.random.RandomState(11)
    curve = 13.58 + 0.03 * np.sin(np.arange(257) / 9.0) + 0.004 * rs.randn(257)
    curve[224:] = curve[256]
    return [float(np.float32(v)) for v in curve]


def test_every_target_on_a_recorded_curve():
    curve = _recorded_curve()
    assert len(set(curve)) > 200 and curve[0] > min(curve)
    for target in sorted(set(curve)) + [min(curve) - 1.0]:
        if curve[0] >= target:                                   # level 0 is asked first and is the answer, whatever the top does
            assert _run([v >= target for v in curve]) == (0, 1)
        elif curve[256] >= target:
            k, _ = _run([v >= target for v in curve])
            assert curve[k] >= target and curve[k - 1] < target
        else:
            with pytest.raises(ValueError):
                codec.quality_search(lambda k: curve[k] >= target, 256)
    assert _run([v >= min(curve) - 1.0 for v in curve]) == (0, 1)


# ---- a Measure from the device's six values ---------------------------------------------------------------------------------------

def test_measure_from_values():
    vals = [0.9, 0.8, 0.7, 0.95, 0.6]
    m = codec.measure_from_values(vals + [4.0], 1200, 64 * 96)
    assert m == codec.Measure(1200, 8.0 * 1200 / (64 * 96), 4.0, metrics.psnr_from_mse(4.0), metrics.msssim_from_scale_values(vals))
    assert codec.measure_from_values([1.0] * 5 + [0.0], 10, 100).psnr == float('inf')
    for bad in (-0.1, float('nan')):
        for at in range(5):
            m = codec.measure_from_values(vals[:at] + [bad] + vals[at + 1:] + [4.0], 1200, 64 * 96)
            assert isinstance(m.ms_ssim, float) and math.isnan(m.ms_ssim) and m.psnr == metrics.psnr_from_mse(4.0)
    # what the NumPy code gives there
    w = np.array(metrics._MSSSIM_WEIGHTS)
    with np.errstate(invalid='ignore'):
        assert math.isnan(float(np.prod(np.array([0.9, -0.1, 0.7, 0.95]) ** w[:-1]) * 0.6 ** w[-1]))
    assert codec.measure_from_values([0.0] + vals[1:] + [4.0], 1, 1).ms_ssim == 0.0
    with pytest.raises(ValueError):
        codec.measure_from_values(vals, 1, 1)


def test_a_nan_never_meets_a_target():
    m = codec.Measure(1, 1.0, 4.0, 42.0, float('nan'))
    assert not codec.meets_target(m, 'ms_ssim', 0.0) and codec.meets_target(m, 'psnr', 42.0) and not codec.meets_target(m, 'psnr', 42.5)
    assert codec.meets_target(m._replace(psnr=float('inf')), 'psnr', float('inf'))


# ---- arguments that need no device ---------------------------------------------------------------------------------------------------

def test_measured_image_shape():
    img = np.zeros((61, 93, 3), np.uint8)
    assert codec.check_measured_image(img, 61, 93) is not None
    assert codec.check_measured_image(np.zeros((61, 93, 4), np.uint8), 61, 93).shape == (61, 93, 3)
    with pytest.raises(ValueError) as e:
        codec.check_measured_image(img, 64, 96)
    assert '61 x 93' in str(e.value) and '64 x 96' in str(e.value)
    for bad in (img.astype(np.float32), img[:, :, 0], np.zeros((61, 93, 2), np.uint8)):
        with pytest.raises(ValueError):
            codec.check_measured_image(bad, 61, 93)


def test_measure_rect():
    assert codec.measure_rect((10, 20, 30, 16), 61, 93) == (10, 20, 40, 36)
    assert codec.measure_rect((-5, -5, 40, 40), 61, 93) == (0, 0, 35, 35)              # clipped as --roi clips
    for rect in ((0, 0, 15, 40), (0, 0, 40, 15), (80, 0, 40, 40), (0, 50, 40, 40)):    # under 16 a side, before or after clipping
        with pytest.raises(ValueError, match='at least 16'):
            codec.measure_rect(rect, 61, 93)
    for rect in ((200, 0, 20, 20), (0, 0, 0, 20), 'x'):
        with pytest.raises(ValueError):
            codec.measure_rect(rect, 61, 93)


def test_quality_target():
    assert codec.quality_target(psnr=30) == ('psnr', 30.0) and codec.quality_target(ms_ssim=0.9) == ('ms_ssim', 0.9)
    assert codec.quality_target(psnr=float('inf')) == ('psnr', float('inf'))
    with pytest.raises(ValueError, match='both'):
        codec.quality_target(psnr=30, ms_ssim=0.9)
    with pytest.raises(ValueError, match='neither'):
        codec.quality_target()
    for kw in (dict(psnr=float('nan')), dict(psnr='x'), dict(ms_ssim=1.5), dict(ms_ssim=-0.1), dict(ms_ssim=float('nan'))):
        with pytest.raises(ValueError):
            codec.quality_target(**kw)


def test_rd_levels():
    assert codec.rd_levels(32) == [2.0 * k for k in range(17)] == codec.check_rd_levels(None, 32)
    assert codec.rd_levels(32, 1) == [0.0, 32.0] and len(codec.rd_levels(32, 256)) == 257
    assert [np.float32(v) for v in codec.rd_levels(32, 256)] == list(codec.cap_levels(32))
    for bad in (0, 257, -1, 2.5, '4', True, None):
        with pytest.raises(ValueError, match='--levels'):
            codec.rd_levels(32, bad)
    assert codec.check_rd_levels([0, 2.5, float('inf')], 32) == [0.0, 2.5, float('inf')]
    for bad in ([], [1, 1], [2, 1], [-1, 2], [float('nan')], 4, ['x']):
        with pytest.raises(ValueError):
            codec.check_rd_levels(bad, 32)


# ---- the command line's options -----------------------------------------------------------------------------------------------------

def _flags(command='compress', **kw):
    base = dict(command=command, tile=None, checked=False, wavefront=False, salvage=False, channels=None, layers=None, progressive=False,
                front_layers=None, front_progressive=False, partial=False, recover=False, chunk=None, fronts=False,
                cap=None, roi=None, background=None, max_bytes=None, bpp=None, region=None, min_psnr=None, min_ms_ssim=None, levels=None)
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.mark.parametrize('command,kw,words', [
    ('compress', dict(min_psnr=30.0, min_ms_ssim=0.9), '--min-psnr does not go with --min-ms-ssim'),
    ('compress', dict(min_psnr=30.0, cap=4.0), '--min-psnr does not go with --cap'),
    ('compress', dict(min_ms_ssim=0.9, max_bytes=1000), '--min-ms-ssim does not go with --max-bytes'),
    ('compress-dir', dict(min_psnr=30.0, bpp=0.5), '--min-psnr does not go with --bpp'),
    ('compress', dict(min_psnr=30.0, roi=['0,0,8,8'], background=1.0), '--min-psnr does not go with --background'),
    ('compress-dir', dict(min_psnr=30.0, roi=['0,0,8,8']), '--roi belongs to compress'),
    ('compress', dict(min_psnr=float('nan')), 'psnr target'),
    ('compress', dict(min_ms_ssim=1.5), 'ms_ssim target'),
    ('decompress', dict(min_psnr=30.0), '--min-psnr belongs to compress'),
    ('stream', dict(min_ms_ssim=0.5), '--min-ms-ssim belongs to compress'),
    ('measure', dict(min_psnr=30.0), '--min-psnr belongs to compress'),
    ('rd', dict(min_psnr=30.0), '--min-psnr belongs to compress'),
    ('transcode', dict(min_psnr=30.0, salvage=True), '--min-psnr does not go with --salvage'),
    ('transcode-dir', dict(min_ms_ssim=0.9, recover=True), '--min-ms-ssim does not go with --recover'),
    ('transcode', dict(min_psnr=30.0, roi=['0,0,8,8']), '--min-psnr does not go with --roi'),
    ('transcode', dict(min_psnr=30.0, cap=4.0), '--min-psnr does not go with --cap'),
    ('compress', dict(levels=16), '--levels belongs to rd'),
    ('rd', dict(levels=0), '--levels 0'),
    ('rd', dict(levels=257), '--levels 257'),
    ('rd', dict(cap=4.0), '--cap belongs to compress'),
    ('rd', dict(max_bytes=100), '--max-bytes belongs to compress'),
    ('rd', dict(roi=['0,0,8']), '--roi'),
    ('rd', dict(checked=True), '--checked needs --tile'),
    ('rd', dict(salvage=True), '--salvage belongs to decompress'),
    ('measure', dict(tile=64), '--tile belongs to compress'),
    ('measure', dict(checked=True, tile=64), '--tile belongs to compress'),
    ('measure', dict(roi=['0,0,8,8']), '--roi belongs to compress'),
    ('measure', dict(region='0,0,8'), '--region'),
    ('measure', dict(region='0,0,40,15'), 'at least 16 pixels a side'),
    ('measure', dict(channels=0), '--channels 0 is not at least 1'),
    ('measure', dict(recover=True), '--recover belongs to decompress'),
    ('rd', dict(region='0,0,32,32'), '--region belongs to decompress'),
    ('rd', dict(channels=4), '--channels belongs to decompress'),
])
def test_option_refusals(command, kw, words):
    with pytest.raises(ValueError) as e:
        codec.check_option_args(_flags(command, **kw))
    assert words in str(e.value), str(e.value)


def test_options_that_pass():
    for command, kw in (('compress', dict(min_psnr=30.0)), ('compress', dict(min_ms_ssim=0.9, tile=64, checked=True)),
                        ('compress', dict(min_psnr=30.0, roi=['0,0,8,8'])), ('compress-dir', dict(min_ms_ssim=1.0)),
                        ('transcode', dict(min_psnr=float('inf'))), ('transcode-dir', dict(min_ms_ssim=0.0, tile=64)),
                        ('measure', {}), ('measure', dict(channels=4, region='0,0,32,32')),
                        ('rd', {}), ('rd', dict(levels=256, tile=64, front_progressive=True)), ('rd', dict(roi=['0,0,8,8'], levels=1))):
        codec.check_option_args(_flags(command, **kw))
    # namespaces from before the options pass where they passed
    for command in ('compress', 'decompress', 'transcode', 'stream'):
        codec.check_option_args(argparse.Namespace(command=command, tile=None))
    codec.check_option_args(argparse.Namespace(command='compress', tile=None, roi=['0,0,8,8'], background=1.0))
    with pytest.raises(ValueError, match='--roi needs --background or a budget'):
        codec.check_option_args(argparse.Namespace(command='compress', tile=None, roi=['0,0,8,8']))


def test_dir_refusals_come_before_the_directories(tmp_path):
    for command, kw, words in (('compress-dir', dict(min_psnr=30.0, cap=4.0), '--min-psnr does not go with --cap'),
                               ('transcode-dir', dict(min_psnr=30.0, salvage=True), '--min-psnr does not go with --salvage'),
                               ('decompress-dir', dict(min_ms_ssim=0.5), '--min-ms-ssim belongs to compress')):
        flags = _flags(command, batch=8, input=str(tmp_path / 'missing'), output=str(tmp_path / 'out'), **kw)
        with pytest.raises(ValueError) as e:
            codec.check_dir_args(flags, 8)
        assert words in str(e.value), str(e.value)
    (tmp_path / 'in').mkdir()
    (tmp_path / 'in' / 'a.png').write_bytes(b'')
    jobs, tile = codec.check_dir_args(_flags('compress-dir', batch=8, input=str(tmp_path / 'in'), output=str(tmp_path / 'out'), min_psnr=30.0), 8)
    assert len(jobs) == 1 and tile is None


def test_printed_lines():
    m = codec.Measure(1200, 1.5625, 4.0, 42.1102, 0.912345)
    assert codec._quality_note(2.5, m, 7) == ', cap level 2.5 after 7 probes: PSNR 42.1102 dB, MS-SSIM 0.912345, MSE 4.0000'
    assert codec._measure_line('a.icf', m) == 'a.icf: 1200 bytes = 1.5625 bpp, PSNR 42.1102 dB, MS-SSIM 0.912345, MSE 4.0000'
    assert codec._measure_line('a.icf', m, 4, 32, (0, 0, 32, 16)).endswith(', of the region x 0..32 y 0..16, preview from 4 of 32 channels')
    assert codec._rd_line(8.0, m).startswith('level 8: 1200 bytes = 1.5625 bpp, PSNR')
    assert codec._quality_of(argparse.Namespace()) is None and codec._quality_of(_flags(min_ms_ssim=0.5)) == {'ms_ssim': 0.5}
