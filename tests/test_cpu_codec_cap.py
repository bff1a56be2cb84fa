"""Importance-map cap, the host side (no GPU): the two forms of the rule, the level grid, cap planes, the budget search's contract
on synthetic `fits` functions, the command line's refusals."""
import argparse

import numpy as np
import pytest

from imgcomp_cvpr_amd import codec
from tests import cap_rule as R

F = np.float32


# ---- the rule -----------------------------------------------------------------------------------------------------------------

def _caps(C):
    special = np.concatenate([[0.0], np.arange(0, C + 1), codec.cap_levels(C)[1::7], R.ulp_neighbours(np.arange(1, C + 1)), [C, np.inf]]).astype(F)
    return special[special >= 0]


@pytest.mark.parametrize('N,C,h,w', [(2, 32, 9, 13), (1, 5, 1, 1)])
def test_the_two_forms_agree_bit_for_bit(N, C, h, w):
    rs = np.random.RandomState(5)
    bott = rs.normal(0, 2, (N, C + 1, h, w)).astype(F)
    m, z = R.direct(bott, np.full((N, h, w), np.inf, F))
    assert m.dtype == F and z.dtype == F and m.min() == 0 and m.max() == 1 and ((m > 0) & (m < 1)).any()
    caps = _caps(C)
    planes = [np.full((N, h, w), c, F) for c in caps]                             # every special value everywhere ..
    planes += [rs.choice(caps, size=(N, h, w)).astype(F) for _ in range(8)]       # .. and mixed within a plane
    for cap in planes:
        m1, z1 = R.direct(bott, cap)
        m2, z2 = R.from_heatmap(m, cap, bott[:, 1:])
        assert np.array_equal(m1.view(np.uint32), m2.view(np.uint32)), float(cap.flat[0])
        assert np.array_equal(z1.view(np.uint32), z2.view(np.uint32)), float(cap.flat[0])
    for big in (F(C), np.nextafter(F(C), F(np.inf)), F(np.inf)):                  # consequence 1: cap >= C changes nothing
        m1, z1 = R.direct(bott, np.full((N, h, w), big, F))
        assert np.array_equal(m1.view(np.uint32), m.view(np.uint32)) and np.array_equal(z1.view(np.uint32), z.view(np.uint32))
    for K in sorted({1, 2, C - 1}):                                               # consequence 2: an integer cap cuts at a channel plane
        m1, z1 = R.direct(bott, np.full((N, h, w), K, F))
        assert np.array_equal(m1[:, :K].view(np.uint32), m[:, :K].view(np.uint32))
        assert np.array_equal(z1[:, :K].view(np.uint32), z[:, :K].view(np.uint32))
        assert not m1[:, K:].any() and not z1[:, K:].any()


def test_cap_levels():
    lv = codec.cap_levels(32)
    assert lv.dtype == F and lv.shape == (257,) and lv[0] == 0 and lv[-1] == 32
    assert np.array_equal(lv, np.arange(257, dtype=F) * F(0.125))
    for C in (5, 7, 64):
        lv = codec.cap_levels(C)
        assert lv.dtype == F and lv[0] == 0 and lv[256] == C and (np.diff(lv) > 0).all()
        assert np.array_equal(lv, np.array([F(k * C / 256.0) for k in range(257)], F))


# ---- cap_plane ----------------------------------------------------------------------------------------------------------------

H, W, FACTOR = 61, 93, 8                    # pads: top (3 // 2) = 1, left (3 // 2) = 1; the plane is 8 x 12


def _cells(plane, value):
    return sorted((int(y), int(x)) for y, x in zip(*np.nonzero(plane == F(value))))


def test_cap_plane_levels():
    p = codec.cap_plane(H, W, FACTOR)
    assert p.shape == (8, 12) and p.dtype == F and np.isinf(p).all()
    p = codec.cap_plane(H, W, FACTOR, level=2.5)
    assert p.shape == (8, 12) and p.dtype == F and (p == F(2.5)).all()
    assert (codec.cap_plane(H, W, FACTOR, level=0) == 0).all()
    assert codec.cap_plane(64, 96, FACTOR, level=1).shape == (8, 12) and codec.cap_plane(65, 97, FACTOR, level=1).shape == (9, 13)


def test_cap_plane_rectangles():
    # one pixel: image pixel (x, y) is padded pixel (x + 1, y + 1)
    p = codec.cap_plane(H, W, FACTOR, level=4, rois=[(20, 30, 1, 1)], background=1)
    assert _cells(p, 4) == [(31 // 8, 21 // 8)] and (p == 1).sum() == 8 * 12 - 1
    # a rectangle that touches one pixel of the next cell: x = 0 .. 7 is padded 1 .. 8, which reaches cell 1 by its last pixel
    assert _cells(codec.cap_plane(H, W, FACTOR, level=4, rois=[(0, 0, 7, 7)], background=1), 4) == [(0, 0)]
    assert _cells(codec.cap_plane(H, W, FACTOR, level=4, rois=[(0, 0, 8, 7)], background=1), 4) == [(0, 0), (0, 1)]
    assert _cells(codec.cap_plane(H, W, FACTOR, level=4, rois=[(0, 0, 7, 8)], background=1), 4) == [(0, 0), (1, 0)]
    # on the pad boundary: image x = 6 is the last pixel of cell 0, x = 7 the first of cell 1 (a centred pad shifts the grid by one)
    assert _cells(codec.cap_plane(H, W, FACTOR, level=4, rois=[(6, 6, 1, 1)], background=1), 4) == [(0, 0)]
    assert _cells(codec.cap_plane(H, W, FACTOR, level=4, rois=[(7, 7, 1, 1)], background=1), 4) == [(1, 1)]
    # the last pixel of the image: padded (93, 61) -> cell (7, 11); the cells hold the bottom / right pad as well
    assert _cells(codec.cap_plane(H, W, FACTOR, level=4, rois=[(92, 60, 1, 1)], background=1), 4) == [(7, 11)]
    # the whole image, and a rectangle larger than it (clipped): every cell
    for r in ((0, 0, W, H), (-5, -5, W + 50, H + 50)):
        assert (codec.cap_plane(H, W, FACTOR, level=4, rois=[r], background=1) == 4).all()
    # level None inside: +inf
    p = codec.cap_plane(H, W, FACTOR, rois=[(0, 0, 7, 7)], background=0.5)
    assert np.isinf(p[0, 0]) and (p.reshape(-1)[1:] == F(0.5)).all()
    # two overlapping rectangles: the union
    p = codec.cap_plane(H, W, FACTOR, level=4, rois=[(7, 7, 16, 8), (15, 7, 16, 16)], background=1)
    a = {(1, 1), (1, 2)}                                                  # padded x 8 .. 23, y 8 .. 15
    b = {(y, x) for y in (1, 2) for x in (2, 3)}                          # padded x 16 .. 31, y 8 .. 23
    assert set(_cells(p, 4)) == a | b and (p == 1).sum() == 96 - len(a | b)
    # an image that needs no padding
    assert _cells(codec.cap_plane(64, 96, FACTOR, level=4, rois=[(8, 8, 8, 8)], background=1), 4) == [(1, 1)]


@pytest.mark.parametrize('kw,word', [
    (dict(level=4, rois=[(93, 0, 4, 4)], background=1), 'does not intersect'),
    (dict(level=4, rois=[(0, 61, 4, 4)], background=1), 'does not intersect'),
    (dict(level=4, rois=[(-4, 0, 4, 4)], background=1), 'does not intersect'),
    (dict(level=4, rois=[(0, 0, 0, 4)], background=1), 'not positive'),
    (dict(level=4, rois=[(0, 0, 4, -1)], background=1), 'not positive'),
    (dict(level=-0.5), 'not in [0, +inf]'),
    (dict(level=float('nan')), 'not in [0, +inf]'),
    (dict(level=4, rois=[(0, 0, 4, 4)], background=-1), 'not in [0, +inf]'),
    (dict(level=4, rois=[(0, 0, 4, 4)], background=float('nan')), 'not in [0, +inf]'),
    (dict(level=4, rois=[(0, 0, 4, 4)]), 'needs a background'),
    (dict(level=4, rois=[(0, 0, 4)], background=1), 'is not (x, y, w, h)'),
])
def test_cap_plane_refusals(kw, word):
    with pytest.raises(ValueError) as e:
        codec.cap_plane(H, W, FACTOR, **kw)
    assert word in str(e.value), str(e.value)


# ---- budget_search ------------------------------------------------------------------------------------------------------------

def _run(table, estimate):
    calls = []

    def fits(k):
        assert 0 <= k <= 256
        calls.append(k)
        return bool(table[k])

    k, probes = codec.budget_search(fits, estimate)
    assert probes == len(calls) <= 12, (estimate, calls)
    assert len(set(calls)) == len(calls), (estimate, calls)                       # no index coded twice
    assert k in calls and table[k], (estimate, k, calls)                          # fits(k) was established by a call ..
    assert k == 256 or (k + 1 in calls and not table[k + 1]), (estimate, k, calls)    # .. and so was not fits(k + 1)
    assert calls[0] == 256
    return k, calls


def test_budget_search_monotone():
    for threshold in list(range(0, 257, 5)) + [1, 2, 254, 255, 256]:
        table = [k <= threshold for k in range(257)]
        for estimate in range(257):
            k, calls = _run(table, estimate)
            assert k == threshold
            if estimate == threshold and threshold < 256:
                assert len(calls) <= 3, calls                                     # a right estimate costs its own pair


def test_budget_search_non_monotone():
    rs = np.random.RandomState(7)
    tables = [[(k * 37) % 11 < 6 for k in range(257)], [k % 2 == 0 for k in range(257)], [k < 40 or 100 < k < 130 for k in range(257)]]
    tables += [list(rs.rand(257) < p) for p in (0.1, 0.5, 0.9)]
    for table in tables:
        table[0], table[256] = True, False
        for estimate in range(257):
            _run(table, estimate)


def test_budget_search_all_fit_and_none_fit():
    for estimate in range(257):
        k, calls = _run([True] * 257, estimate)
        assert k == 256 and calls == [256]
        calls = []
        with pytest.raises(ValueError) as e:
            codec.budget_search(lambda k: calls.append(k) or False, estimate)
        assert 'smallest file' in str(e.value) and 'bytes' in str(e.value)
        assert len(calls) <= 12 and len(set(calls)) == len(calls) and 0 in calls
    table = [False] * 257
    table[0] = True
    for estimate in range(257):
        assert _run(table, estimate)[0] == 0
    for estimate in (-3, 1000):                                                   # advice only: any integer is taken
        assert _run([k <= 77 for k in range(257)], estimate)[0] == 77


# ---- the command line ---------------------------------------------------------------------------------------------------------

def _flags(command='compress', **kw):
    base = dict(command=command, tile=None, checked=False, wavefront=False, salvage=False, channels=None, layers=None, progressive=False,
                front_layers=None, front_progressive=False, partial=False, recover=False, chunk=None, fronts=False,
                cap=None, roi=None, background=None, max_bytes=None, bpp=None)
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.mark.parametrize('kw,words', [
    (dict(roi=['0,0,8,8']), ('--roi needs --background or a budget',)),
    (dict(cap=4.0, roi=['0,0,8,8']), ('--roi needs --background or a budget',)),
    (dict(cap=4.0, max_bytes=1000), ('--cap does not go with --max-bytes',)),
    (dict(cap=4.0, bpp=0.5), ('--cap does not go with --bpp',)),
    (dict(max_bytes=1000, bpp=0.5), ('--max-bytes does not go with --bpp',)),
    (dict(command='compress-dir', roi=['0,0,8,8'], background=1.0), ('--roi belongs to compress',)),
    (dict(command='decompress', cap=4.0), ('--cap belongs to compress / compress-dir',)),
    (dict(command='decompress-dir', max_bytes=100), ('--max-bytes belongs to compress / compress-dir',)),
    (dict(command='stream', bpp=1.0), ('--bpp belongs to compress / compress-dir',)),
    (dict(command='decompress', roi=['0,0,8,8'], background=1.0), ('belongs to compress',)),
    (dict(background=1.0), ('--background needs --roi',)),
    (dict(cap=-1.0), ('--cap', 'not in [0, +inf]')),
    (dict(cap=float('nan')), ('--cap', 'not in [0, +inf]')),
    (dict(roi=['0,0,8,8'], background=-2.0), ('--background', 'not in [0, +inf]')),
    (dict(roi=['0,0,8'], background=1.0), ('--roi', 'X,Y,W,H')),
    (dict(roi=['0,0,8,0'], background=1.0), ('--roi', 'not positive')),
    (dict(roi=['a,0,8,8'], background=1.0), ('--roi', 'X,Y,W,H')),
    (dict(max_bytes=0), ('--max-bytes 0 is not at least 1',)),
    (dict(bpp=0.0), ('--bpp', 'not above 0')),
])
def test_cli_option_refusals(kw, words):
    with pytest.raises(ValueError) as e:
        codec.check_option_args(_flags(**kw))
    for word in words:
        assert word in str(e.value), str(e.value)


def test_cli_options_accepted():
    for kw in (dict(cap=4.0), dict(cap=0.0), dict(cap=float('inf')), dict(roi=['0,0,8,8'], background=1.0), dict(cap=8.0, roi=['0,0,8,8', '9,9,1,1'], background=1.0),
               dict(max_bytes=1000), dict(bpp=0.25), dict(roi=['0,0,8,8'], max_bytes=1000), dict(roi=['0,0,8,8'], bpp=0.5),
               dict(command='compress-dir', cap=4.0), dict(command='compress-dir', max_bytes=500), dict(command='compress-dir', bpp=0.5),
               dict(tile=128, cap=4.0, checked=True), dict(tile=128, max_bytes=900, front_progressive=True)):
        codec.check_option_args(_flags(**kw))
    codec.check_option_args(argparse.Namespace(command='decompress', tile=None))           # a command line from before the options
    assert codec.parse_roi_arg('3,-4,5,6') == (3, -4, 5, 6)
