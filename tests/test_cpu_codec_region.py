"""Region decode on the host: the decoder's reach (decoder_reach) against the float64 oracle by the impulse method, region_plan
against a brute-force statement of its rule, the refusals of decompress_region and of the command line, and `info`."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest

from imgcomp_cvpr_amd import codec
from tests import codec_golden_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 8


# ---- the reach ------------------------------------------------------------------------------------------------------------------

def test_reach_is_walked_through_the_layer_list():
    from imgcomp_cvpr_amd import weights as W
    for B in (0, 1, 2, 5):
        layers = codec.decoder_layers(B)
        dec = [(s, k, shape) for s, k, shape in W.ae_conv_specs(32, B) if s.startswith(W.DEC + '/')]
        assert len(layers) == len(dec) == 6 * B + 5
        assert layers[0] == (3, 2) and layers[-2:] == [(5, 2), (5, 2)] and set(layers[1:-2]) == {(3, 1)}
        n3 = 6 * B + 2
        assert codec.decoder_reach(B) == (4 * n3 + 3, 4 * n3 + 10)
    assert codec.decoder_reach(5) == (131, 138)
    # in cells: pixel p depends on the cells ceil((p - 7 - after) / 8) .. floor((p + before) / 8): up to 18 before and 17 after for B = 5
    pixels = range(1000, 1008)                                               # the 8 pixels of cell 125
    assert max(125 + (138 + 7 - p) // 8 for p in pixels) == 18 and max((p + 131) // 8 - 125 for p in pixels) == 17
    with pytest.raises(ValueError, match='negative'):
        codec.decoder_reach(-1)


def _impulse_box(B, amp, cell=(20, 20), latent=40):
    """the bounding box of the pixels oracle.decode changes when `amp` is added to every channel of one latent cell of a random
    volume -> (before, after) per axis, in pixels from the cell's 8 x 8 block.  Both decodes have one shape, so an untouched pixel
    is the same sum in the same order: equal, not close."""
    import torch
    from imgcomp_cvpr_amd import config_parser as cp, weights as W
    from oracle import oracle as O
    ae_cfg, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc_cfg, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    ae_cfg._values['arch_param_B'] = B
    wts = W.synthetic_weights(ae_cfg, pc_cfg)
    q = torch.as_tensor(np.random.RandomState(B).normal(0, 1, (1, ae_cfg.num_chan_bn, latent, latent)))
    base = O.decode(q, wts, ae_cfg.as_dict())
    assert base.dtype == torch.float64 and not bool(((base == 0) | (base == 255)).any())          # (the clip hides nothing)
    q2 = q.clone()
    q2[0, :, cell[0], cell[1]] += amp
    changed = (O.decode(q2, wts, ae_cfg.as_dict()) != base).any(dim=1)[0].numpy()
    ys, xs = np.flatnonzero(changed.any(1)), np.flatnonzero(changed.any(0))
    return (F * cell[0] - ys.min(), ys.max() - (F * cell[0] + F - 1)), (F * cell[1] - xs.min(), xs.max() - (F * cell[1] + F - 1))


@pytest.mark.parametrize('B', [1, 2])
def test_reach_against_the_oracle(B):
    """the shallow decoders: the impulse reaches exactly as far as decoder_reach says, in both axes"""
    rows, cols = _impulse_box(B, 1.0)
    assert rows == cols == codec.decoder_reach(B), (B, rows, cols)


def test_reach_of_the_shipped_depth_against_the_oracle():
    """B = 5: behind 32 layers the impulse arrives at the rim of its box at an ulp of the pixel (1.4e-14 measured), so the last
    pixels may or may not differ.  Asserted: nothing changes OUTSIDE the box of decoder_reach (the property a window rests on), and
    the box found is less than one cell smaller (the rule does not ask for a tile too many)."""
    before, after = codec.decoder_reach(5)
    for got in _impulse_box(5, 4.0):
        assert got[0] <= before and got[1] <= after, got
        assert got[0] > before - F and got[1] > after - F, got


def _touched_pixels(cell, ncells, B, f4_convs, f4_h12):
    """one axis, forwards and output by output: which pixels read a value that the cell has touched.  Every layer is stated by the
    inputs ONE output reads: a SAME convolution of extent k its k neighbours; a stride-2 transposed one the inputs i with
    o = 2 i + t - pad; an F(4x4) output 4 n + r the inputs 4 n - 1 .. 4 n + 3 (r = 0), 4 n .. 4 n + 3 (r = 1, 2), 4 n .. 4 n + 4 (r = 3)."""
    f4 = lambda o: {0: (4 * (o // 4) - 1, 4 * (o // 4) + 3), 3: (4 * (o // 4), 4 * (o // 4) + 4)}.get(o % 4, (4 * (o // 4), 4 * (o // 4) + 3))
    x = np.zeros(ncells, bool)
    x[cell] = True
    layers = codec.decoder_layers(B)
    for n, (k, up) in enumerate(layers):
        y = np.zeros(len(x) * up, bool)
        for o in range(len(y)):
            if up == 2 and f4_h12 and n == len(layers) - 2:
                lo, hi = f4(o // 2)
            elif up == 2:
                pad = (k - 2) // 2
                ins = [(o - t + pad) // 2 for t in range(k) if (o - t + pad) % 2 == 0]
                lo, hi = min(ins), max(ins)
            elif f4_convs:
                lo, hi = f4(o)
            else:
                lo, hi = o - k // 2, o + k // 2
            y[o] = x[max(lo, 0):max(hi + 1, 0)].any()
        x = y
    return x


@pytest.mark.parametrize('f4_convs,f4_h12', [(False, False), (True, True), (True, False), (False, True)])
def test_decoder_cells_against_a_forward_walk(f4_convs, f4_h12):
    for B, ncells, cells in ((1, 40, (0, 1, 17, 18, 19, 20, 39)), (2, 56, (0, 26, 27, 55)), (5, 96, (0, 47, 48, 49, 50, 95))):
        touched = {c: _touched_pixels(c, ncells, B, f4_convs, f4_h12) for c in cells}
        for p in range(8 * ncells):
            lo, hi = codec.decoder_cells(p, p, B, f4_convs, f4_h12)
            for c in cells:
                assert touched[c][p] == (lo <= c <= hi), (B, c, p, lo, hi)
        # an interval of pixels reads the union
        assert codec.decoder_cells(100, 131, B, f4_convs, f4_h12) == (codec.decoder_cells(100, 100, B, f4_convs, f4_h12)[0],
                                                                     codec.decoder_cells(131, 131, B, f4_convs, f4_h12)[1])


def test_decoder_cells_without_f4_is_the_reach():
    for B in (1, 2, 5):
        before, after = codec.decoder_reach(B)
        for p in range(0, 3000, 7):
            assert codec.decoder_cells(p, p + 11, B) == (-((after + 7 - p) // 8), (p + 11 + before) // 8)
    # F(4x4) reads about two positions a layer where the arithmetic needs one: up to 35 cells before a pixel's own and 34 after
    # for B = 5, where the arithmetic needs 18 and 17
    spans = [tuple(c - p // 8 for c in codec.decoder_cells(p, p, 5, True, True)) for p in range(1000, 1064)]
    assert (min(a for a, _ in spans), max(a for a, _ in spans), min(b for _, b in spans), max(b for _, b in spans)) == (-35, -33, 32, 34)
    spans = [tuple(c - p // 8 for c in codec.decoder_cells(p, p, 5)) for p in range(1000, 1064)]
    assert (min(a for a, _ in spans), max(b for _, b in spans)) == (-18, 17)


# ---- the plan -------------------------------------------------------------------------------------------------------------------

def _brute(H, W, h, w, th, tw, rect, reach, align=1):
    """the rule, pixel by pixel: mark the cells every pixel of the clipped rectangle depends on, take the tiles they touch"""
    if callable(reach):
        of_pixel = lambda p: reach(p, p)
    else:
        before, after = reach
        of_pixel = lambda p: (int(np.ceil((p - (F - 1) - after) / float(F))), int(np.floor((p + before) / float(F))))
    x, y, rw, rh = rect
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + rw, W), min(y + rh, H)
    top, left = ((-H) % F) // 2, ((-W) % F) // 2
    need = np.zeros((h, w), bool)
    rows, cols = np.zeros(h, bool), np.zeros(w, bool)
    for p in range(y0 + top, y1 + top):
        lo, hi = of_pixel(p)
        rows[max(lo, 0):min(hi, h - 1) + 1] = True
    for p in range(x0 + left, x1 + left):
        lo, hi = of_pixel(p)
        cols[max(lo, 0):min(hi, w - 1) + 1] = True
    need[np.ix_(rows, cols)] = True
    grid = codec.tile_grid(h, w, th, tw)
    tiles = [t for t, (a, b, c, d) in enumerate(grid) if need[a:a + c, b:b + d].any()]
    ncols = -(-w // tw)
    r0, r1, c0, c1 = min(t // ncols for t in tiles), max(t // ncols for t in tiles) + 1, min(t % ncols for t in tiles), max(t % ncols for t in tiles) + 1
    while (r0 * th) % align:
        r0 -= 1
    while (c0 * tw) % align:
        c0 -= 1
    tiles = [r * ncols + c for r in range(r0, r1) for c in range(c0, c1)]
    return (x0, y0, x1 - x0, y1 - y0), (r0, r1), (c0, c1), tiles, (y0 + top, x0 + left)


def _rects(H, W):
    s = 16
    out = [(0, 0, s, s), (W - s, 0, s, s), (0, H - s, s, s), (W - s, H - s, s, s),                     # corners
           (W // 2, 0, s, s), (W // 2, H - s, s, s), (0, H // 2, s, s), (W - s, H // 2, s, s),          # edges
           (W // 2 - 5, H // 2 - 3, s, s), (W // 3, H // 3, 40, 24),                                     # interior
           (0, 0, W, H),                                                                                 # the whole image
           (0, 0, 1, 1), (W - 1, H - 1, 1, 1), (W // 2, H // 2, 1, 1),                                   # one pixel
           (-20, -30, 40, 50), (W - 7, H - 9, 100, 100), (-5, H // 2, W + 10, 3), (-1000, -1000, 5000, 5000)]       # poking out: clipped
    return out


@pytest.mark.parametrize('H,W', [(256, 384), (250, 380), (333, 517), (64, 64), (8, 9)])
@pytest.mark.parametrize('tile', [4, 8, 16])
def test_region_plan_against_brute_force(H, W, tile):
    h, w = -(-H // F), -(-W // F)
    for B, align in ((1, 1), (5, 1), (5, 2), (2, 2), (-1, 2)):
        # (-1: the reach as a function of the pixels, the F(4x4) kernels' of B = 1 -- short enough to leave windows in these images)
        reach = codec.decoder_reach(B) if B >= 0 else (lambda p0, p1: codec.decoder_cells(p0, p1, 1, True, True))
        for th, tw in ((tile, tile), (tile, 5), (3, tile)):
            grid = codec.tile_grid(h, w, th, tw)
            for rect in _rects(H, W):
                p = codec.region_plan(H, W, F, h, w, th, tw, rect, reach, align=align)
                clipped, rows, cols, tiles, corner = _brute(H, W, h, w, th, tw, rect, reach, align)
                assert (p.rect, p.rows, p.cols, p.tiles) == (clipped, rows, cols, tiles), (H, W, th, tw, rect, B, align)
                y0, x0, wh, ww = p.window
                # the window is cut at the tile grid: its own grid is exactly the plan's tiles, ragged ones included, each where it was
                assert (y0, x0) == (rows[0] * th, cols[0] * tw) and y0 % align == 0 and x0 % align == 0
                assert [(a + y0, b + x0, c, d) for a, b, c, d in codec.tile_grid(wh, ww, th, tw)] == [grid[t] for t in p.tiles]
                assert p.offset == (corner[0] - F * y0, corner[1] - F * x0)
                assert 0 <= p.offset[0] and p.offset[0] + p.rect[3] <= F * wh and 0 <= p.offset[1] and p.offset[1] + p.rect[2] <= F * ww
                if rect[:2] == (0, 0) and rect[2:] == (W, H):
                    assert p.tiles == list(range(len(grid))) and p.window == (0, 0, h, w)


def test_region_plan_of_the_design():
    """the figures of the feature's case: 512 x 512 of a 4K frame at --tile 128 is a window of 7 x 8 tiles of 510"""
    p = codec.region_plan(2160, 3840, 8, 270, 480, 16, 16, (1664, 824, 512, 512), codec.decoder_reach(5))
    assert len(codec.tile_grid(270, 480, 16, 16)) == 510
    assert (p.rows, p.cols, p.window, p.offset) == ((5, 12), (11, 19), (80, 176, 112, 128), (184, 256))
    # the test image of the device tests: 256 x 384 at --tile 64, a 16 x 16 corner needs 3 x 3 of the 4 x 6 tiles
    p = codec.region_plan(256, 384, 8, 32, 48, 8, 8, (0, 0, 16, 16), codec.decoder_reach(5))
    assert p.tiles == [0, 1, 2, 6, 7, 8, 12, 13, 14] and p.window == (0, 0, 24, 24) and p.offset == (0, 0)


def test_region_plan_refusals():
    args = (250, 380, 8, 32, 48, 8, 8)
    reach = codec.decoder_reach(5)
    for rect, why in (((0, 0, 0, 5), 'the extent 0 x 5 is not positive'), ((0, 0, 5, -1), 'is not positive'),
                      ((380, 0, 5, 5), 'does not intersect the 380 x 250 image'), ((0, 250, 5, 5), 'does not intersect'),
                      ((-10, 0, 10, 10), 'does not intersect'), ((1, 2, 3), r'is not \(x, y, w, h\) in pixels'), ('abcd', 'is not')):
        with pytest.raises(ValueError, match=why):
            codec.region_plan(*(args + (rect, reach)))
        if isinstance(rect, tuple) and len(rect) == 4:                        # cap_plane's words
            with pytest.raises(ValueError, match=why):
                codec.cap_plane(250, 380, 8, 4, rois=[rect], background=1)
    with pytest.raises(ValueError, match='does not belong'):
        codec.region_plan(250, 380, 8, 32, 47, 8, 8, (0, 0, 5, 5), reach)
    with pytest.raises(ValueError, match='tile grid'):
        codec.region_plan(250, 380, 8, 32, 48, 0, 8, (0, 0, 5, 5), reach)


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def _shell(golden, model='plain'):
    class _Pred(object):
        freqs_resolution = G.RESOLUTION

        def decode_tiles_batch(self, *a, **kw):
            raise AssertionError('a refused request reached the decoder')
    shell = codec.Codec.__new__(codec.Codec)
    shell.ae_name, shell.pc_name, shell.fingerprint = G.AE, G.PC_OF[model], G.fingerprint(G.weights(model))
    shell.C, shell.L, shell.factor, shell.pred = G.SHAPE[0], 6, G.FACTOR, _Pred()
    shell.wavefront_refusal = shell.layered_refusal = None
    return shell


@pytest.fixture(scope='module')
def golden():
    return G.Golden()


def test_format_1_is_refused_and_names_the_option(golden):
    shell = _shell(golden)
    data = golden.file('plain', 'iid', 1)
    shell.check_container(codec.parse_container(data))
    with pytest.raises(ValueError, match=r'region decode needs tiles: a format-1 file .* write it with --tile'):
        shell.decompress_region(data, (0, 0, 8, 8))
    # behind a request that passes the host checks: the index is the refused one's, and nothing has reached the decoder
    shell.ae = argparse.Namespace(config=argparse.Namespace(arch_param_B=5), decode_family=lambda H, W: (1, 'whole', False))
    with pytest.raises(ValueError, match=r'^request 1: region decode needs tiles.*--tile'):
        shell.decompress_regions_many([(golden.file('plain', 'iid', 4), (0, 0, 67, 50)), (data, (0, 0, 8, 8))])


def test_the_whole_file_is_checked_before_anything_else(golden):
    """a flipped byte, another model, a bad rectangle, bad channels: refused on the host, request by request"""
    shell = _shell(golden)
    shell.ae = argparse.Namespace(config=argparse.Namespace(arch_param_B=5), decode_family=lambda H, W: (1, 'whole', False))
    data = golden.file('plain', 'iid', 4)
    bad = bytearray(data)
    bad[-20] ^= 1
    with pytest.raises(ValueError, match='CRC mismatch'):
        shell.decompress_region(bytes(bad), (0, 0, 8, 8))
    with pytest.raises(ValueError, match='does not intersect the 67 x 50 image'):
        shell.decompress_region(data, (67, 0, 8, 8))
    with pytest.raises(ValueError, match='is not positive'):
        shell.decompress_region(data, (0, 0, 0, 8))
    with pytest.raises(ValueError, match='channels = 33'):
        shell.decompress_region(data, (0, 0, 8, 8), channels=33)
    with pytest.raises(ValueError, match='^request 0: model fingerprint mismatch'):
        shell.decompress_regions_many([(golden.file('sharp', 'iid', 4), (0, 0, 8, 8))])
    with pytest.raises(ValueError, match='^request 1: CRC mismatch'):
        shell.decompress_regions_many([(data, (0, 0, 67, 50)), (bytes(bad), (0, 0, 8, 8))])
    # the plan of a checked request, as Codec.region_plan states it: every tile of this small file (the reach is 18 cells)
    p = shell.region_plan(codec.parse_container(data), (10, 10, 8, 8))
    assert p.tiles == [0, 1, 2, 3] and p.window == (0, 0, 7, 9) and p.offset == (10 + 3, 10 + 2)


def _flags(command, **kw):
    base = dict(command=command, tile=None, checked=False, wavefront=False, salvage=False, channels=None, layers=None, progressive=False,
                front_layers=None, front_progressive=False, partial=False, recover=False, chunk=None, batch=8, region=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_option_clashes():
    codec.check_option_args(_flags('decompress', region='0,0,16,16'))
    codec.check_option_args(_flags('decompress', region='-3,5,16,16', channels=4))
    for flags, why in ((_flags('decompress', region='0,0,16,16', salvage=True), '--region does not go with --salvage'),
                       (_flags('decompress', region='0,0,16,16', partial=True), '--region does not go with --partial'),
                       (_flags('decompress', region='0,0,16,16', recover=True), '--region does not go with --recover'),
                       (_flags('decompress-dir', region='0,0,16,16'), '--region belongs to decompress'),
                       (_flags('compress', region='0,0,16,16'), '--region belongs to decompress'),
                       (_flags('transcode', region='0,0,16,16'), '--region belongs to decompress'),
                       (_flags('stream', region='0,0,16,16'), '--region belongs to decompress'),
                       (_flags('decompress', region='0,0,16'), "--region '0,0,16' is not X,Y,W,H in pixels"),
                       (_flags('decompress', region='0,0,16,0'), r"--region '0,0,16,0': the extent 16 x 0 is not positive")):
        with pytest.raises(ValueError, match=why):
            codec.check_option_args(flags)
    old = argparse.Namespace(command='decompress', tile=None, checked=False, wavefront=False, salvage=True, channels=None)
    codec.check_option_args(old)                                              # a namespace without the key reads as no option


def test_command_line_refuses_before_any_model(tmp_path, capsys):
    src = tmp_path / 'a.icf'
    src.write_bytes(b'x')
    for extra, why in ((['--region', '0,0,8,8', '--salvage'], '--region does not go with --salvage'),
                       (['--region', '0,0,8,8', '--partial'], '--region does not go with --partial'),
                       (['--region', '0,0,8,8', '--recover'], '--region does not go with --recover'),
                       (['--region', '0,0,8'], 'is not X,Y,W,H in pixels')):
        # (a model on the device 'nowhere' could not be built: the refusal comes first)
        assert codec.main(['decompress', str(src), str(tmp_path / 'o.png'), '--device', 'nowhere'] + extra) == 2
        assert why in capsys.readouterr().err
        assert not (tmp_path / 'o.png').exists()


# ---- info -----------------------------------------------------------------------------------------------------------------------

def test_info_on_the_golden_files(golden):
    for fmt in G.FORMATS:
        data = golden.file('plain', 'masked', fmt)
        c = codec.parse_container(data)
        text = codec.info_file(data)
        assert 'format {}, {} bytes'.format(fmt, len(data)) in text and 'image 50 x 67 (H x W), latent 32 x 7 x 9' in text
        assert G.AE in text and '{:08x}'.format(G.fingerprint(G.weights('plain'))) in text
        if fmt == 1:
            assert 'no tiles' in text
            with pytest.raises(ValueError, match='write it with --tile'):
                codec.info_file(data, (0, 0, 8, 8))
            continue
        per_tile = [sum(len(s) for s in b) if fmt in (6, 8) else len(b) for b in c.streams]
        assert 'tiles of 4 x 8 cells, grid 2 x 2 = 4 tiles, last row 3 cells high, last column 1 wide' in text
        assert 'payload {} bytes'.format(len(c.payload)) in text and sum(per_tile) == len(c.payload)
        assert 'bytes per tile: {}'.format(','.join(str(n) for n in per_tile)) in text
        if fmt in (6, 8):
            assert 'layer ends 8,20,32; bytes per layer {}'.format(','.join(str(sum(len(s) for s in layer)) for layer in c.segments)) in text
        else:
            assert 'layer ends' not in text
        assert 'region' not in text
        text = codec.info_file(data, (60, 40, 100, 100))                      # clipped; this small file lies inside any pixel's reach
        assert 'region 60,40,7,10 (reach 131 before, 138 after): tile rows 0 .. 1, columns 0 .. 1, 4 of 4 tiles' in text
        assert 'window 7 x 9 cells at (0, 0), a decoder pass of 56 x 72 pixels of 56 x 72; {0} of {0} payload bytes = 100.0 %'.format(len(c.payload)) in text
        with pytest.raises(ValueError, match='does not intersect the 67 x 50 image'):
            codec.info_file(data, (67, 0, 5, 5))


def test_info_shows_the_plan_of_a_larger_file():
    """a 250 x 380 image at tile 8 x 8 (streams of known lengths: info reads lengths alone): the corner's window is 3 x 3 of 4 x 6 tiles"""
    grid = codec.tile_grid(32, 48, 8, 8)
    streams = [bytes(bytearray([t])) * (10 + t) for t in range(len(grid))]
    data = codec.build_checked_container(G.AE, 'cvpr/res_shallow', 250, 380, 32, 32, 48, 6, 1e9, 0x1234, 8, 8, [0] * len(grid), streams)
    plan = codec.region_plan(250, 380, 8, 32, 48, 8, 8, (0, 0, 16, 16), codec.decoder_reach(5), align=2)
    assert plan.tiles == [0, 1, 2, 6, 7, 8, 12, 13, 14]
    part, total = sum(10 + t for t in plan.tiles), sum(10 + t for t in range(24))
    text = codec.info_file(data, (0, 0, 16, 16))
    assert 'tile rows 0 .. 2, columns 0 .. 2, 9 of 24 tiles' in text
    assert 'window 24 x 24 cells at (0, 0), a decoder pass of 192 x 192 pixels of 256 x 384; {} of {} payload bytes = {:.1f} %'.format(
        part, total, 100.0 * part / total) in text
    assert 'tiles 0,1,2,6,7,8,12,13,14' in text
    # and the wider plan of a picture whose decoder runs F(4x4)
    wide = codec.region_plan(250, 380, 8, 32, 48, 8, 8, (0, 0, 16, 16), lambda p0, p1: codec.decoder_cells(p0, p1, 5, True, True), align=2)
    assert set(plan.tiles) < set(wide.tiles) and len(wide.tiles) < 24
    assert 'region 0,0,16,16 (where the decoder runs its F(4x4) kernels): tile rows {} .. {}, columns {} .. {}, {} of 24 tiles'.format(
        wide.rows[0], wide.rows[1] - 1, wide.cols[0], wide.cols[1] - 1, len(wide.tiles)) in text
    assert 'tiles {}'.format(','.join(str(t) for t in wide.tiles)) in text


def test_info_command(tmp_path, golden):
    """no torch, no model: the command runs with torch unimportable"""
    for fmt in (1, 4, 6):
        (tmp_path / 'f{}.icf'.format(fmt)).write_bytes(golden.file('plain', 'iid', fmt))
    (tmp_path / 'bad.icf').write_bytes(golden.file('plain', 'iid', 4)[:-3])
    block = tmp_path / 'block'
    block.mkdir()
    (block / 'torch.py').write_text("raise ImportError('info must not import torch')\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(block), ROOT] + ([os.environ['PYTHONPATH']] if os.environ.get('PYTHONPATH') else [])))
    run = lambda *args: subprocess.run([sys.executable, '-m', 'imgcomp_cvpr_amd.codec', 'info'] + list(args), cwd=ROOT, env=env,
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    r = run(str(tmp_path / 'f4.icf'), str(tmp_path / 'f6.icf'))
    assert r.returncode == 0 and 'Traceback' not in r.stderr, r.stderr
    assert r.stdout.count('grid 2 x 2 = 4 tiles') == 2 and 'layer ends 8,20,32' in r.stdout and 'region' not in r.stdout
    r = run(str(tmp_path / 'f4.icf'), '--region', '0,0,16,16')
    assert r.returncode == 0 and 'region 0,0,16,16 (reach 131 before, 138 after)' in r.stdout and '4 of 4 tiles' in r.stdout, r.stdout + r.stderr
    r = run(str(tmp_path))                                                    # a directory: every *.icf, the damaged one named, exit 1
    assert r.returncode == 1 and 'bad.icf: ' in r.stdout and 'CRC mismatch' in r.stdout and 'f1.icf: format 1' in r.stdout
    r = run(str(tmp_path / 'f1.icf'), '--region', '0,0,16,16')
    assert r.returncode == 1 and 'write it with --tile' in r.stdout
    r = run(str(tmp_path / 'f4.icf'), '--region', '0,0,16')
    assert r.returncode == 2 and 'is not X,Y,W,H' in r.stderr
