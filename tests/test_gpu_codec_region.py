"""-m gpu: region decode -- Codec.decompress_region / decompress_regions_many.  The contract is an equality of pixels: a rectangle
decoded from the tiles it needs is the crop of decompress, bit for bit, in every tiled format, with and without --channels, whatever
kernel form the window alone would have been given."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE, ENDS = (8, 8), [4, 8, 16, 32]            # --tile 64: a 256 x 384 picture is 32 x 48 cells, 4 x 6 tiles
FORMATS = {2: dict(tile=TILE), 4: dict(tile=TILE, checked=True), 5: dict(tile=TILE, order='wavefront'),
           6: dict(tile=TILE, layers=ENDS), 8: dict(tile=TILE, front_layers=ENDS)}
# (x, y, w, h) -> the tile rows and columns region_plan names (B = 5: 131 pixels before, 138 after)
RECTS = {(256, 384): {'corner': ((0, 0, 16, 16), (0, 3), (0, 3)), 'edge': ((210, 0, 16, 16), (0, 3), (1, 6)),
                      'interior': ((210, 120, 16, 16), (0, 4), (1, 6)), 'far corner': ((368, 240, 16, 16), (1, 4), (3, 6)),
                      'wide': ((100, 8, 200, 30), (0, 3), (0, 6))},
         # 250 x 380 is padded by 3 + 3 rows and 2 + 2 columns: the rectangle at its end reaches the last cells
         (250, 380): {'corner': ((0, 0, 16, 16), (0, 3), (0, 3)), 'ragged end': ((364, 234, 16, 16), (1, 4), (3, 6)),
                      'poking out': ((-8, 240, 30, 40), (1, 4), (0, 3))}}


def _picture(h, w, seed):
    from imgcomp_cvpr_amd import weights as W_
    return np.ascontiguousarray(np.transpose(W_.synthetic_image((1, 3, h, w), 'natural', seed=seed)[0], (1, 2, 0)))


def _set(c, kw):
    c.tile, c.checked, c.order = kw.get('tile'), kw.get('checked', False), kw.get('order', 'raster')
    c.layers, c.front_layers = kw.get('layers'), kw.get('front_layers')
    return c


@pytest.fixture(scope='module')
def cdc(cuda, configs, syn_weights):
    from imgcomp_cvpr_amd import codec
    c = codec.Codec(configs[0], configs[1], syn_weights, cuda)
    assert (c.C, c.L, c.factor) == (32, 6, 8) and codec.decoder_reach(configs[0].arch_param_B) == (131, 138)
    yield c
    _set(c, {})


class _Files(object):
    """every file written once per module, every whole picture decoded once: the reference of all the crops, never changed"""

    def __init__(self, cdc):
        self.cdc, self.files, self.whole = cdc, {}, {}

    def file(self, size, fmt, **kw):
        key = (size, fmt) + tuple(sorted(kw.items()))
        if key not in self.files:
            self.files[key] = _set(self.cdc, dict(FORMATS[fmt], **kw)).compress(_picture(size[0], size[1], 11))
            _set(self.cdc, {})
        return self.files[key]

    def picture(self, data, channels=None):
        key = (data, channels)
        if key not in self.whole:
            self.whole[key] = self.cdc.decompress(data, channels=channels)
            self.whole[key].setflags(write=False)
        return self.whole[key]

    def crop(self, data, rect, channels=None):
        img = self.picture(data, channels)
        x0, y0, x1, y1 = max(rect[0], 0), max(rect[1], 0), min(rect[0] + rect[2], img.shape[1]), min(rect[1] + rect[3], img.shape[0])
        return img[y0:y1, x0:x1]


@pytest.fixture(scope='module')
def files(cdc):
    return _Files(cdc)


class _Recorder(object):
    """pred.decode_tiles_batch wrapped: the volumes of every call"""

    def __init__(self, monkeypatch, cdc):
        self.calls, inner = [], cdc.pred.decode_tiles_batch

        def wrapped(volumes, *a, **kw):
            self.calls.append([(list(s), list(f), tuple(int(v) for v in shape)) for s, f, shape in volumes])
            return inner(volumes, *a, **kw)
        monkeypatch.setattr(cdc.pred, 'decode_tiles_batch', wrapped)


# ---- the pixels -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('fmt', sorted(FORMATS))
def test_region_is_the_crop_of_the_whole_picture(cdc, files, fmt):
    from imgcomp_cvpr_amd import codec
    from tests import fenced as Fz
    for size, rects in sorted(RECTS.items()):
        data = files.file(size, fmt)
        c = codec.parse_container(data)
        assert c.version == fmt and (c.h, c.w, c.th, c.tw) == (32, 48, 8, 8)
        for name, (rect, rows, cols) in sorted(rects.items()):
            plan = cdc.region_plan(c, rect)
            assert (plan.rows, plan.cols) == (rows, cols) and len(plan.tiles) < 24, (size, name)
            if fmt == 4:                                                      # before the cast too: the cast hides most of a rounding difference
                whole, forced, _ = _floats(cdc, c, plan, cdc.ae.plan_like(256, 384))
                assert Fz.same_bits(forced, whole), '{} {}: {} values differ before the cast'.format(size, name, int((forced != whole).sum()))
            for channels in (None, 4):
                got = cdc.decompress_region(data, rect, channels=channels)
                want = files.crop(data, rect, channels)
                assert got.dtype == np.uint8 and got.shape == want.shape == (plan.rect[3], plan.rect[2], 3) and got.flags['C_CONTIGUOUS']
                assert np.array_equal(got, want), 'format {} {} {} channels {}: {} pixels differ'.format(
                    fmt, size, name, channels, int((got != want).any(axis=2).sum()))
        whole = cdc.decompress_region(data, (-5, -5, 1000, 1000))              # clipped to the image: the decompress path itself
        assert np.array_equal(whole, files.picture(data))
    assert not np.array_equal(files.picture(data), files.picture(data, 4))    # (the preview is another picture)


@pytest.mark.parametrize('fmt', [2, 6])
def test_the_decoder_gets_the_tiles_of_the_plan_and_no_others(cdc, files, fmt, monkeypatch):
    from imgcomp_cvpr_amd import codec
    rec = _Recorder(monkeypatch, cdc)
    for size, rects in sorted(RECTS.items()):
        data = files.file(size, fmt)
        c = codec.parse_container(data)
        for name, (rect, _, _) in sorted(rects.items()):
            del rec.calls[:]
            cdc.decompress_region(data, rect)
            plan = codec.region_plan(c.H, c.W, 8, c.h, c.w, c.th, c.tw, rect, codec.decoder_reach(5))
            assert len(rec.calls) == 1 and len(rec.calls[0]) == 1, (size, name)
            streams, firsts, shape = rec.calls[0][0]
            assert streams == [c.streams[t] for t in plan.tiles] and firsts == [c.first_syms[t] for t in plan.tiles]
            assert shape == (32, plan.window[2], plan.window[3])
            assert set(plan.tiles) < set(range(len(c.streams)))               # a strict subset
        del rec.calls[:]
        cdc.decompress_region(data, (0, 0, c.W, c.H))                         # the whole image: every tile, by decompress's own path
        assert sum(len(v[0]) for call in rec.calls for v in call) in (0, len(c.streams))


# ---- the kernel form is the whole picture's ----------------------------------------------------------------------------------------

def test_window_and_picture_would_pick_different_forms(cdc, files):
    """512 x 768 at --tile 128: the picture's 3 x 3 layers run F(4x4) (192 work-groups), a corner's window of 384 x 384 alone would
    run F(2x2) (72), and h12 changes kernels with them.  Forced, the window gives the picture's values bit for bit before the cast
    to uint8; left to itself it does not -- how many values differ, before and after the cast, is printed.  The window is the
    F(4x4) kernels' (decoder_cells): 3 x 3 tiles where the arithmetic's reach asks for 2 x 2."""
    import torch
    from imgcomp_cvpr_amd import _lib, codec
    from tests import fenced as Fz
    data = files.file((512, 768), 4, tile=(16, 16))
    c = codec.parse_container(data)
    flags = cdc.ae._abi_flags(cdc.ae.plan_flags)
    assert int(_lib.lib.ic_conv3x3_c128_pick_form(1, 128, 192, flags)) == 2
    assert cdc.ae.decode_family(512, 768) == (2, None, True)
    for rect, window in (((0, 0, 16, 16), (0, 0, 48, 48)), ((752, 496, 16, 16), (16, 48, 48, 48)), ((0, 0, 200, 16), (0, 0, 48, 64))):
        plan = cdc.region_plan(c, rect)
        assert plan.window == window
        narrow = codec.region_plan(c.H, c.W, 8, c.h, c.w, c.th, c.tw, rect, codec.decoder_reach(5), align=2)
        assert set(narrow.tiles) < set(plan.tiles) < set(range(len(c.streams)))
        assert int(_lib.lib.ic_conv3x3_c128_pick_form(1, 4 * window[2] // 2, 4 * window[3] // 2, flags)) == 1
        bits = cdc.ae.plan_like(512, 768)
        assert bits & _lib.CONV3_FORM_MASK == _lib.CONV3_WINO4 and bits & _lib.CONV5_WINO4
        assert cdc.ae.plan_holds(bits, 512, 768, 8 * window[2], 8 * window[3], 8 * window[0], 8 * window[1])
        got = cdc.decompress_region(data, rect)
        want = files.crop(data, rect)
        assert np.array_equal(got, want), '{}: {} pixels differ'.format(rect, int((got != want).any(axis=2).sum()))
        # the same window with and without the forced plan, before the cast: every value of the window that lies inside the reach
        # of no cell outside it -- the rectangle -- is the picture's float, bit for bit, only when forced
        whole, forced, free = _floats(cdc, c, plan, bits)
        assert Fz.same_bits(forced, whole), '{}: {} values differ'.format(rect, int((forced != whole).sum()))
        assert not Fz.same_bits(free, whole), 'the window alone ran the kernels of the picture: this shape shows nothing'
        # and the window of the arithmetic's reach under the forced plan: what the F(4x4) transforms carry in from beyond it
        _, short, _ = _floats(cdc, c, narrow, bits)
        print('rectangle {} of 512 x 768: from the {} tiles of the arithmetic\'s reach, forced plan, {} of {} values differ before the cast'.format(
            rect, len(narrow.tiles), int((short != whole).sum()), whole.numel()))
        cast = lambda t: t.to(torch.uint8)
        print('rectangle {} of 512 x 768, window {}: without the forced plan {} of {} values differ from the picture\'s before the cast, by up to '
              '{:.3e} of 255, and {} after it'.format(rect, window, int((free != whole).sum()), whole.numel(), float((free - whole).abs().max()),
                                                       int((cast(free) != cast(whole)).sum())))


def _floats(cdc, c, plan, bits):
    """the rectangle of plan before the cast to uint8: from the whole picture, from the window with the forced plan, from the
    window left to itself -> three (3, h, w) float32 device tensors"""
    volume = lambda tiles, h, w: [([c.streams[t] for t in tiles], [c.first_syms[t] for t in tiles], (32, h, w))]
    q_all = cdc.pred.decode_tiles_batch(volume(range(len(c.streams)), c.h, c.w), c.th, c.tw, want='q')[0]
    q_win = cdc.pred.decode_tiles_batch(volume(plan.tiles, plan.window[2], plan.window[3]), c.th, c.tw, want='q')[0]
    (x, y, rw, rh), (oy, ox) = plan.rect, plan.offset
    top, left = ((-c.H) % 8) // 2, ((-c.W) % 8) // 2
    whole = cdc.ae.decode(q_all[None], is_training=False)[0, :, y + top:y + top + rh, x + left:x + left + rw].clone()
    forced = cdc.ae.decode(q_win[None], is_training=False, plan_flags=bits)[0, :, oy:oy + rh, ox:ox + rw].clone()
    free = cdc.ae.decode(q_win[None], is_training=False)[0, :, oy:oy + rh, ox:ox + rw].clone()
    return whole, forced, free


def test_a_width_the_f4_kernels_do_not_take(cdc, files):
    """256 x 376: 47 cells, 94 positions at H/4 -- no multiple of 4, so the picture runs F(2x2), and so does every window, the one
    with the ragged, odd last column included"""
    from imgcomp_cvpr_amd import _lib, codec
    from tests import fenced as Fz
    data = files.file((256, 376), 5)
    c = codec.parse_container(data)
    assert (c.h, c.w) == (32, 47) and int(_lib.lib.ic_conv3x3_c128_pick_form(1, 64, 94, cdc.ae._abi_flags(0))) == 1
    bits = cdc.ae.plan_like(256, 376)
    assert bits & _lib.CONV3_FORM_MASK == _lib.CONV3_WINO_WHOLEK and bits & _lib.CONV5_NO_WINO4
    for rect, window in (((0, 0, 16, 16), (0, 0, 24, 24)), ((360, 240, 16, 16), (8, 24, 24, 23))):
        assert cdc.region_plan(c, rect).window == window
        assert cdc.ae.plan_holds(bits, 256, 376, 8 * window[2], 8 * window[3], 8 * window[0], 8 * window[1])
        whole, forced, _ = _floats(cdc, c, cdc.region_plan(c, rect), bits)
        assert Fz.same_bits(forced, whole), '{}: {} values differ before the cast'.format(rect, int((forced != whole).sum()))
        for channels in (None, 4):
            assert np.array_equal(cdc.decompress_region(data, rect, channels=channels), files.crop(data, rect, channels)), (rect, channels)


def test_a_window_that_cannot_have_the_form_widens_to_the_picture(cdc, files, monkeypatch):
    """an F(4x4) picture cut into tiles 15 cells wide: a window of three tile columns is 45 cells, 90 positions at H/4, which the
    F(4x4) kernels do not take -- the whole picture is decoded and cropped, the pixels are the same"""
    from imgcomp_cvpr_amd import codec
    from tests import fenced as Fz
    data = files.file((512, 768), 5, tile=(16, 15))
    c = codec.parse_container(data)
    rect = (0, 0, 16, 16)
    plan = cdc.region_plan(c, rect)
    assert plan.window == (0, 0, 48, 45) and len(plan.tiles) == 9 < len(c.streams) == 28
    assert not cdc.ae.plan_holds(cdc.ae.plan_like(512, 768), 512, 768, 384, 360, 0, 0)
    rec = _Recorder(monkeypatch, cdc)
    got = cdc.decompress_region(data, rect)
    assert [len(v[0]) for call in rec.calls for v in call] == [len(c.streams)]
    assert np.array_equal(got, files.crop(data, rect))
    # an odd first cell is moved to an even one (align = 2), a tile column further out: the window keeps the picture's F(4x4) tiles
    rect = (680, 0, 16, 16)
    plan = cdc.region_plan(c, rect)
    free = codec.region_plan(c.H, c.W, 8, c.h, c.w, c.th, c.tw, rect, lambda p0, p1: codec.decoder_cells(p0, p1, 5, True, True))
    assert free.cols == (3, 7) and plan.cols == (2, 7) and plan.window == (0, 30, 48, 66)
    bits = cdc.ae.plan_like(512, 768)
    assert cdc.ae.plan_holds(bits, 512, 768, 384, 528, 0, 240) and not cdc.ae.plan_holds(bits, 512, 768, 384, 408, 0, 360)
    del rec.calls[:]
    got = cdc.decompress_region(data, rect)
    assert [len(v[0]) for call in rec.calls for v in call] == [len(plan.tiles)]
    assert np.array_equal(got, files.crop(data, rect))
    whole, forced, _ = _floats(cdc, c, plan, bits)
    assert Fz.same_bits(forced, whole), '{} values differ before the cast'.format(int((forced != whole).sum()))


# ---- nothing outside the window is read --------------------------------------------------------------------------------------------

def test_the_decoder_pass_reads_the_window_alone(cdc, files, cuda):
    import torch
    from imgcomp_cvpr_amd import codec
    from tests import fenced as Fz
    for size, fmt, kw, rect in (((256, 384), 4, {}, (368, 240, 16, 16)), ((512, 768), 4, dict(tile=(16, 16)), (0, 0, 16, 16))):
        data = files.file(size, fmt, **kw)
        c = codec.parse_container(data)
        plan = cdc.region_plan(c, rect)
        bits = cdc.ae.plan_like(c.h * 8, c.w * 8)
        q = cdc.pred.decode_tiles_batch([([c.streams[t] for t in plan.tiles], [c.first_syms[t] for t in plan.tiles], (32,) + plan.window[2:])],
                                        c.th, c.tw, want='q')[0]
        qf = Fz.fenced(q, torch.float32, device=cuda, fill=Fz.IN_FENCE, name='q of the window')
        x0 = cdc.ae.decode(q[None], is_training=False, plan_flags=bits)
        x1 = cdc.ae.decode(qf[None], is_training=False, plan_flags=bits)
        torch.cuda.synchronize()
        assert qf[None].data_ptr() == qf.data_ptr()
        assert bool(torch.isfinite(x1).all()) and Fz.same_bits(x0, x1)
        Fz.check_fences(qf)
        got = np.transpose(cdc._window_pixels(cdc.ae, qf, plan, bits).cpu().numpy(), (1, 2, 0))
        assert np.array_equal(got, files.crop(data, rect))


# ---- a batch of requests ----------------------------------------------------------------------------------------------------------

def test_regions_many(cdc, files, monkeypatch):
    a, b, l = files.file((256, 384), 4), files.file((250, 380), 4), files.file((256, 384), 6)
    requests = [(a, (0, 0, 16, 16)), (l, (210, 0, 16, 16)), (b, (364, 234, 16, 16)), (a, (368, 240, 16, 16)), (a, (0, 0, 384, 256)),
                (l, (0, 0, 16, 16)), (b, (-8, 240, 30, 40)), (a, (0, 0, 16, 16))]
    rec = _Recorder(monkeypatch, cdc)
    got = cdc.decompress_regions_many(requests)
    # one call per group -- the raster files of both sizes together, the layered file -- not one per request
    assert sorted(len(call) for call in rec.calls) == [2, 6]
    assert sorted(len(v[0]) for call in rec.calls for v in call) == [9, 9, 9, 9, 9, 9, 15, 24]
    assert len(got) == len(requests)
    for i, (data, rect) in enumerate(requests):
        one = cdc.decompress_region(data, rect)
        assert np.array_equal(got[i], one) and np.array_equal(one, files.crop(data, rect)), i
    assert np.array_equal(got[0], got[7])
    preview = cdc.decompress_regions_many(requests[:3], channels=4)
    for i, (data, rect) in enumerate(requests[:3]):
        assert np.array_equal(preview[i], files.crop(data, rect, 4)), i
    # a small workspace cuts the tile list into chunks: the same pixels
    small = cdc.decompress_regions_many(requests[:4], max_workspace_bytes=1 << 26)
    assert all(np.array_equal(x, y) for x, y in zip(small, got[:4]))
    assert cdc.decompress_regions_many([]) == []


# ---- the whole file is checked --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('fmt', [2, 4, 6])
def test_damage_outside_the_window_is_still_refused(cdc, files, fmt, monkeypatch):
    from imgcomp_cvpr_amd import codec
    data = files.file((256, 384), fmt)
    c = codec.parse_container(data)
    rect = (0, 0, 16, 16)
    assert 23 not in cdc.region_plan(c, rect).tiles
    bad = bytearray(data)
    bad[-5] ^= 0x10                                                           # the last byte of the last tile's stream (last layer)
    assert bytes(bad[:-4]).endswith(bytes(bytearray([(c.streams[23][-1] if fmt == 6 else c.streams[23])[-1] ^ 0x10])))
    rec = _Recorder(monkeypatch, cdc)
    with pytest.raises(ValueError, match='CRC'):
        cdc.decompress_region(bytes(bad), rect)
    with pytest.raises(ValueError, match='^request 1: .*CRC'):
        cdc.decompress_regions_many([(data, rect), (bytes(bad), rect)])
    assert rec.calls == []                                                    # nothing has reached the device
    with pytest.raises(ValueError, match='--tile'):
        cdc.decompress_region(_set(cdc, {}).compress(_picture(64, 64, 3)), rect)
