"""-m gpu: every format through the same calls of one Codec -- what it says it writes, the single-image and the batch calls against
each other both ways, transcode back into the format, measure.  Two pictures of 5 x 7 and 7 x 5 latent cells in tiles of 4 x 4: ragged
right and bottom tiles, all four tile shapes, and two volume shapes for the batch calls to group.  Every comparison is an equality."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = (4, 4)
OPTIONS = {1: dict(tile=None), 2: dict(), 4: dict(checked=True), 5: dict(order='wavefront'), 6: dict(layers='default'),
           8: dict(front_layers='default'), 10: dict(depth_block=4), 12: dict(rans=8)}


@pytest.fixture(scope='module')
def cdc(cuda, configs, syn_weights):
    from imgcomp_cvpr_amd import codec
    return codec.Codec(configs[0], configs[1], syn_weights, cuda)


@pytest.fixture(scope='module')
def images():
    from imgcomp_cvpr_amd import weights as W
    return [np.ascontiguousarray(W.synthetic_image((1, 3, H, W_), 'natural', seed=H)[0].transpose(1, 2, 0)) for H, W_ in ((40, 56), (56, 40))]


def _writes(c, version):
    for name, value in dict(dict(tile=TILE, checked=False, order='raster', layers=None, front_layers=None, depth_block=None, rans=None),
                            **OPTIONS[version]).items():
        setattr(c, name, value)


@pytest.mark.parametrize('version', sorted(OPTIONS))
def test_one_codec_every_call(cdc, images, version):
    from imgcomp_cvpr_amd import codec
    _writes(cdc, version)
    try:
        assert cdc.written_version() == version
        files = [cdc.compress(img) for img in images]
        assert [codec.parse_container(data).version for data in files] == [version, version]
        assert cdc.compress_many(images[:1]) == files[:1]
        assert cdc.compress_many(images) == files
        pictures = [cdc.decompress(data) for data in files]
        many = cdc.decompress_many(files)
        assert len(many) == 2 and all(np.array_equal(a, b) for a, b in zip(many, pictures))
        assert [cdc.transcode(data) for data in files] == files
        assert cdc.measure(images[0], files[0]).bytes == len(files[0])
    finally:
        _writes(cdc, 1)
