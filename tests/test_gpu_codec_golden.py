"""-m gpu: the device against tests/golden/codec_files.npz -- files a past build wrote and the frequency tables it coded them with
(tests/codec_golden_cases.py has the models, volumes and formats, tools/make_codec_golden.py the recipe).  Every other codec test
encodes and decodes with one build in one process and so compares things that move together; here every comparison is an equality
against committed bytes, so a change in the accumulation order of the context-model kernels, in pc_table_row's expression or in the
math library's expf shows as what it is: files written before it no longer decode.  The logits' hash and the tables are separate
tests, so a failure says whether the context model (csrc/probclass.hip, csrc/pc_decode.hip) or the table pass (csrc/pc_table.h)
moved.  Regenerating the fixture to make this file pass is a file-format break.

One comparison is not against the fixture: logits and bit cost of the peaked model `sharp` (and of `k64`, `plain`) against the
float64 oracle at RTOL of tests/util.py -- context-dependent, peaked tables are what a trained model produces, and every other
parity test of the context model runs on near-uniform ones.  The bound is relative to the tensor's scale, max(1, max|oracle|),
which for sharp's logits is SHARP times plain's: the absolute error may grow by that factor, the relative one may not.
Measured on the MI355X that wrote the fixture (HIP 7.0.51831), max error relative to scale, logits / bits, bound 2e-5:
    plain  iid 2.61e-7 / 1.89e-7   masked 2.79e-7 / 1.90e-7
    sharp  iid 2.61e-7 / 2.64e-7   masked 2.79e-7 / 3.36e-7   (absolute: logits 5.2e-6 of up to 20.0, bits 9.0e-6 of up to 29)
    k64    iid 2.89e-7 / 2.17e-7   masked 3.10e-7 / 2.17e-7
sharp's logits carry exactly plain's relative error -- they are plain's times 16, bit for bit.

Sensitivity, shown once on a scratch build: with e[j] * (1.0f / s) for e[j] / s in pc_table_row AND in its restatement in
pc_dec_symbol_wave (csrc/pc_decode.hip), tests/test_gpu_codec.py and tests/test_gpu_codec_decoder.py pass (17 + 17: every path
moved together) and 54 of the 67 tests here fail -- all but the fixture check, the six logits hashes and the six oracle
comparisons.  With the change in pc_table.h alone the two statements disagree, which those two files already catch (6 and 8
failures)."""
import numpy as np
import pytest
import torch

from tests import codec_golden_cases as G
from tests.util import RTOL, assert_close

pytestmark = pytest.mark.gpu
K24_PAIRS = [p for p in G.PAIRS if G.formats_of(p[0]) == G.FORMATS]


@pytest.fixture(scope='module')
def golden():
    return G.Golden()


@pytest.fixture(scope='module')
def codecs(cuda):
    return {m: G.load_codec(m, cuda) for m in G.MODELS}


def _parsed(golden, model, vol, fmt):
    from imgcomp_cvpr_amd import codec
    return codec.parse_container(golden.file(model, vol, fmt))


def _volume_arg(c):
    """a parsed tiled file as decode_tiles_batch takes it"""
    return (c.streams, c.first_syms, (c.C, c.h, c.w))


def _pinned_equal(golden, model, vol, what, got):
    assert G.sha256(got, '<i4') == golden.digest(model, vol, what), \
        '{}/{} {}: the device derives other frequency tables than the build that wrote the golden files'.format(model, vol, what)
    pinned = golden.tables(model, vol, what)
    if pinned is not None:
        assert np.array_equal(got, pinned)


def test_fixture_belongs_to_these_models(golden, codecs):
    print('the fixture was written with HIP {}, this is HIP {}'.format(golden.rocm, torch.version.hip))
    for m, c in codecs.items():
        assert c.fingerprint == golden.fingerprint(m) == G.fingerprint(G.weights(m))
        assert (c.layered_refusal is None and c.wavefront_refusal is None) == (G.formats_of(m) == G.FORMATS)


@pytest.mark.parametrize('model,vol', G.PAIRS)
def test_context_model_logits_are_the_pinned_bits(golden, codecs, model, vol):
    logits = G.device_logits(codecs[model], golden.symbols(model, vol))
    assert logits.shape == (1,) + G.SHAPE + (6,) and bool(torch.isfinite(logits).all())
    assert G.sha256(logits.cpu().numpy(), '<f4') == golden.digest(model, vol, 'logits'), \
        '{}/{}: the context model computes other logit bits than the build that wrote the golden files'.format(model, vol)


@pytest.mark.parametrize('model,vol', G.PAIRS)
def test_frequency_tables_are_the_pinned_integers(golden, codecs, model, vol):
    c, sym = codecs[model], golden.symbols(model, vol)
    _pinned_equal(golden, model, vol, 'tables', G.device_tables(c, sym))
    _pinned_equal(golden, model, vol, 'tile_tables', G.device_tile_tables(c, sym))


def test_table_pass_on_a_second_stream_after_an_unrelated_launch(cuda, golden, codecs):
    """the fixture's premise: the bits do not depend on what ran before or on which stream"""
    c, sym = codecs['sharp'], golden.symbols('sharp', 'iid')
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        a = torch.full((257, 131), 3.0, device=cuda)
        (a @ a.t()).relu_().sum()
        logits = G.device_logits(c, sym)
        tables = G.device_tables(c, sym)
    side.synchronize()
    assert G.sha256(logits.cpu().numpy(), '<f4') == golden.digest('sharp', 'iid', 'logits')
    assert np.array_equal(tables, golden.tables('sharp', 'iid'))


@pytest.mark.parametrize('model,vol', G.PAIRS)
def test_encoder_writes_the_golden_bytes(golden, codecs, model, vol):
    c, sym = codecs[model], golden.symbols(model, vol)
    for fmt in G.formats_of(model):
        assert G.device_file(c, fmt, sym) == golden.file(model, vol, fmt), 'format {}'.format(fmt)
    try:
        c.device_encode = False
        assert G.device_file(c, 1, sym) == golden.file(model, vol, 1), 'format 1 through the host coder'
    finally:
        c.device_encode = True


@pytest.mark.parametrize('model', G.MODELS)
def test_batch_encoder_writes_the_golden_streams(golden, codecs, model):
    """compress_many's path: the tiles of both volumes grouped by shape, one launch per group"""
    pred = codecs[model].pred
    syms = [torch.as_tensor(golden.symbols(model, v)) for v in G.VOLUMES]
    kw = {2: dict(order='raster'), 5: dict(order='wavefront'), 6: dict(layer_ends=list(G.ENDS)), 8: dict(front_ends=list(G.ENDS))}
    for fmt in (f for f in G.formats_of(model) if f in kw):
        coded = pred.encode_tiles_batch(syms, G.TILE[0], G.TILE[1], **kw[fmt])
        for v, per_tile in zip(G.VOLUMES, coded):
            want = _parsed(golden, model, v, fmt)
            assert [f for _, f in per_tile] == want.first_syms and [b for b, _ in per_tile] == want.streams, 'format {} of {}'.format(fmt, v)
    want = [_parsed(golden, model, v, 1) for v in G.VOLUMES]
    assert pred.encode_stream(torch.stack(syms)) == [(w.payload, w.first_sym) for w in want]


@pytest.mark.parametrize('model,vol', G.PAIRS)
def test_decode_symbols_reads_every_golden_file(golden, codecs, model, vol):
    c, sym = codecs[model], golden.symbols(model, vol)
    for fmt in G.formats_of(model):
        got, head = c.decode_symbols(golden.file(model, vol, fmt))
        assert head.version == fmt and np.array_equal(got, sym), 'format {}'.format(fmt)


@pytest.mark.parametrize('model,vol', G.PAIRS)
def test_serial_decoders_read_the_golden_stream(golden, codecs, model, vol):
    from imgcomp_cvpr_amd import _lib
    c, sym, head = codecs[model], golden.symbols(model, vol), _parsed(golden, model, vol, 1)
    for flags in (0, _lib.PC_DECODE_RECOMPUTE, _lib.PC_DECODE_PER_LAYER):
        assert np.array_equal(c.pred.decode_stream(head.payload, G.SHAPE, head.first_sym, flags=flags), sym), 'flags {}'.format(flags)


@pytest.mark.parametrize('model,vol', G.PAIRS)
def test_tile_decoders_read_the_golden_streams(golden, codecs, model, vol):
    c, sym = codecs[model], golden.symbols(model, vol)
    centers = c.pred.centers.float()
    for fmt in (2, 4):
        head = _parsed(golden, model, vol, fmt)
        assert np.array_equal(c.pred.decode_tiles(head.streams, head.first_syms, G.SHAPE, head.th, head.tw), sym), 'format {}'.format(fmt)
        (q, s), = c.pred.decode_tiles_batch([_volume_arg(head)], head.th, head.tw, want='both')
        assert np.array_equal(s.cpu().numpy(), sym), 'format {}'.format(fmt)
        assert torch.equal(q, centers[torch.as_tensor(sym).to(q.device)]), 'format {}: q is not centres[symbols]'.format(fmt)


@pytest.mark.parametrize('model', sorted({m for m, _ in K24_PAIRS}))
def test_batch_entry_reads_the_wavefront_and_layered_golden_files(golden, codecs, model):
    """formats 5, 6 and 8 through decode_tiles_batch, both volumes of the model in one call"""
    from imgcomp_cvpr_amd.codec import _ends_kw
    c = codecs[model]
    centers = c.pred.centers.float()
    for fmt in (5, 6, 8):
        heads = [_parsed(golden, model, v, fmt) for v in G.VOLUMES]
        kw = dict(order='wavefront') if fmt == 5 else _ends_kw(heads[0])
        both = c.pred.decode_tiles_batch([_volume_arg(h) for h in heads], G.TILE[0], G.TILE[1], want='both', **kw)
        for v, (q, s) in zip(G.VOLUMES, both):
            sym = golden.symbols(model, v)
            assert np.array_equal(s.cpu().numpy(), sym), 'format {} of {}'.format(fmt, v)
            assert torch.equal(q, centers[torch.as_tensor(sym).to(q.device)]), 'format {} of {}: q is not centres[symbols]'.format(fmt, v)


@pytest.mark.parametrize('model,vol', K24_PAIRS)
@pytest.mark.parametrize('fmt', [6, 8])
def test_layer_prefixes_decode_as_previews(golden, codecs, model, vol, fmt):
    """decompress_partial's symbol path on the prefix that ends with each layer"""
    from imgcomp_cvpr_amd import codec
    c, sym, data = codecs[model], golden.symbols(model, vol), golden.file(model, vol, fmt)
    fill = codec.fill_symbol(c.pred.centers.cpu().numpy())
    assert fill == c.pred.conceal_fallback()
    for g, e_g in enumerate(G.ENDS):
        prefix = data[:codec.layer_prefix_bytes(data, g + 1)]
        head, complete, _ = codec.parse_partial(prefix)
        c.check_container(head)
        assert complete == g + 1 and head.layer_ends[complete - 1] == e_g
        got = c.pred.decode_tiles_batch([_volume_arg(head)], head.th, head.tw, want='symbols', channels=e_g, **codec._ends_kw(head))[0]
        assert np.array_equal(got.cpu().numpy(), codec.preview_symbols(sym, e_g, fill)), 'layer {}'.format(g)
    img, report = c.decompress_partial(data[:codec.layer_prefix_bytes(data, 1)])
    assert report == codec.PartialReport(3, 1, G.ENDS[0], False)
    assert np.array_equal(img, c._image(codec.preview_symbols(sym, G.ENDS[0], fill), head))


@pytest.mark.parametrize('model,vol', K24_PAIRS)
def test_stream_decoder_reads_the_front_layered_golden_file(golden, codecs, model, vol):
    """format 8 through StreamDecoder(fronts=True), 64 bytes a feed, a picture whenever a tile has gained a layer"""
    c, sym, data = codecs[model], golden.symbols(model, vol), golden.file(model, vol, 8)
    head = _parsed(golden, model, vol, 8)
    sd = c.open_stream(fronts=True)
    seen, pictures = (), 0
    for pos in range(0, len(data), 64):
        if sd.feed(data[pos:pos + 64]) and sd.progress() != seen and any(sd.progress()):
            seen = sd.progress()
            img, report = sd.image()
            pictures += 1
    assert sd.bytes_fed == len(data) and seen == (3, 3, 3, 3) and pictures >= 3
    assert report.tiles == [] and report.file_crc_ok and (report.ntiles, report.layers_total) == (4, 3)
    assert np.array_equal(img, c._image(sym, head))


@pytest.mark.parametrize('model,vol', G.PAIRS)
def test_salvage_of_an_undamaged_golden_file_reports_no_damage(golden, codecs, model, vol):
    c, sym, data = codecs[model], golden.symbols(model, vol), golden.file(model, vol, 4)
    img, report = c.salvage(data)
    assert report.damaged == [] and report.file_crc_ok and report.ntiles == 4
    assert np.array_equal(img, c._image(sym, _parsed(golden, model, vol, 4)))


@pytest.mark.parametrize('model,vol', G.PAIRS)
def test_peaked_tables_against_the_float64_oracle(golden, codecs, model, vol):
    """logits and bit cost against oracle.bitcost in float64, on the volume padded as the codec pads it (symbol 0's centre)"""
    from oracle import oracle as O
    c, sym = codecs[model], golden.symbols(model, vol)
    wts = G.weights(model)
    centers = G.centers(wts)
    s = torch.as_tensor(sym)[None]
    ref_bits, ref_logits = O.bitcost(torch.as_tensor(centers)[s].double(), s, wts, float(centers[0]))
    logits = G.device_logits(c, sym)
    sd = s.to(c.device)
    bits = c.pc.bitcost(c.pred.centers.float()[sd].contiguous(), sd, False, pad_value=float(centers[0]))
    what = '{}/{} shape {}'.format(model, vol, G.SHAPE)
    print('{}: max |logit| {:.3f}, max bits {:.3f}'.format(what, float(ref_logits.abs().max()), float(ref_bits.max())))
    e_l = assert_close(logits, ref_logits, 'codec golden logits ' + what, rtol=RTOL)
    e_b = assert_close(bits, ref_bits, 'codec golden bits ' + what, rtol=RTOL)
    print('{}: logits {:.3e}, bits {:.3e} relative to scale (bound {:.1e})'.format(what, e_l, e_b, RTOL))
