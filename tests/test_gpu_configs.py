"""-m gpu: the BASELINE.json configurations at (or near) their real sizes -- the cases the small parity tests leave out:

  cfg2  Kodak-shaped 512 x 768 image, low + res_shallow: the whole path against the float64 oracle at FULL size in every plan the
        benchmark's step runs (the oracle takes 4 s on the GPU box's host);
  cfg3  ae_configs/cvpr/med + res_shallow, 32 x 3 x 128 x 128 crops, MS-SSIM loss: one training step, forward values and a
        spread of parameter gradients against float64 autograd of the oracle;
  cfg4  --real_bpp on a full Kodak-sized symbol volume (32 x 64 x 96 = 196,608 symbols): the parallel pass feeds the
        arithmetic coder, the on-device sequential decoder reproduces every symbol;
  cfg5  ae_configs/cvpr/hi + pc_configs/cvpr/res_shallow (k = 24, the config BASELINE names): oracle parity at a small
        size and size-independent properties at the full 3840 x 2160 tile (540 x 960 feature map: 15 whole-K rounds + a
        remainder launch, 8.3 M symbols)."""
import numpy as np
import pytest
import torch

from tests.util import assert_close, dev, rel_err, record_flips, NET_RTOL, HEATMAP_RTOL

pytestmark = pytest.mark.gpu


def _nets(cuda, ae_name, pc_name, seed=1234):
    from imgcomp_cvpr_amd import autoencoder, probclass, config_parser as cp, weights as W
    ae_cfg, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', ae_name))
    pc_cfg, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', pc_name))
    wts = W.synthetic_weights(ae_cfg, pc_cfg, seed=seed)
    ae = autoencoder.get_network_cls(ae_cfg)(ae_cfg).load_weights(wts, cuda)
    pc = probclass.get_network_cls(pc_cfg)(pc_cfg, num_centers=ae_cfg.num_centers).load_weights(wts, cuda)
    return ae_cfg, pc_cfg, wts, ae, pc


# (plan, H, W, weight seed, image seed): the four plans on the landscape Kodak shape; the PORTRAIT shape (several of the 24 Kodak images
# are 768 high x 512 wide and val.py:157-158 feeds each at its own shape: 192 x 128 maps = 32 x 48 tiles -> 2 segments per tile row
# instead of 3) in the two F(4x4) schedules; a second draw of synthetic weights, so that one lucky draw is not the whole evidence
CFG2_CASES = [('in_flight', 512, 768, 1234, 0), ('one_at_a_time', 512, 768, 1234, 0), ('f2x2', 512, 768, 1234, 0), ('direct', 512, 768, 1234, 0),
              ('in_flight', 768, 512, 1234, 3), ('one_at_a_time', 768, 512, 1234, 3), ('in_flight', 512, 768, 4321, 5), ('wg8', 768, 512, 4321, 6)]


@pytest.mark.parametrize('plan,H,Wd,wseed,xseed', CFG2_CASES, ids=['{}-{}x{}-w{}'.format(c[0], c[1], c[2], c[3]) for c in CFG2_CASES])
def test_cfg2_kodak_size_matches_oracle_in_every_plan(cuda, plan, H, Wd, wseed, xseed):
    """BASELINE configs[1] at its FULL size (512 x 768 and 768 x 512, low + res_shallow) against the float64 oracle, in the plans the benchmark's step
    runs: with images in flight and one image at a time (F(4x4) for the 64 3x3 layers and for h2 / h12; alone, every launch also
    prefetches the next layer's filter fragments), the F(2x2) plan (IC_CONV3_NO_WINO4: what smaller maps run) and all-direct;
    wg8: the F(4x4) layers with 8-wave work-groups.  z, heatmap, symbols (bit-exact outside the fp32 band of a decision midpoint; measured: no flip at all),
    bit cost, bpp, x_out."""
    from imgcomp_cvpr_amd import bits, weights as W, _lib
    from oracle import oracle as O
    ae_cfg, pc_cfg, wts, ae, pc = _nets(cuda, 'low', 'res_shallow', seed=wseed)
    flags = {'in_flight': _lib.CONV3_IN_FLIGHT(4), 'one_at_a_time': 0, 'f2x2': _lib.CONV3_NO_WINO4, 'direct': _lib.CONV3_DIRECT | _lib.CONV5_NO_WINO4,
             'wg8': _lib.CONV3_IN_FLIGHT(4) | _lib.CONV3_WINO4_WG8}[plan]
    assert _lib.lib.ic_conv3x3_c128_pick_form(1, H // 4, Wd // 4, flags) == {'in_flight': 2, 'one_at_a_time': 2, 'f2x2': 1, 'direct': 0, 'wg8': 2}[plan]
    x = W.synthetic_image((1, 3, H, Wd), 'natural', seed=xseed)
    xd = dev(x, cuda)
    tag = 'cfg2 {}x{}{}'.format(H, Wd, '' if wseed == 1234 else ' weights#{}'.format(wseed))
    torch.set_num_threads(16)
    with torch.no_grad():
        ref = O.encode(torch.as_tensor(x).double(), wts, ae_cfg.as_dict())
        centers = wts['autoencoder/encoder/centers']
        rb, _ = O.bitcost(ref.qhard, ref.symbols, wts, float(centers[0]))
        ref_xo = O.decode(ref.qhard, wts, ae_cfg.as_dict())
    enc = ae.encode(xd, False, plan_flags=flags)
    torch.cuda.synchronize()
    assert_close(enc.z, ref.z, '{} z ({})'.format(tag, plan), NET_RTOL)
    assert_close(enc.heatmap, ref.heatmap, '{} heatmap ({})'.format(tag, plan), HEATMAP_RTOL)
    flips = (enc.symbols.cpu() != ref.symbols).numpy()
    assert record_flips('{} {}'.format(tag, plan), flips) < 2e-3
    q = torch.as_tensor(centers)[ref.symbols].double()
    bc = pc.bitcost(dev(q.numpy(), cuda), dev(ref.symbols.numpy(), cuda, torch.int64), False, pad_value=pc.auto_pad_value(ae))
    assert_close(bc, rb, '{} bit cost ({})'.format(tag, plan), NET_RTOL)
    assert abs(float(bits.bitcost_to_bpp(bc, xd)) - O.bitcost_to_bpp(rb, torch.as_tensor(x))) < 1e-4
    xo = ae.decode(dev(ref.qhard.float().numpy(), cuda), False, plan_flags=flags)
    assert_close(xo, ref_xo, '{} x_out ({})'.format(tag, plan), NET_RTOL)
    if plan == 'wg8':
        # same values in the same order as the 4-wave form: bit-identical through the whole encoder and decoder
        e4 = ae.encode(xd, False, plan_flags=_lib.CONV3_IN_FLIGHT(4))
        assert torch.equal(e4.z, enc.z) and torch.equal(e4.symbols, enc.symbols)
        assert torch.equal(xo, ae.decode(dev(ref.qhard.float().numpy(), cuda), False, plan_flags=_lib.CONV3_IN_FLIGHT(4)))


def test_cfg5_hi_res_shallow_matches_oracle(cuda):
    from imgcomp_cvpr_amd import bits, weights as W
    from oracle import oracle as O
    ae_cfg, pc_cfg, wts, ae, pc = _nets(cuda, 'hi', 'res_shallow', seed=55)
    assert ae_cfg.num_chan_bn == 64 and pc_cfg.arch_param__k == 24
    x = W.synthetic_image((1, 3, 64, 96), 'natural', seed=11)
    xd = dev(x, cuda)
    enc = ae.encode(xd, False)
    ref = O.encode(torch.as_tensor(x).double(), wts, ae_cfg.as_dict())
    assert_close(enc.z, ref.z, 'cfg5 z (hi + res_shallow)', NET_RTOL)
    assert_close(enc.heatmap, ref.heatmap, 'cfg5 heatmap', HEATMAP_RTOL)
    assert record_flips('cfg5 hi + res_shallow', (enc.symbols.cpu() != ref.symbols).numpy()) < 2e-3
    sym = enc.symbols.cpu()
    centers = wts['autoencoder/encoder/centers']
    q = torch.as_tensor(centers)[sym].double()
    bc = pc.bitcost(enc.qbar, enc.symbols, False, pad_value=pc.auto_pad_value(ae))
    rb, _ = O.bitcost(q, sym, wts, float(centers[0]))
    assert_close(bc, rb, 'cfg5 bit cost (k = 24, C = 64)', NET_RTOL)
    assert_close(ae.decode(enc.qhard, False), O.decode(q, wts, ae_cfg.as_dict()), 'cfg5 x_out', NET_RTOL)
    assert abs(float(bits.bitcost_to_bpp(bc, xd)) - O.bitcost_to_bpp(rb, torch.as_tensor(x))) < 1e-4


def test_cfg5_full_4k_tile_properties(cuda):
    """3840 x 2160 with cvpr/hi: the 540 x 960 feature map takes the multi-round launch plan (4050 tile groups).  Determinism,
    finiteness, agreement of the automatic plan with a single forced form on the whole map (bit-identical: same operations
    per output), the direct form within fp32 rounding, batch independence of a crop, and the context model on 8.3 M symbols
    (chunked descriptors: the layer volumes are 0.86 GB each)."""
    import ctypes
    from imgcomp_cvpr_amd import bits, weights as W, _lib
    ae_cfg, pc_cfg, wts, ae, pc = _nets(cuda, 'hi', 'res_shallow', seed=55)
    pl = (ctypes.c_longlong * 5)()
    _lib.check(_lib.lib.ic_wino3x3_c128_plan(1, 540, 960, 0, pl))
    assert sum(pl[i] for i in (0, 1, 3, 4)) == 4050                       # every tile group is covered exactly once
    assert _lib.lib.ic_conv3x3_c128_pick_algo(1, 540, 960, 0) == 1        # 265 MB per image: inside the 31-bit offsets
    assert _lib.lib.ic_conv3x3_c128_pick_algo(1, 2048, 2048, 0) == 0      # 2 GiB: the direct form takes over
    x = dev(W.synthetic_image((1, 3, 2160, 3840), 'natural', seed=2), cuda)
    e1 = ae.encode(x, False)
    z1, s1 = e1.z.clone(), e1.symbols.clone()
    assert tuple(s1.shape) == (1, 64, 270, 480) and bool(torch.isfinite(z1).all())
    e2 = ae.encode(x, False)
    assert torch.equal(z1, e2.z) and torch.equal(s1, e2.symbols), 'encode is not deterministic at 4K'
    # the automatic choice at this size is F(4x4) (4050 work-groups); forcing it changes nothing
    assert _lib.lib.ic_conv3x3_c128_pick_form(1, 540, 960, 0) == 2
    assert torch.equal(z1, ae.encode(x, False, plan_flags=_lib.CONV3_WINO4).z), 'forcing the automatic choice changes the result'
    # the F(2x2) multi-round plan against one forced F(2x2) form: bit-identical (same operations per output)
    e3 = ae.encode(x, False, plan_flags=_lib.CONV3_NO_WINO4)
    assert torch.equal(e3.z, ae.encode(x, False, plan_flags=_lib.CONV3_WINO_WHOLEK).z), 'the launch plan changes the result'
    e4 = ae.encode(x, False, plan_flags=_lib.CONV3_DIRECT)
    # F(4x4) vs F(2x2) vs direct through the whole encoder: fp32 evaluations compared with each other, the maximum over 8.3 M
    # values (the small-size tests bound each of them against float64 at 5e-5; measured in round 3: 6.5e-5 F(2x2) vs direct)
    assert rel_err(e4.z, z1.double()) < 1.5e-4 and rel_err(e3.z, z1.double()) < 1.5e-4 and rel_err(e4.z, e3.z.double()) < 1.5e-4
    xo = ae.decode(e1.qhard, False)
    assert xo.shape == x.shape and float(xo.min()) >= 0 and float(xo.max()) <= 255 and bool(torch.isfinite(xo).all())
    bc = pc.bitcost(e1.qbar, e1.symbols, False, pad_value=pc.auto_pad_value(ae))
    assert bool(torch.isfinite(bc).all()) and float(bc.min()) >= 0
    bpp = float(bits.bitcost_to_bpp(bc, x))
    assert 0.05 < bpp < 8
    # a 256 x 384 crop evaluated alone: the context model is causal and local, so the bit cost of symbols whose 9 x 9 x 5
    # context lies inside the crop's interior does not depend on the rest of the volume
    q_crop = e1.qbar[:, :, 100:132, 200:248].contiguous()
    s_crop = e1.symbols[:, :, 100:132, 200:248].contiguous()
    bc_crop = pc.bitcost(q_crop, s_crop, False, pad_value=pc.auto_pad_value(ae))
    assert torch.equal(bc_crop[:, :, 4:-4, 4:-4], bc[:, :, 104:128, 204:244]), 'blockwise != full volume at 4K'


def test_cfg4_real_bpp_full_kodak_volume(cuda):
    """196,608 symbols of a real encoder output: tables for every position from ONE parallel pass, arithmetic-coded on the
    host (arithmetic_coding.py, the reference coder's bit stream), decoded back on the device symbol by symbol.  The
    README's 350 s + 200 s per image (README.md:65-66) is a few seconds here."""
    import os
    import tempfile
    from imgcomp_cvpr_amd import probclass, bit_counter, weights as W
    ae_cfg, pc_cfg, wts, ae, pc = _nets(cuda, 'low', 'res_shallow')
    x = dev(W.synthetic_image((1, 3, 512, 768), 'natural', seed=4), cuda)
    enc = ae.encode(x, False)
    sym = enc.symbols[0].cpu().numpy()
    assert sym.shape == (32, 64, 96)
    pred = probclass.PredictionNetwork(pc, pc_cfg, ae.get_centers_variable())
    checker = probclass.ProbclassNetworkTesting(pc, ae)
    import time
    torch.cuda.synchronize()
    t0 = time.time()
    # the PRODUCT entry point (val.py --real_bpp -> BppFetcher -> this): it asserts the reference's own run-time invariants
    # at full size -- |coded bits - sum(-log2 p)| < 50 bits ABSOLUTE (bit_counter.py:51), file size == virtual bit count
    # (:56), decoded symbols == input (:68; decoded on the device, symbol by symbol)
    nbits = bit_counter.encode_decode_to_file_ctx(sym, pred, syms_format='CHW')
    torch.cuda.synchronize()
    dt = time.time() - t0
    print('cfg4: encode + on-device decode {:.2f} s = {:.2f} us per symbol'.format(dt, dt / sym.size * 1e6))
    # and against the cross-entropy the fully convolutional pass reports (ProbclassNetworkTesting, val.py:279-281 "up to 1 %"):
    # recorded in the parity report; measured in round 3: 1.4e-6 relative
    bits_theory = checker.get_total_bit_cost(sym)
    assert_close(torch.tensor([float(nbits) / bits_theory]), torch.tensor([1.0], dtype=torch.float64),
                 'cfg4 coded bits / cross-entropy bits, 196,608 symbols', 1e-5)
    print('cfg4: {} symbols, {} bits coded, {:.1f} bits cross-entropy ({:+.4f} %)'.format(sym.size, nbits, bits_theory,
                                                                                        100.0 * (nbits - bits_theory) / bits_theory))


# Bounds ~3 x what the MI355X measured in round 3, per tensor: the error of a gradient grows with the depth of backward it has been
# through (training-mode BatchNorm re-normalises the gradient at every one of the 70 layers), so the encoder's first layers --
# the LAST ones of the backward pass -- carry the accumulated fp32 error of everything behind them.
CFG3_GRAD_RTOL_DEFAULT = 6e-5
CFG3_GRAD_RTOL = {   # measured (gpurun_out/r3d/cfg3.log): 2.3e-3, 1.6e-3, 9.7e-4, 1.0e-3, 5.0e-4, 4.7e-4, 4.7e-4, 1.1e-4, 9.6e-4; the rest <= 1.8e-5
    'autoencoder/encoder/h1/weights': 7e-3, 'autoencoder/encoder/h2/BatchNorm/gamma': 5e-3,
    'autoencoder/encoder/res_block_enc_2/enc_2_2/conv1/weights': 3e-3, 'autoencoder/encoder/to_bn/weights': 3e-3,
    'autoencoder/encoder/centers': 1.5e-3, 'autoencoder/decoder/from_bn/weights': 1.5e-3,
    'autoencoder/decoder/res_block_dec_0/dec_0_1/conv1/weights': 1.5e-3, 'autoencoder/decoder/dec_after_res/conv2/weights': 3.5e-4,
    'autoencoder/decoder/h12/weights': 3e-3}
CFG3_GRAD_RTOL_FLIPS = 5e-2
# The same bounds are asserted of max|ref| itself (no clamp at 1).  One of the fifteen tensors is small enough for that to bite: the
# encoder's last beta has max|ref| = 1.5e-2 and sits behind the same depth of backward as to_bn's filter (3e-3); measured 2.06e-5
# absolute = 1.39e-3 of max|ref| in the F(2x2)-forward run, bound twice that.  Every other tensor keeps its bound above.
CFG3_GRAD_TRUE_RTOL = {'autoencoder/encoder/res_block_enc_final/conv2/BatchNorm/beta': 2.8e-3}


_CFG3_ORACLE = {}


def _cfg3_oracle():
    """the cfg3 batch, its float64 loss and autograd gradients over the oracle (oracle/train_oracle.py) -- once per test process"""
    if not _CFG3_ORACLE:
        from imgcomp_cvpr_amd import config_parser as cp, weights as W
        from oracle import train_oracle as T
        ae, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'med'))
        pc, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
        assert ae.distortion_to_minimize == 'ms_ssim'
        ae.H_target = 0.5                                     # keep the rate term active on synthetic weights
        wts = W.synthetic_weights(ae, pc)
        x = W.synthetic_image((32, 3, 128, 128), 'natural', 7)
        torch.set_num_threads(16)
        total, comps, p = T.train_loss(x, wts, ae.as_dict(), pc.as_dict(), torch.float64)
        total.backward()
        _CFG3_ORACLE.update(ae=ae, pc=pc, wts=wts, x=x, comps=comps, p=p)
    return _CFG3_ORACLE


# The specification bounds OUTPUTS (1e-4 of the tensor scale, symbols bit-exact); it sets no gradient tolerance.  The shipped step runs
# its 3x3 layers in F(4x4) form in both directions (training.wino4_mode): its outputs hold the specification's bounds and its gradients
# are REPORTED against 5 x the per-tensor bounds of the F(2x2)-forward step -- the factor measured in round 5 (1.1 - 4.5 x), not a
# target.  The same step with the forward convolutions in F(2x2) ('bwd': round 5's default) keeps the tight bounds: the backward
# arithmetic itself is what they pin.
@pytest.mark.parametrize('mode', ['shipped', 'f2x2_forward'])
def test_cfg3_training_step_full_size(cuda, mode):
    """32 crops of 128 x 128, cvpr/med, MS-SSIM distortion: the step BASELINE configs[2] names.  Forward values and the
    gradients of a spread of tensors (first / middle / last layers of encoder, decoder and context model, BatchNorm scales,
    centres) against float64 autograd over the oracle (oracle/train_oracle.py)."""
    from imgcomp_cvpr_amd import training
    from tests import util
    o = _cfg3_oracle()
    ae, pc, wts, x, comps, p = o['ae'], o['pc'], o['wts'], o['x'], o['comps'], o['p']
    g = training.TrainGraph(ae, pc, wts, cuda, wino4=None if mode == 'shipped' else 'bwd')
    out = g.forward_backward(dev(x, cuda))
    torch.cuda.synchronize()
    assert g._w3_f4 == ((True, True) if mode == 'shipped' else (False, True)), g._w3_f4
    grad_factor = 5.0 if mode == 'shipped' else 1.0
    label = 'cfg3' if mode == 'shipped' else 'cfg3 [F(2x2) forward]'
    flips = (g.last['symbols'].cpu() != comps['symbols']).numpy()
    rate = record_flips(label + ' training forward', flips)
    assert rate < 2e-3
    assert_close(g.last['z'], comps['z'].detach(), label + ' z (training-mode BN, batch 32)', 1e-4)
    assert abs(out['d_loss_scaled'] - float(comps['d_loss_scaled'])) < 2e-3 * abs(float(comps['d_loss_scaled']))
    assert out['ms_ssim'] is not None and abs(out['ms_ssim'] - (1.0 - float(comps['d_loss_scaled']) / float(ae.K_ms_ssim))) < 2e-4
    names = ['autoencoder/encoder/h1/weights', 'autoencoder/encoder/h2/BatchNorm/gamma',
             'autoencoder/encoder/res_block_enc_2/enc_2_2/conv1/weights', 'autoencoder/encoder/res_block_enc_final/conv2/BatchNorm/beta',
             'autoencoder/encoder/to_bn/weights', 'autoencoder/encoder/centers',
             'autoencoder/decoder/from_bn/weights', 'autoencoder/decoder/res_block_dec_0/dec_0_1/conv1/weights',
             'autoencoder/decoder/dec_after_res/conv2/weights', 'autoencoder/decoder/h12/weights', 'autoencoder/decoder/h13/weights',
             'autoencoder/decoder/h13/BatchNorm/gamma',
             'probclass3d/logits/conv3d_conv0_mask/weights', 'probclass3d/logits/res1/conv3d_conv2_mask/weights',
             'probclass3d/logits/conv3d_conv2_mask/biases']
    # Every gradient is a sum over 32 x 128 x 128 positions (x 70 layers of backward) accumulated in fp32 on the matrix cores,
    # against float64 autograd (the batch-2 32 x 32 step in test_gpu_training.py holds 2e-4 for all 219 tensors).  Every
    # tensor's achieved error goes into the run's parity report with its own bound (CFG3_GRAD_RTOL).  A flipped symbol changes
    # the decoder input by a whole centre distance: with flips the gradients of the two runs are not comparable element-wise,
    # so a run with flips only checks the looser CFG3_GRAD_RTOL_FLIPS (recorded under its own label).
    tag = '' if not flips.any() else ' [with {} symbol flips]'.format(int(flips.sum()))
    bad = []
    for n in names:
        tol = CFG3_GRAD_RTOL_FLIPS if flips.any() else grad_factor * CFG3_GRAD_RTOL.get(n, CFG3_GRAD_RTOL_DEFAULT)
        e, a_ = rel_err(g.grads[n], p[n].grad), util.abs_err(g.grads[n], p[n].grad)
        te = util.true_rel_err(g.grads[n], p[n].grad)          # of max|ref| itself: the same bound, no clamp at 1 (tests/util.py)
        what = '{} grad {}{}'.format(label, n.replace('autoencoder/', 'ae/').replace('probclass3d/logits/', 'pc/'), tag)
        util.REPORT.append((what, a_, e, tol))
        util.SCALES.append((what, util.ref_scale(p[n].grad)))
        ttol = tol if flips.any() or n not in CFG3_GRAD_TRUE_RTOL else grad_factor * CFG3_GRAD_TRUE_RTOL[n]
        if e > tol or te > ttol:
            bad.append('{}: {:.3e} > {:.1e} or {:.3e} of max|ref| > {:.1e}'.format(n, e, tol, te, ttol))
    assert not bad, label + ' gradients outside their bounds (relative to the tensor scale): ' + '; '.join(bad)


def test_cfg1_256_png_through_val(cuda, tmp_path, configs, syn_weights):
    """BASELINE configs[0] at its exact size: ONE 256 x 256 PNG, ae_configs/cvpr/low + pc_configs/cvpr/res_shallow, through the val.py
    entry point (val.py:81-94, :157-158).  The measures.csv row equals the oracle's validate_forward of the same pixels: bpp to
    1e-4, the reconstruction it saves equals the oracle's truncated uint8 output except where the oracle's float64 value sits on an
    integer boundary, and MS-SSIM / PSNR equal the numpy twins of the reference's host metrics evaluated on that saved image."""
    from PIL import Image
    from imgcomp_cvpr_amd import val, metrics, weights as W
    from oracle import oracle as O
    ae_cfg, _ = configs
    imgs = tmp_path / 'one256'
    imgs.mkdir()
    x = W.synthetic_image((1, 3, 256, 256), 'natural', seed=17)
    Image.fromarray(x[0].transpose(1, 2, 0)).save(str(imgs / 'img00.png'))
    root = tmp_path / 'logs'
    (root / '0515_1103 ae_configs@cvpr@low pc_configs@cvpr@res_shallow').mkdir(parents=True)
    val.main([str(root), '0515_1103', str(imgs), '--weights', 'synthetic', '--save_ours', '--in_flight', '1'])
    out = root / '0515_1103 one256'
    rows = (out / 'measures.csv').read_text().strip().split('\n')
    assert rows[0] == 'img_name,bpp,ms-ssim,psnr' and len(rows) == 2
    name, bpp, msssim, psnr = rows[1].split(',')
    torch.set_num_threads(16)
    with torch.no_grad():
        ref = O.validate_forward(x, syn_weights, ae_cfg.as_dict(), torch.float64)
    assert tuple(ref['enc'].symbols.shape) == (1, 32, 32, 32)                     # cfg1: 32,768 symbols
    assert abs(float(bpp) - float(ref['bpp'])) < 1e-4, (bpp, float(ref['bpp']))
    saved = np.asarray(Image.open(str(out / 'imgs' / 'img00.png'))).transpose(2, 0, 1)[None]
    want = ref['x_out_uint8'].numpy()
    diff = saved.astype(np.int32) - want.astype(np.int32)
    frac = ref['x_out'].numpy() - np.floor(ref['x_out'].numpy())
    off = diff != 0
    assert np.abs(diff).max() <= 1 and off.mean() < 1e-4, (int(np.abs(diff).max()), float(off.mean()))
    assert np.all(np.minimum(frac[off], 1 - frac[off]) < 1e-3)                    # only values within 1e-3 of an integer may differ
    assert abs(float(msssim) - metrics.msssim_nchw_uint8(x, saved)) < 1e-5
    assert abs(float(psnr) - metrics.psnr_uint8(x, saved)) < 1e-3
    assert abs(metrics.psnr_uint8(x, saved) - O.psnr_uint8(x, saved)) < 1e-9


def test_cfg5_tiles_sharded_world2(cuda, tmp_path):
    """BASELINE configs[4] as it words it -- "4K tiles, batch sharded across the GPUs": a 3840 x 2160 frame cut into four 1920 x 1080
    tiles (independent images: SURVEY 8(e), the encoder's receptive field forbids halo-free stitching and the reference has no
    tiling), ae_configs/cvpr/hi + res_shallow, evaluated by val.py on one rank and on two ranks (imgcomp_cvpr_amd.sharding:
    round-robin tiles, no data-path collective, one gather of the per-tile scalars; the box has one GPU, so both ranks use cuda:0
    over gloo).  The gathered measures.csv is identical."""
    import os
    import subprocess
    import sys
    from PIL import Image
    from imgcomp_cvpr_amd import val, weights as W
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    frame = W.synthetic_image((1, 3, 2160, 3840), 'natural', seed=3)[0]
    imgs = tmp_path / 'tiles4k'
    imgs.mkdir()
    for ty in range(2):
        for tx in range(2):
            t = frame[:, ty * 1080:(ty + 1) * 1080, tx * 1920:(tx + 1) * 1920].transpose(1, 2, 0)
            Image.fromarray(np.ascontiguousarray(t)).save(str(imgs / 'tile_{}_{}.png'.format(ty, tx)), compress_level=1)
    root = tmp_path / 'logs'
    (root / '0601_0000 ae_configs@cvpr@hi pc_configs@cvpr@res_shallow').mkdir(parents=True)
    val.main([str(root), '0601_0000', str(imgs), '--weights', 'synthetic', '--reset', '--in_flight', '1'])
    out = root / '0601_0000 tiles4k' / 'measures.csv'
    one = out.read_text()
    rows = one.strip().split('\n')
    assert len(rows) == 5 and [r.split(',')[0] for r in rows[1:]] == ['tile_0_0.png', 'tile_0_1.png', 'tile_1_0.png', 'tile_1_1.png']
    assert all(0.01 < float(r.split(',')[1]) < 8 for r in rows[1:])
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', '29583', '-m', 'imgcomp_cvpr_amd.val', str(root), '0601_0000', str(imgs), '--weights', 'synthetic',
           '--reset', '--backend', 'gloo', '--device', 'cuda:0', '--in_flight', '1']
    p = subprocess.run(cmd, cwd=root_dir, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900, universal_newlines=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert out.read_text() == one


def test_pin_reference_end_to_end_on_a_written_bundle(cuda, tmp_path, configs, syn_weights):
    """tools/pin_reference.py, all six steps, on assets made here: the synthetic weights as a TF-1 bundle in the reference's ckpts layout
    (README.md:14-15) and three PNGs.  The per-image rows equal val.py's, the symbol CRCs are those of ae.encode, the run fails when
    the expected means are not met to three decimals and passes when they are."""
    import os
    import pickle
    import sys
    import zlib
    from PIL import Image
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root_dir, 'tools'))
    import pin_reference as P
    from imgcomp_cvpr_amd import tf_checkpoint as T, val, weights as W, autoencoder
    job = '0515_1103 ae_configs@cvpr@low pc_configs@cvpr@res_shallow'
    ck = tmp_path / 'ckpts_root' / job / 'ckpts'
    ck.mkdir(parents=True)
    T.write_bundle(str(ck / 'ckpt-1000'), syn_weights)
    with open(str(ck / 'var_names.pkl'), 'wb') as f:
        pickle.dump([n + ':0' for n in sorted(syn_weights)], f)
    imgs = tmp_path / 'kodak3'
    imgs.mkdir()
    xs = []
    for i, (h, w) in enumerate(((128, 192), (192, 128), (96, 96))):
        x = W.synthetic_image((1, 3, h, w), 'natural', seed=70 + i)
        xs.append(x)
        Image.fromarray(x[0].transpose(1, 2, 0)).save(str(imgs / 'kodim{:02d}.png'.format(i + 1)))
    out = str(tmp_path / 'golden' / 'kodak_test.npz')
    res = P.pin(str(tmp_path / 'ckpts_root'), str(imgs), expect_bpp=None, expect_msssim=None, out=None, verbose=False)
    # README-style expectations, three decimals
    with pytest.raises(P.PinError, match='NOT reproduced: mean bpp'):
        P.pin(str(tmp_path / 'ckpts_root'), str(imgs), expect_bpp=res['mean_bpp'] + 0.002, expect_msssim=res['mean_msssim'], verbose=False)
    again = P.pin(str(tmp_path / 'ckpts_root'), str(imgs), expect_bpp=round(res['mean_bpp'], 3), expect_msssim=round(res['mean_msssim'], 3),
                  out=out, verbose=False)
    assert again['rows'] == res['rows'] and again['symbol_crc32'] == res['symbol_crc32']
    z = np.load(out)
    assert list(z['names']) == ['kodim01.png', 'kodim02.png', 'kodim03.png'] and z['symbol_crc32'].dtype == np.uint32
    # the same rows as the val.py entry point on the same directory (host metrics)
    val.main([str(tmp_path / 'ckpts_root'), '0515_1103', str(imgs), '--reset', '--host_metrics'])
    rows = (tmp_path / 'ckpts_root' / '0515_1103 kodak3' / 'measures.csv').read_text().strip().split('\n')[1:]
    for r, (name, bpp, ms, ps) in zip(rows, res['rows']):
        n2, b2, m2, p2 = r.split(',')
        assert n2 == name and abs(float(b2) - bpp) < 1e-6 and abs(float(m2) - ms) < 1e-9 and abs(float(p2) - ps) < 1e-9
    ae_cfg, _ = configs
    ae = autoencoder.get_network_cls(ae_cfg)(ae_cfg).load_weights(syn_weights, cuda)
    for x, crc in zip(xs, res['symbol_crc32']):
        sym = ae.encode(dev(x, cuda), False).symbols.cpu().numpy().astype(np.int64)
        assert zlib.crc32(np.ascontiguousarray(sym).tobytes()) & 0xffffffff == crc


def test_pinned_kodak_fixture(cuda):
    """Replays tests/golden/kodak_0515_1103.npz (written by tools/pin_reference.py from the reference's published checkpoint and the
    Kodak set) -- the TF-1.4 pin of SURVEY 8(c).  Needs the assets: IMGCOMP_CKPTS_ROOT (extracted ckpts.tar.gz) and IMGCOMP_KODAK
    (directory of the 24 PNGs); neither exists in the build container or on the GPU boxes, where this skips."""
    import os
    import sys
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fixture = os.path.join(root_dir, 'tests', 'golden', 'kodak_0515_1103.npz')
    ck, kodak = os.environ.get('IMGCOMP_CKPTS_ROOT'), os.environ.get('IMGCOMP_KODAK')
    if not (ck and kodak and os.path.isfile(fixture)):
        pytest.skip('needs the 0515_1103 checkpoint, the Kodak images and the fixture pin_reference.py writes from them')
    sys.path.insert(0, os.path.join(root_dir, 'tools'))
    import pin_reference as P
    z = np.load(fixture)
    res = P.pin(ck, kodak, out=None, verbose=False)                      # asserts 0.370 / 0.975 to three decimals itself
    assert [r[0] for r in res['rows']] == list(z['names'])
    assert res['symbol_crc32'] == [int(c) for c in z['symbol_crc32']]    # bit-exact symbols
    assert np.allclose([r[1] for r in res['rows']], z['bpp'], atol=1e-4)
