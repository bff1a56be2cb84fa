"""tests/config_cases.py is what tests/test_gpu_config_space.py takes it for (no GPU: the oracle on the CPU in float32 and float64,
and the host side of the library).  The conditions are conditions on the oracle, the variables and the table -- they keep the GPU
comparisons from passing vacuously (an x_out pinned to the clip's edges, all symbols in one bin): a case that misses one gets
another seed (the next that passes), never a weaker condition."""
import numpy as np
import pytest
import torch

from tests import config_cases as K
from tests import step_cases as S
from tests.util import NET_RTOL, _boundary_margin, rel_err

MAX_EDGE_SHARE = 0.01          # of x_out on 0 or 255
MIN_SYMBOL_SHARE = 0.05        # at least two symbols hold this much of the volume each
# A TRAINING step's x_out is another matter: BatchNorm with batch statistics standardises h13's output, so x_out's channel c is
# gamma_c s n + (beta_c s + m) with n of zero mean and unit variance whatever the variables -- with gamma up to 1.5 and s = 68 the
# edges 0 and 255 sit 1.2 standard deviations from the mean in the widest channel, under FIXED and OFF alike.  Some clipped elements
# are wanted there (the clip is one of the step's forced decisions); what must not happen is that most of x_out is pinned.
STEP_MAX_EDGE_SHARE = 0.10


def _non_degenerate(label, x_out, symbols, L, max_edge_share=MAX_EDGE_SHARE):
    edge, shares = K.edge_share(x_out), K.symbol_shares(symbols, L)
    print('{}: x_out {:.1f} .. {:.1f}, on the clip\'s edges {:.4f}; symbol shares {}'.format(
        label, float(x_out.min()), float(x_out.max()), edge, np.round(shares, 3).tolist()))
    assert edge <= max_edge_share, (label, edge)
    assert int((shares >= MIN_SYMBOL_SHARE).sum()) >= 2, (label, shares)


def test_table_is_what_it_claims():
    """the overrides parse under the config grammar's constraints, the sizes are the table's, and each case reaches the dispatch
    branch it is there for (restated from csrc/conv_mfma.hip and csrc/conv_direct.hip by the library's host queries)"""
    from imgcomp_cvpr_amd import _lib as L, weights as W
    assert [c.id for c in K.TABLE] == ['norm_off', 'c16_b1_l8', 'c8_b0_l2_nohm', 'c96_b3_l16', 'c48_b3_nohm', 'base_c192_b3']
    assert [sc.id for sc in K.STEP_CASES] == ['norm_off', 'c16_b1_l8', 'c8_b0_l2_nohm', 'c96_b3_l16']
    for c in K.TABLE:
        sc = K.case(c)
        ae, pc = S.configs(sc)
        assert (ae.normalization, ae.num_chan_bn, ae.arch_param_B, ae.num_centers, bool(ae.heatmap)) == (c.normalization, c.C, c.B, c.L, c.heatmap)
        assert ae.arch == 'CVPR' and ae.H_target == 0.5 and ae.distortion_to_minimize == 'mse'
        assert c.to_bn == c.C + int(c.heatmap)
        w = S.weights(sc)
        assert w['autoencoder/encoder/to_bn/weights'].shape == (5, 5, 128, c.to_bn)
        assert w['autoencoder/decoder/from_bn/weights'].shape == (3, 3, 128, c.C)
        assert w['autoencoder/encoder/centers'].shape == (c.L,) and w['probclass3d/logits/conv3d_conv2_mask/weights'].shape[-1] == c.L
        assert len(W.ae_conv_specs(c.C, c.B, c.heatmap)) == 2 * (6 * c.B + 2) + 6
        assert (S.relu_layers(sc), S.residual_layers(sc), S.gradients(sc)) == (4 + 6 * c.B, 12 * c.B + 4, 3 * (12 * c.B + 10) + 9)
        assert S.decision_kinds(sc) == {'symbols', 'relu', 'x_out_low', 'x_out_high'} | ({'heatmap_low', 'heatmap_high'} if c.heatmap else set())
        # to_bn and the data gradient of from_bn have a matrix-core form up to 128 channels; ae_configs/base's 193 / 192 have none
        mfma = int(L.lib.ic_conv2d_mfma_packed_floats(5, 5, 128, c.to_bn, 2, 0))
        assert (mfma > 0) == (c.to_bn <= 128) and (int(L.lib.ic_conv2d_mfma_packed_floats(3, 3, 128, c.C, 2, 0)) > 0) == (c.C <= 128)
        for shape in c.shapes + (K.STEP_SHAPE,):
            assert shape[2] % 8 == 0 and shape[3] % 8 == 0
    # from_bn: deconv3_mfma_kernel<32 | 64> only; the x1 form of to_bn at C + 1 = 32 m + 1 > 1
    assert all(c.C not in (32, 64) for c in K.TABLE if c.id != 'norm_off')
    assert [c.id for c in K.TABLE if c.to_bn % 32 == 1 and c.to_bn <= 128] == ['norm_off', 'c96_b3_l16'] and (K.BY_ID['c96_b3_l16'].to_bn - 1) // 32 == 3
    assert [c.id for c in K.TABLE if c.to_bn < 32] == ['c16_b1_l8', 'c8_b0_l2_nohm'] and K.BY_ID['c48_b3_nohm'].to_bn == 32 + 16
    # the square image's 8 x 8 maps take the F(4x4)-over-phases form of h2 / h12, the narrow one's 4 x 6 do not
    assert int(L.lib.ic_wino4_conv5s2_supported(2, 8, 8)) == 1 and int(L.lib.ic_wino4_conv5s2_supported(1, 4, 6)) == 0
    # the training step's 8 x 16 maps: one 2 x 8 segment per map with all its tiles, 4 work-groups -- the half-full rule of
    # TrainGraph._pack_all_3x3 admits them (the square image's 8 x 8 maps it would not), so wino4=True runs F(4x4) both ways
    assert K.STEP_SHAPE == (2, 3, 32, 64) and S.segments(8, 16) == ('2x8', 1) and S.workgroups(2, 8, 16) == 4
    assert S.half_full(2, 8, 16) and not S.half_full(2, 8, 8)
    assert int(L.lib.ic_conv3x3_c128_pick_algo(2, 8, 16, 0)) == 1 and int(L.lib.ic_wino4_3x3_c128_supported(2, 8, 16)) == 1
    assert int(L.lib.ic_wino4_3x3_c128_workgroups(2, 8, 16)) == 4 and int(L.lib.ic_wino4_3x3_c128_stats_parts(2, 8, 16)) == 2
    assert all(sc.shape == K.STEP_SHAPE and sc.maps == (8, 16) and sc.segments == '2x8' and sc.modes == (False, True) for sc in K.STEP_CASES)
    # the existing table is untouched by the new field
    assert all(c.overrides == () for c in S.CASES) and S.weights() is S.weights(S.CASES[0]) is S.weights(S.CASES[2])


def test_off_fold_is_the_fixed_normalisation_at_a_grey_interior():
    """OFF with the folded variables computes, away from the border, what the plain ones compute on (x - m) / s with the scalar m, s
    of the fold (FIXED itself differs from that by the spread of the three channels' constants about their means); the fold touches
    h1 and h13 alone"""
    from imgcomp_cvpr_amd import weights as W
    from oracle import oracle as O
    sc = K.case(K.BY_ID['norm_off'])
    ae, pc = S.configs(sc)
    folded, plain = S.weights(sc), W.synthetic_weights(ae, pc)
    changed = sorted(n for n in plain if not np.array_equal(plain[n], folded[n]))
    assert changed == sorted(['autoencoder/encoder/h1/weights', 'autoencoder/encoder/h1/BatchNorm/moving_mean',
                              'autoencoder/decoder/h13/BatchNorm/gamma', 'autoencoder/decoder/h13/BatchNorm/beta'])
    mean, std = O.norm_consts(torch.float64)
    m, s = float(mean.mean()), float(std.mean())
    x = torch.as_tensor(S.image(sc)).double()[:, :1].repeat(1, 3, 1, 1)
    h1 = 'autoencoder/encoder/h1'
    off = O.conv_bn_act(x, folded, h1, 2, False)
    fixed = O.conv_bn_act((x - m) / s, plain, h1, 2, False)
    assert rel_err(off[:, :, 1:-1, 1:-1], fixed[:, :, 1:-1, 1:-1]) <= 1e-6          # (float32 storage of the folded variables)
    assert rel_err(off, fixed) > 1e-3                                             # the border sees the zero padding un-normalised
    h13 = 'autoencoder/decoder/h13'
    t = torch.as_tensor(np.random.RandomState(0).normal(0, 1, (1, 64, 4, 4)))
    assert rel_err(O.conv_bn_act(t, folded, h13, 2, False, transpose=True), O.conv_bn_act(t, plain, h13, 2, False, transpose=True) * s + m) <= 1e-6


@pytest.mark.parametrize('c,shape', K.INFERENCE, ids=[K.inference_id(cs) for cs in K.INFERENCE])
def test_inference_oracle_is_not_degenerate_and_fp32_meets_float64(c, shape):
    """per case and image: at most 1 % of the float64 oracle's x_out on the clip's edges, at least two symbols with 5 % of the
    volume each; and the float32 oracle against the float64 one inside the bounds the GPU test uses -- z, x_out and the bit cost at
    NET_RTOL, the importance map at heatmap_rtol, no symbol flip outside the band of 2 x the z error about a decision midpoint."""
    from oracle import oracle as O
    sc = K.case(c, shape)
    r64, r32 = K.reference(c, shape), K.reference(c, shape, torch.float32)
    label = 'inference {} {}'.format(c.id, shape)
    _non_degenerate(label, r64.x_out, r64.enc.symbols, c.L)
    assert (r64.enc.heatmap is None) == (not c.heatmap)
    errs = {'z': rel_err(r32.enc.z, r64.enc.z)}
    if c.heatmap:
        errs['heatmap'] = rel_err(r32.enc.heatmap, r64.enc.heatmap)
        assert errs['heatmap'] <= K.heatmap_rtol(c), errs
    # decoder and context model fed the SAME (float64 oracle's) symbols, as the GPU test feeds them
    w, cfg = S.weights(sc), S.configs(sc)[0].as_dict()
    with torch.no_grad():
        errs['x_out'] = rel_err(O.decode(r64.enc.qhard.float(), w, cfg), r64.x_out)
        errs['bits'] = rel_err(O.bitcost(r64.enc.qhard.float(), r64.enc.symbols, w, float(S.centers(sc)[0]))[0], r64.bits)
    flips = (r32.enc.symbols != r64.enc.symbols).numpy()
    zerr = float((r32.enc.z.double() - r64.enc.z).abs().max())
    print('{}: float32 against float64 oracle {}; {} of {} symbols flipped'.format(
        label, {k: '{:.2e}'.format(v) for k, v in errs.items()}, int(flips.sum()), flips.size))
    assert errs['z'] <= NET_RTOL and errs['x_out'] <= NET_RTOL and errs['bits'] <= NET_RTOL, errs
    assert not np.any(flips & (_boundary_margin(r64.enc.z.numpy(), S.centers(sc)) > 2 * zerr + 1e-12))


def test_off_and_fixed_encodes_differ():
    """the same variables under the other normalisation give another z (what the GPU test asserts of the device, of the oracle)"""
    from oracle import oracle as O
    for cid in ('norm_off', 'c8_b0_l2_nohm'):
        c = K.BY_ID[cid]
        sc = K.case(c, K.SQUARE)
        cfg = dict(S.configs(sc)[0].as_dict(), normalization='FIXED')
        with torch.no_grad():
            other = O.encode(torch.as_tensor(S.image(sc)).double(), S.weights(sc), cfg)
        assert rel_err(other.z, K.reference(c, K.SQUARE).enc.z) > 1e-2


OFF_INFERENCE = [cs for cs in K.INFERENCE if cs[0].normalization == 'OFF']


@pytest.mark.parametrize('c,shape', OFF_INFERENCE, ids=[K.inference_id(cs) for cs in OFF_INFERENCE])
def test_clip_probe_engages_both_edges(c, shape):
    """the decoder input that the GPU test feeds the OFF cases' clip-only epilogue: at least 0.5 % of the float64 oracle's x_out on
    EACH edge, at least half of it strictly between them; float32 against float64 within NET_RTOL"""
    from oracle import oracle as O
    sc = K.case(c, shape)
    assert set(K.CLIP_PROBE_SIGMA) == {k.id for k in K.TABLE if k.normalization == 'OFF'}
    q, x_out = K.clip_probe(c, shape)
    low, high = float((x_out <= 0).double().mean()), float((x_out >= 255).double().mean())
    with torch.no_grad():
        err = rel_err(O.decode(torch.as_tensor(q), S.weights(sc), S.configs(sc)[0].as_dict()), x_out)
    print('clip probe {} {}: on 0 {:.4f}, on 255 {:.4f}; float32 against float64 {:.2e}'.format(c.id, shape, low, high, err))
    assert low >= 0.005 and high >= 0.005 and low + high <= 0.5, (low, high)
    assert err <= NET_RTOL, err


@pytest.mark.parametrize('sc', K.STEP_CASES, ids=lambda sc: sc.id)
def test_step_oracle_is_not_degenerate_and_fp32_meets_float64_at_forced_decisions(sc):
    """the training-mode oracle of the four step cases: at most STEP_MAX_EDGE_SHARE of its own x_out on the clip's edges, two symbols
    with 5 % each; float32 against float64 forward (z, bit cost, x_out) within the 1e-4 of the GPU test; and, as
    test_cpu_step_cases.test_fp32_oracle_meets_float64_at_forced_decisions does for the existing cases, the float32 decisions in band
    and at most MAX_DIFFERING of all, every gradient at the float32 decisions within GTOL."""
    c = K.BY_ID[sc.id]
    _, comps64, grads64 = S.unforced(sc)
    _non_degenerate('step {}'.format(sc.id), comps64['x_out'], comps64['symbols'], c.L, STEP_MAX_EDGE_SHARE)
    assert set(comps64['decisions']) == S.decision_kinds(sc) and len(comps64['relu_pre']) == S.relu_layers(sc)
    assert len(grads64) == S.gradients(sc)
    _, comps32, grads32 = S.oracle(sc, dtype=torch.float32)
    fwd = {k: rel_err(comps32[k], comps64[k]) for k in ('z', 'bc', 'x_out')}
    counts = S.in_band(S.oracle_side(comps32), comps64, sc)
    print('step {}: float32 against float64 forward {}; decisions {}'.format(sc.id, {k: '{:.2e}'.format(v) for k, v in fwd.items()}, dict(counts)))
    assert max(fwd.values()) <= 1e-4, fwd
    assert counts['out_of_band'] == 0, counts
    assert counts['differing'] <= S.MAX_DIFFERING * counts['total'], counts
    _, comps_f, grads_f = S.oracle(sc, decisions=comps32['decisions'])
    assert torch.equal(comps_f['symbols'], comps32['symbols'])
    name, err = S.worst_gradient_error(grads32, grads_f)
    print('step {}: worst gradient, float32 against float64 at the float32 decisions: {} {:.3e}'.format(sc.id, name, err))
    assert err <= S.GTOL, (name, err)
