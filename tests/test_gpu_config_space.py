"""-m gpu: the configurations of tests/config_cases.py -- normalization = OFF, C outside {32, 64}, B other than 5, L other than 6,
with and without the importance map -- through inference (encode under three plans, decode, bit cost) and through one whole training
step, against the float64 oracle.  tests/test_cpu_config_cases.py holds the conditions that keep these comparisons from passing
vacuously; tests/config_cases.py says what each case reaches.

Bounds: util.NET_RTOL for z, x_out and the bit cost (what tests/test_gpu_network.py holds cvpr/low to); the importance map at
HEATMAP_RTOL * max(1, C / 64) -- tests/util.py derives HEATMAP_RTOL from the C / 4 amplification of z0's error by sigmoid(z0) * C at
C <= 64, so the bound scales with C and is not tuned against the device; the training step exactly as
tests/test_gpu_step_decisions.py (its check_step, unchanged)."""
import numpy as np
import pytest
import torch

from tests import config_cases as K
from tests import step_cases as S
from tests import test_gpu_step_decisions as D
from tests import util
from tests.util import NET_RTOL, RTOL, _boundary_margin, assert_close, dev, record_flips

pytestmark = pytest.mark.gpu
_NETS = {}                       # case id -> (autoencoder, context model): one pair per case per process


def _nets(cuda, c):
    if c.id not in _NETS:
        from imgcomp_cvpr_amd import autoencoder, probclass
        sc = K.case(c)
        ae_cfg, pc_cfg = S.configs(sc)
        ae = autoencoder.get_network_cls(ae_cfg)(ae_cfg).load_weights(S.weights(sc), cuda)
        pc = probclass.get_network_cls(pc_cfg)(pc_cfg, num_centers=ae_cfg.num_centers).load_weights(S.weights(sc), cuda)
        _NETS[c.id] = (ae, pc)
    return _NETS[c.id]


def _plans():
    from imgcomp_cvpr_amd import _lib
    return (('default', 0), ('wino4', _lib.CONV3_WINO4 | _lib.CONV5_WINO4), ('no_wino4', _lib.CONV3_NO_WINO4 | _lib.CONV5_NO_WINO4))


def _check_encode(enc, ae, ref, c, centers, label):
    """one encode against the float64 oracle's: the rule of test_gpu_network.test_encode_matches_oracle"""
    from oracle import oracle as O
    assert enc.symbols.dtype == torch.int64 and enc.symbols.shape == ref.symbols.shape
    assert_close(enc.z, ref.z, label + ': z', NET_RTOL)
    if c.heatmap:
        assert_close(enc.heatmap, ref.heatmap, label + ': heatmap', K.heatmap_rtol(c))
    else:
        assert enc.heatmap is None and enc.qbar is enc.qhard
    # symbols: the oracle's wherever z is farther from a decision midpoint than twice the measured z error
    zerr = float((enc.z.double().cpu() - ref.z).abs().max())
    flips = (enc.symbols.cpu() != ref.symbols).numpy()
    assert not np.any(flips & (_boundary_margin(ref.z.numpy(), centers) > 2 * zerr + 1e-12)), 'symbol flips away from decision boundaries'
    assert record_flips(label, flips) < 2e-3, 'too many boundary flips: {}'.format(flips.mean())
    same = torch.as_tensor(~flips)
    assert torch.equal(enc.qhard.cpu()[same], ref.qhard.float()[same])
    # given the device's own z, symbols and qhard are exactly O.quantize's
    _, qh, sym = O.quantize(enc.z.cpu(), centers, 1.0)
    assert torch.equal(sym, enc.symbols.cpu()) and torch.equal(qh, enc.qhard.cpu())
    if c.heatmap:
        assert torch.equal(enc.qbar.cpu(), (ae._last_qsoft + (enc.qhard - ae._last_qsoft)).cpu())


def _check_decode(x_out, ref_x_out, label):
    """the rule of test_gpu_network.test_decode_matches_oracle"""
    assert float(x_out.min()) >= 0 and float(x_out.max()) <= 255
    assert_close(x_out, ref_x_out, label + ': x_out', NET_RTOL)
    # uint8 truncation (val.py:91) can differ only where the float64 value sits on an integer boundary
    frac = ref_x_out - torch.floor(ref_x_out)
    near_int = torch.minimum(frac, 1 - frac) < 255 * RTOL
    assert not bool(((x_out.to(torch.uint8).cpu() != ref_x_out.to(torch.uint8)) & ~near_int).any())


@pytest.mark.parametrize('c,shape', K.INFERENCE, ids=[K.inference_id(cs) for cs in K.INFERENCE])
def test_inference_matches_oracle(cuda, c, shape):
    ae, pc = _nets(cuda, c)
    ref = K.reference(c, shape)
    centers = np.asarray(S.weights(K.case(c))['autoencoder/encoder/centers'])
    x = dev(ref.x, cuda)
    label = 'config {} {}'.format(c.id, K.shape_id(shape))
    # encode: the default plan, F(4x4) wherever the maps allow (3x3 layers and h2), F(4x4) nowhere
    zs = {}
    for name, flags in _plans():
        enc = ae.encode(x, is_training=False, plan_flags=flags)
        torch.cuda.synchronize()
        _check_encode(enc, ae, ref.enc, c, centers, '{} encode {}'.format(label, name))
        zs[name] = enc.z.clone()
    if shape == K.SQUARE:
        assert not torch.equal(zs['wino4'], zs['no_wino4']), 'the plan flags reached no kernel'
    # decode and bit cost, fed the oracle's qhard and symbols
    q = dev(ref.enc.qhard.float().numpy(), cuda)
    for name, flags in _plans():
        x_out = ae.decode(q, is_training=False, plan_flags=flags)
        torch.cuda.synchronize()
        assert x_out.shape == tuple(shape)
        _check_decode(x_out, ref.x_out, '{} decode {}'.format(label, name))
    bc = pc.bitcost(q, ref.enc.symbols.to(cuda), is_training=False, pad_value=float(centers[0]))
    torch.cuda.synchronize()
    assert_close(bc, ref.bits, label + ': bit cost', NET_RTOL)


@pytest.mark.parametrize('cid', [c.id for c in K.TABLE if c.normalization == 'OFF'])
def test_normalization_off_reaches_the_kernels(cuda, cid):
    """the same variables under FIXED give another z and another x_out: normalize_on reached h1 and h13"""
    from imgcomp_cvpr_amd import autoencoder
    c = K.BY_ID[cid]
    sc = K.case(c)
    ae, _ = _nets(cuda, c)
    fixed_cfg = S.configs(sc._replace(overrides=sc.overrides + (('normalization', 'FIXED'),)))[0]
    assert fixed_cfg.normalization == 'FIXED' and ae.config.normalization == 'OFF'
    fixed = autoencoder.get_network_cls(fixed_cfg)(fixed_cfg).load_weights(S.weights(sc), cuda)
    ref = K.reference(c, K.SQUARE)
    x, q = dev(ref.x, cuda), dev(ref.enc.qhard.float().numpy(), cuda)
    assert util.rel_err(fixed.encode(x, is_training=False).z, ref.enc.z) > 1e-2
    assert util.rel_err(fixed.decode(q, is_training=False), ref.x_out) > 1e-2
    assert_close(ae.encode(x, is_training=False).z, ref.enc.z, 'config {} OFF beside FIXED: z'.format(cid), NET_RTOL)


OFF_INFERENCE = [cs for cs in K.INFERENCE if cs[0].normalization == 'OFF']


@pytest.mark.parametrize('c,shape', OFF_INFERENCE, ids=[K.inference_id(cs) for cs in OFF_INFERENCE])
def test_normalization_off_decode_clips(cuda, c, shape):
    """h13's clip-only epilogue with the clip engaged (config_cases.clip_probe: the oracle's x_out sits on both edges): within
    [0, 255], on an edge wherever the oracle's is, and the oracle's value at NET_RTOL, under the three plans"""
    ae, _ = _nets(cuda, c)
    q, ref = K.clip_probe(c, shape)
    label = 'config {} {} clip probe'.format(c.id, K.shape_id(shape))
    for name, flags in _plans():
        x_out = ae.decode(dev(q, cuda), is_training=False, plan_flags=flags)
        torch.cuda.synchronize()
        _check_decode(x_out, ref, '{} decode {}'.format(label, name))
        got = x_out.cpu()
        assert int((got == 0).sum()) > 0 and int((got == 255).sum()) > 0


@pytest.mark.parametrize('case,mode', K.STEP_CASE_MODES, ids=[S.case_mode_id(cm) for cm in K.STEP_CASE_MODES])
def test_step_matches_oracle_at_the_devices_decisions(cuda, case, mode):
    """one whole training step of the configuration: everything tests/test_gpu_step_decisions.py asserts of its own cases"""
    D.check_step(cuda, case, mode)


def test_base_sizes_train_and_evaluate_in_training(cuda):
    """ae_configs/base's sizes (C = 192, B = 3; to_bn has 193 output channels, beyond the matrix-core form): one training step,
    then the test-in-train evaluation -- encode / decode with is_training=False on the bound object -- runs and matches the oracle
    evaluated with the updated variables and their moving statistics"""
    from imgcomp_cvpr_amd import autoencoder, probclass, training
    from oracle import oracle as O
    c = K.BY_ID['base_c192_b3']
    sc = K.case(c)
    ae_cfg, pc_cfg = S.configs(sc)
    trainer = training.Trainer(ae_cfg, pc_cfg, S.weights(sc), cuda, wino4=False)
    ae = autoencoder.get_network_cls(ae_cfg)(ae_cfg)
    pc = probclass.get_network_cls(pc_cfg)(pc_cfg, num_centers=ae_cfg.num_centers)
    trainer.graph.bind(ae, pc)
    out = trainer.step(dev(S.image(sc), cuda))
    assert all(np.isfinite(v) for v in out.values()), out
    x = K.reference(c, K.TINY).x
    enc = ae.encode(dev(x, cuda), is_training=False)
    torch.cuda.synchronize()
    now = trainer.state_weights(training_state=False)
    before = S.weights(sc)
    for name in ('autoencoder/encoder/to_bn/weights', 'autoencoder/encoder/to_bn/BatchNorm/moving_mean', 'autoencoder/decoder/from_bn/weights'):
        assert not np.array_equal(now[name], before[name]), name + ' did not move in the step'
    with torch.no_grad():
        ref = O.encode(torch.as_tensor(x).double(), now, ae_cfg.as_dict())
        ref_x_out = O.decode(ref.qhard, now, ae_cfg.as_dict())
    label = 'config base_c192_b3 test-in-train'
    _check_encode(enc, ae, ref, c, np.asarray(now['autoencoder/encoder/centers']), label + ' encode')
    assert util.rel_err(enc.z, K.reference(c, K.TINY).enc.z) > 1e-3, 'is_training=False did not pick up the updated variables'
    _check_decode(ae.decode(dev(ref.qhard.float().numpy(), cuda), is_training=False), ref_x_out, label + ' decode')
