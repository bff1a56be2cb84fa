"""-m gpu: one whole training step per case and F(4x4) mode of tests/step_cases.py against the float64 oracle WITH THE DEVICE'S
DISCRETE DECISIONS FORCED (oracle.train_oracle.train_loss(decisions=...)): every one of the gradients (219 here) at GTOL = 2e-4 on maps
larger than 8 x 8, on the shipped path of the 3x3 layers (F(4x4) forward with the BatchNorm sums in its epilogue, F(4x4) data
gradient; TrainGraph.WINO4_MIN_WORKGROUPS lowered on the instance) and on the F(2x2) path, with every decision that differs from the
oracle's own checked to sit inside the rounding band of its threshold.  tests/step_cases.py says why.

GTOL is the project's bound for every gradient of a small step (tests/test_gpu_training.py).  In float32-against-float64 runs of the
oracle alone the gradient error at forced decisions about equals the forward error relative to scale (a few 1e-6); training.py records
F(4x4)'s z error as 3.6e-5, which leaves about 5 x."""
import pytest
import torch

from tests import step_cases as S
from tests import util
from tests.util import assert_close, dev, record_flips, rel_err

pytestmark = pytest.mark.gpu
_RUNS = {}                       # (case id, mode) -> the device step's record: one step per case and mode per process


def _run(cuda, case, mode):
    key = (case.id, mode)
    if key not in _RUNS:
        from imgcomp_cvpr_amd import training
        ae, pc = S.configs(case)
        g = training.TrainGraph(ae, pc, S.weights(case), cuda, wino4=mode)
        if mode is not False:
            g.WINO4_MIN_WORKGROUPS = 1               # on the instance: the class default stays 160
        x = dev(S.image(case), cuda)
        if case.distortion == 'ms_ssim':
            from imgcomp_cvpr_amd import _lib as L
            assert L.lib.ic_msssim_plan_bytes(case.shape[2], case.shape[3]) > 0
            assert isinstance(g._hip_distortion(x), training._HipMsSsimDistortion)
        out, side, served = S.device_decisions(g, x)
        grads = {n: t.detach().cpu().clone() for n, t in g.grads.items()}
        _RUNS[key] = {'out': out, 'side': side, 'served': served, 'f4': tuple(bool(b) for b in g._w3_f4), 'grads': grads,
                      'reg': g.regularization_loss(), 'class_default': training.TrainGraph.WINO4_MIN_WORKGROUPS}
    return _RUNS[key]


def check_step(cuda, case, mode):
    """the whole comparison of one case and mode (tests/test_gpu_config_space.py runs its own cases through it, unchanged); the
    counts of gradients, ReLU layers and residual layers come from the case's configuration (S.gradients / relu_layers /
    residual_layers)"""
    label = 'step {} wino4={}'.format(case.id, mode)
    run = _run(cuda, case, mode)
    out, side = run['out'], run['side']
    n_grads, n_relu, n_res = S.gradients(case), S.relu_layers(case), S.residual_layers(case)
    # 1. the path taken (every case's maps pass TrainGraph's half-full rule: tests/test_cpu_step_cases.py, test_cpu_config_cases.py)
    assert run['f4'] == (mode in (True, 'fwd'), mode in (True, 'bwd')) and run['class_default'] == 160
    assert run['served'] == (n_res if run['f4'][0] else 0), 'conv + BatchNorm sums served {} of the {} residual 3x3 layers'.format(run['served'], n_res)
    # 2. forward, against the unforced float64 oracle
    _, ref, _ = S.unforced(case)
    assert_close(side['z'], ref['z'], label + ': z', 1e-4)
    assert_close(side['bc'], ref['bc'], label + ': bit cost', 1e-4)
    assert_close(side['x_out'], ref['x_out'], label + ': x_out', 1e-4)
    assert list(side['relu_out']) == list(ref['relu_pre']) and len(side['relu_out']) == n_relu
    scope = max(side['relu_out'], key=lambda s: rel_err(side['relu_out'][s], torch.relu(ref['relu_pre'][s])))
    assert_close(side['relu_out'][scope], torch.relu(ref['relu_pre'][scope]), label + ': worst post-ReLU layer output', 1e-4)
    # 3. decisions: every difference inside the rounding band of its threshold, and few
    counts = S.in_band(side, ref, case)
    print('{}: decisions {}'.format(label, dict(counts)))
    util.REPORT.append(('{}: differing decisions relu {} hm {} x_out {}'.format(label, counts['relu'], counts['heatmap'], counts['x_out']),
                        counts['differing'], counts['differing'] / counts['total'], S.MAX_DIFFERING))
    record_flips(label, (side['decisions']['symbols'] != ref['symbols']).numpy())
    assert counts['out_of_band'] == 0, counts
    assert counts['differing'] <= S.MAX_DIFFERING * counts['total'], counts
    # 4. gradients and scalars, against the float64 oracle at the device's decisions
    _, forced, grads = S.oracle(case, decisions=side['decisions'])
    assert torch.equal(forced['symbols'], side['decisions']['symbols'])          # the symbols the forced evaluation used
    assert set(grads) == set(run['grads']) and len(grads) == n_grads
    print('{}: worst gradient {}; against the UNFORCED oracle (not asserted: what the differing decisions alone move) {}'.format(
        label, S.worst_gradient_error(run['grads'], grads), S.worst_gradient_error(run['grads'], S.unforced(case)[2])))
    for name, ref_grad in grads.items():
        assert_close(run['grads'][name], ref_grad, label + ': every gradient, forced oracle', S.GTOL)
    assert abs(out['d_loss_scaled'] - float(forced['d_loss_scaled'])) < 1e-3 * abs(float(forced['d_loss_scaled']))
    assert abs(out['pc_loss'] - float(forced['pc_loss'])) < 1e-3 * abs(float(forced['pc_loss'])) and out['pc_loss'] > 0
    assert abs(out['H_real'] - float(forced['H_real'])) < 1e-4 * abs(float(forced['H_real']))
    assert abs(out['H_mask'] - float(forced['H_mask'])) < 1e-4 * abs(float(forced['H_mask']))
    assert abs(run['reg'] - float(forced['reg'])) < 1e-4 * float(forced['reg'])
    if case.distortion == 'ms_ssim':
        K = float(S.configs(case)[0].K_ms_ssim)
        assert abs(out['ms_ssim'] - (1.0 - float(forced['d_loss_scaled']) / K)) <= 2e-4


@pytest.mark.parametrize('case,mode', S.CASE_MODES, ids=[S.case_mode_id(cm) for cm in S.CASE_MODES])
def test_step_matches_oracle_at_the_devices_decisions(cuda, case, mode):
    assert (S.gradients(case), S.relu_layers(case), S.residual_layers(case)) == (219, 34, 64)          # cvpr/med: B = 5
    check_step(cuda, case, mode)


def test_wide_forward_does_not_depend_on_the_backward_mode(cuda):
    """z and symbols of 'bwd' are bit-identical to False, those of True to 'fwd' (the data gradient's form cannot reach the forward);
    and the F(4x4) forward is really another kernel."""
    case = S.BY_ID['wide']
    r = {m: _run(cuda, case, m)['side'] for m in case.modes}
    for a, b in (('bwd', False), (True, 'fwd')):
        assert torch.equal(r[a]['z'], r[b]['z']) and torch.equal(r[a]['decisions']['symbols'], r[b]['decisions']['symbols']), (a, b)
    assert not torch.equal(r['fwd']['z'], r[False]['z'])
