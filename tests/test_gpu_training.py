"""-m gpu: training-mode kernels (BatchNorm, filter gradients, quantiser / context-model backward) and one whole
training step against the CPU oracle's autograd (oracle/train_oracle.py)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.util import assert_close, dev, true_rel_err

pytestmark = pytest.mark.gpu
GTOL = 2e-4        # gradients: relative to the tensor scale, vs the float64 autograd of the oracle


def _L():
    from imgcomp_cvpr_amd import _lib
    return _lib


def test_bn_train_forward_backward(cuda):
    L = _L()
    rs = np.random.RandomState(0)
    N, C, H, W = 3, 37, 6, 10
    x = rs.normal(0.3, 2.0, (N, C, H, W)).astype(np.float32)
    gamma = rs.uniform(0.5, 1.5, C).astype(np.float32)
    beta = rs.normal(0, 0.3, C).astype(np.float32)
    res = rs.normal(0, 1, (N, C, H, W)).astype(np.float32)
    dy = rs.normal(0, 1, (N, C, H, W)).astype(np.float32)
    for relu in (0, 1):
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        gt = torch.tensor(gamma, dtype=torch.float64, requires_grad=True)
        bt = torch.tensor(beta, dtype=torch.float64, requires_grad=True)
        y = F.batch_norm(xt, None, None, gt, bt, training=True, eps=1e-5)
        if relu:
            y = F.relu(y)
        y = y + torch.tensor(res, dtype=torch.float64)
        y.backward(torch.tensor(dy, dtype=torch.float64))
        d = lambda a: dev(a, cuda)
        xd, dyd = d(x), d(dy)
        ws = torch.empty(L.lib.ic_bn_workspace_bytes(C), dtype=torch.uint8, device=cuda)
        mean, var = torch.empty(C, device=cuda), torch.empty(C, device=cuda)
        L.check(L.lib.ic_bn_stats_f32(L.ptr(xd), L.ptr(mean), L.ptr(var), N, C, H * W, L.ptr(ws), L.current_stream()))
        assert_close(mean, xt.detach().mean(dim=(0, 2, 3)), 'batch mean', 1e-6)
        assert_close(var, xt.detach().var(dim=(0, 2, 3), unbiased=False), 'batch var (biased)', 1e-6)
        invstd = torch.rsqrt(var + 1e-5)
        scale = d(gamma) * invstd
        shift = d(beta) - mean * scale
        yd = torch.empty_like(xd)
        resd, gammad = d(res), d(gamma)
        L.check(L.lib.ic_bn_apply_f32(L.ptr(xd), L.ptr(scale), L.ptr(shift), L.ptr(resd), None, L.ptr(yd), N, C, H * W,
                                      relu, L.current_stream()))
        assert_close(yd, y.detach(), 'bn apply', 1e-5)
        dx, dg, db = torch.empty_like(xd), torch.empty(C, device=cuda), torch.empty(C, device=cuda)
        L.check(L.lib.ic_bn_backward_f32(L.ptr(dyd), L.ptr(xd), L.ptr(scale), L.ptr(shift), L.ptr(mean), L.ptr(invstd),
                                         L.ptr(gammad), L.ptr(dx), L.ptr(dg), L.ptr(db), N, C, H * W, relu, L.ptr(ws),
                                         L.current_stream()))
        torch.cuda.synchronize()
        assert_close(db, bt.grad, 'dbeta', 1e-5)
        assert_close(dg, gt.grad, 'dgamma', 1e-5)
        assert_close(dx, xt.grad, 'bn dx', 1e-5)


@pytest.mark.parametrize('N,H,W', [(32, 32, 32), (2, 37, 68), (1, 128, 192), (3, 30, 44), (30, 40, 40)])
def test_conv3x3_epilogue_batchnorm_sums(cuda, N, H, W):
    """Round 6: the training step's forward 3x3 convolution leaves the per-segment channel sums of its RAW output
    behind (ic_wino4_3x3_c128_raw_stats_f32: both segment shapes, ragged maps -- rows and tiles beyond the map must not count), and
    ic_bn_train_forward_cstats_f32 makes the layer's training-mode BatchNorm of them in one launch.  Against the two-launch form on the
    same raw tensor (ic_bn_train_forward_f32: float64 sums): raw output bit-identical to the plain F(4x4) launch, statistics within
    1e-6, outputs and moving averages within 1e-6 of the tensor scale; repeated launches give the same bits."""
    L = _L()
    g = torch.Generator().manual_seed(21 + H)
    x = (torch.relu(torch.randn((N, 128, H, W), generator=g)) * 1.3).to(cuda)
    w = (torch.randn((3, 3, 128, 128), generator=g) * 0.04).to(cuda)
    gamma, beta = (torch.rand(128, generator=g) * 0.8 + 0.6).to(cuda), (torch.randn(128, generator=g) * 0.2).to(cuda)
    res = torch.randn((N, 128, H, W), generator=g).to(cuda)
    st = L.current_stream()
    wp = torch.empty(L.lib.ic_wino4_3x3_c128_packed_floats(), device=cuda)
    L.check(L.lib.ic_pack_wino4_3x3_c128_f32(L.ptr(w), L.ptr(wp), 0, st))
    ones, zeros = torch.ones(128, device=cuda), torch.zeros(128, device=cuda)
    raw_ref = torch.empty((N, 128, H, W), device=cuda)
    L.check(L.lib.ic_wino4_3x3_c128_bn_act_f32(L.ptr(x), L.ptr(wp), L.ptr(ones), L.ptr(zeros), None, None, L.ptr(raw_ref), N, H, W, 0,
                                               L.CONV3_WINO4_WG4, st))
    parts = int(L.lib.ic_wino4_3x3_c128_stats_parts(N, H, W))
    assert parts == int(L.lib.ic_wino4_3x3_c128_workgroups(N, H, W)) // 2
    outs = []
    for _ in range(2):
        raw = torch.full((N, 128, H, W), float('nan'), device=cuda)
        cst = torch.full((128, parts, 2), float('nan'), device=cuda)
        L.check(L.lib.ic_wino4_3x3_c128_raw_stats_f32(L.ptr(x), L.ptr(wp), L.ptr(raw), L.ptr(cst), N, H, W, 0, st))
        outs.append((raw, cst))
    torch.cuda.synchronize()
    raw, cst = outs[0]
    assert torch.equal(raw, raw_ref), 'the STATS instantiation stores other values than the plain launch'
    assert torch.equal(outs[1][0], raw) and torch.equal(outs[1][1], cst) and bool(torch.isfinite(cst).all())
    tot = cst.double().sum(dim=1)
    assert_close(tot[:, 0], raw.double().sum(dim=(0, 2, 3)), 'conv epilogue: channel sums', 1e-6)
    assert_close(tot[:, 1], (raw.double() ** 2).sum(dim=(0, 2, 3)), 'conv epilogue: channel sums of squares', 1e-6)

    def bn(fused):
        mm, mv = torch.full((128,), 0.25, device=cuda), torch.full((128,), 1.5, device=cuda)
        o = [torch.empty(128, device=cuda) for _ in range(4)]
        y = torch.empty_like(raw)
        if fused:
            L.check(L.lib.ic_bn_train_forward_cstats_f32(L.ptr(raw), L.ptr(cst), parts, L.ptr(gamma), L.ptr(beta), L.ptr(mm), L.ptr(mv), 0.9, 1e-5,
                                                         L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]), L.ptr(o[3]), L.ptr(res), None, L.ptr(y), N, 128, H * W, 1, st))
        else:
            ws = torch.empty(L.lib.ic_bn_workspace_bytes(128), dtype=torch.uint8, device=cuda)
            L.check(L.lib.ic_bn_train_forward_f32(L.ptr(raw), L.ptr(gamma), L.ptr(beta), L.ptr(mm), L.ptr(mv), 0.9, 1e-5, L.ptr(o[0]), L.ptr(o[1]),
                                                  L.ptr(o[2]), L.ptr(o[3]), L.ptr(res), None, L.ptr(y), N, 128, H * W, 1, L.ptr(ws), st))
        torch.cuda.synchronize()
        return [y, mm, mv] + o
    a_, b_ = bn(True), bn(False)
    for name, u, v in zip(('y', 'moving mean', 'moving variance', 'mean', 'invstd', 'scale', 'shift'), a_, b_):
        assert_close(u, v.double(), 'BatchNorm from the conv epilogue sums: ' + name, 2e-6)


def test_fused_adam_matches_the_multi_tensor_form(cuda):
    """ic_adam_tf_f32 on flat buffers against TFAdam's seven multi-tensor passes (tf.train.AdamOptimizer: epsilon outside the
    bias correction) over three steps, tensors of odd sizes at 256-byte aligned offsets of the flat buffers."""
    from imgcomp_cvpr_amd import training
    rs = np.random.RandomState(5)
    sizes = [(3, 3, 5, 7), (33,), (128, 3), (1,)]
    offs, total = [], 0
    for sh in sizes:
        offs.append(total)
        total += (int(np.prod(sh)) + 63) // 64 * 64
    fp, fg = torch.zeros(total, device=cuda), torch.zeros(total, device=cuda)
    ps = [fp[o:o + int(np.prod(sh))].view(sh) for o, sh in zip(offs, sizes)]
    gs = [fg[o:o + int(np.prod(sh))].view(sh) for o, sh in zip(offs, sizes)]
    for p in ps:
        p.copy_(dev(rs.normal(0, 1, tuple(p.shape)), cuda))
    ref_p = [p.clone() for p in ps]
    ref_g = [torch.zeros_like(p) for p in ps]
    fused = training.TFAdam(ps, gs, lr=3e-3, flat=[(fp, fg)])
    plain = training.TFAdam(ref_p, ref_g, lr=3e-3)
    for step in range(3):
        for g, rg in zip(gs, ref_g):
            v = dev(rs.normal(0, 10.0 ** -step, tuple(g.shape)), cuda)
            g.copy_(v); rg.copy_(v)
        fused.step(); plain.step()
    torch.cuda.synchronize()
    for i, (p, rp) in enumerate(zip(ps, ref_p)):
        assert_close(p, rp.double(), 'fused Adam, variable {}'.format(i), 1e-6)
        assert_close(fused.m[i], plain.m[i].double(), 'fused Adam m {}'.format(i), 1e-6)
        # true_rtol: the kernel forms 1.f - beta2 in float32 as TensorFlow's does (0.00099998713, -1.29e-5 of the multi-tensor form's
        # 0.001), so every element of v differs by that share of itself: measured 1.305e-5 of max|v| (1.3e-2), bound twice that
        assert_close(fused.v[i], plain.v[i].double(), 'fused Adam v {}'.format(i), 1e-6, true_rtol=2.7e-5)
    assert float(fp[offs[1] + 33:offs[2]].abs().max()) == 0.0          # the padding between tensors stays zero


@pytest.mark.parametrize('N,H,W', [(2, 16, 16), (1, 12, 20), (1, 7, 8), (3, 9, 34), (32, 32, 32), (30, 40, 40)])
def test_winograd_filter_gradient(cuda, N, H, W):
    """ic_conv3x3_c128_wgrad_f32 (Winograd-domain GEMMs over all 2x2 tiles) against autograd in float64 on the small shapes and
    against the direct-form kernel everywhere: ragged chunks of tiles (W = 20: 10 tiles = 8 + 2), odd heights, several slices."""
    from oracle import train_oracle as T
    L = _L()
    rs = np.random.RandomState(N * 100 + H)
    x = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    dy = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    w = rs.normal(0, 0.1, (3, 3, 128, 128)).astype(np.float32)
    d = lambda a: dev(a, cuda)
    xd, dyd, wd_ = d(x), d(dy), d(w)
    need = L.lib.ic_conv3x3_c128_wgrad_workspace_bytes(N, H, W)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    dw = torch.full((3, 3, 128, 128), float('nan'), device=cuda)
    L.check(L.lib.ic_conv3x3_c128_wgrad_f32(L.ptr(xd), L.ptr(dyd), L.ptr(dw), N, H, W, L.ptr(wd_), 0.25, L.ptr(ws), need,
                                            L.current_stream()))
    need2 = L.lib.ic_conv2d_wgrad_workspace_bytes(N, 128, 128, H, W, 3, 3)
    ws2 = torch.empty(need2, dtype=torch.uint8, device=cuda)
    dw2 = torch.empty((3, 3, 128, 128), device=cuda)
    L.check(L.lib.ic_conv2d_wgrad_f32(L.ptr(xd), L.ptr(dyd), L.ptr(dw2), N, 128, H, W, 128, 3, 3, 1, L.ptr(wd_), 0.25,
                                      L.ptr(ws2), need2, L.current_stream()))
    torch.cuda.synchronize()
    assert_close(dw, dw2.double(), 'dW winograd vs direct {}x{}x{}'.format(N, H, W), 2e-5)
    if N * H * W <= 2048 or (N, H, W) == (30, 40, 40):          # and the reference's 160 x 160 training crops at full size
        torch.set_num_threads(16)
        wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
        y = T._conv(torch.tensor(x, dtype=torch.float64), wt, 1)
        y.backward(torch.tensor(dy, dtype=torch.float64))
        assert_close(dw, wt.grad + 0.25 * wt.detach(), 'dW winograd {}x{}x{}'.format(N, H, W), 1e-5)
    assert L.lib.ic_conv3x3_c128_wgrad_workspace_bytes(1, 8, 9) == 0          # odd width: the direct form serves it


@pytest.mark.parametrize('name,kind,N,Cin,Cout,H,W,K,stride', [
    ('res3x3', 'conv', 2, 128, 128, 9, 12, 3, 1),
    ('h2', 'conv', 2, 64, 128, 12, 16, 5, 2),
    ('h1', 'conv', 1, 3, 64, 16, 24, 5, 2),
    ('to_bn', 'conv', 2, 128, 33, 8, 12, 5, 2),
    ('from_bn', 'deconv', 2, 32, 128, 5, 6, 3, 2),
    ('h12', 'deconv', 1, 128, 64, 6, 8, 5, 2),
    ('h13', 'deconv', 2, 64, 3, 7, 9, 5, 2),
])
def test_conv_filter_gradients(cuda, name, kind, N, Cin, Cout, H, W, K, stride):
    from oracle import train_oracle as T
    L = _L()
    rs = np.random.RandomState(len(name))
    x = rs.normal(0, 1, (N, Cin, H, W)).astype(np.float32)
    wshape = (K, K, Cin, Cout) if kind == 'conv' else (K, K, Cout, Cin)
    w = rs.normal(0, 0.1, wshape).astype(np.float32)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    y = T._conv(xt, wt, stride) if kind == 'conv' else T._deconv(xt, wt)
    dy = rs.normal(0, 1, tuple(y.shape)).astype(np.float32)
    y.backward(torch.tensor(dy, dtype=torch.float64))
    d = lambda a: dev(a, cuda)
    xd, dyd, wd_ = d(x), d(dy), d(w)
    dw = torch.full(wshape, float('nan'), device=cuda)
    if kind == 'conv':
        U, V, A, B, UH, UW = xd, dyd, Cin, Cout, H, W
    else:
        U, V, A, B, UH, UW = dyd, xd, Cout, Cin, 2 * H, 2 * W
    VH, VW = -(-UH // stride), -(-UW // stride)
    need = L.lib.ic_conv2d_wgrad_workspace_bytes(N, A, B, VH, VW, K, K)
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    L.check(L.lib.ic_conv2d_wgrad_f32(L.ptr(U), L.ptr(V), L.ptr(dw), N, A, UH, UW, B, K, K, stride, L.ptr(wd_), 0.25,
                                      L.ptr(ws), need, L.current_stream()))
    torch.cuda.synchronize()
    assert_close(dw, wt.grad + 0.25 * wt.detach(), 'dW ' + name, 1e-5)
    # data gradient through the graph's dispatch (forward kernels reused as adjoints)
    from imgcomp_cvpr_amd import training, config_parser as cp, weights as Wm
    ae, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    if not hasattr(test_conv_filter_gradients, '_g'):
        test_conv_filter_gradients._g = training.TrainGraph(ae, pc, Wm.synthetic_weights(ae, pc), cuda)
    g = test_conv_filter_gradients._g
    if kind == 'conv' and K == 3:
        dx = g._conv3x3(dyd, wd_, backward=True)
    elif kind == 'conv':
        dx = g._deconv_s(dyd, wd_, K, K, Cout, Cin)
    else:
        dx = g._conv_s(dyd, wd_, K, K, Cout, Cin, 2)
    torch.cuda.synchronize()
    assert_close(dx, xt.grad, 'dX ' + name, 1e-5)


def test_quantizer_backward(cuda):
    L = _L()
    rs = np.random.RandomState(3)
    N, C, h, w = 2, 8, 5, 7
    bott = rs.normal(0, 1.5, (N, C + 1, h, w)).astype(np.float32)
    centers = np.linspace(-2, 2, 6).astype(np.float32)
    gq = rs.normal(0, 1, (N, C, h, w)).astype(np.float32)
    gh = rs.normal(0, 1, (N, C, h, w)).astype(np.float32)
    bt = torch.tensor(bott, dtype=torch.float64, requires_grad=True)
    ct = torch.tensor(centers, dtype=torch.float64, requires_grad=True)
    hm = torch.clamp(torch.clamp(torch.sigmoid(bt[:, 0:1]) * C - torch.arange(C, dtype=torch.float64).view(1, C, 1, 1), max=1.0), min=0.0)
    z = hm * bt[:, 1:]
    dist = (z.unsqueeze(-1) - ct) ** 2
    qsoft = (torch.softmax(-dist, -1) * ct).sum(-1)
    ((qsoft * torch.tensor(gq, dtype=torch.float64)).sum() + (hm * torch.tensor(gh, dtype=torch.float64)).sum()).backward()
    d = lambda a: dev(a, cuda)
    dbott = torch.empty((N, C + 1, h, w), device=cuda)
    dc = torch.empty(6, device=cuda)
    ws = torch.empty(L.lib.ic_heatmap_quantize_bwd_workspace_bytes(6), dtype=torch.uint8, device=cuda)
    keep = [d(bott), d(centers), d(gq), d(gh)]          # hold the device tensors until the kernel has run
    L.check(L.lib.ic_heatmap_quantize_bwd_f32(L.ptr(keep[0]), L.ptr(keep[1]), 6, 1.0, L.ptr(keep[2]), L.ptr(keep[3]),
                                              L.ptr(dbott), L.ptr(dc), N, C, h, w, 1, L.ptr(ws), L.current_stream()))
    torch.cuda.synchronize()
    assert_close(dbott, bt.grad, 'd bottleneck', 1e-5)
    assert_close(dc, ct.grad, 'd centers', 1e-5)


def test_training_step_matches_oracle(cuda):
    """forward values and EVERY parameter gradient of one step (batch 2, 32x32, MSE distortion: MS-SSIM is undefined
    for images this small, it is covered by test_ms_ssim_loss_module) against float64 autograd on the CPU."""
    from imgcomp_cvpr_amd import training, config_parser as cp, weights as W
    from oracle import train_oracle as T
    ae, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'med'))
    pc, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    ae.distortion_to_minimize = 'mse'
    ae.H_target = 0.5                                     # keep the rate term active
    wts = W.synthetic_weights(ae, pc)
    x = W.synthetic_image((2, 3, 32, 32), 'natural', 0)
    total, comps, p = T.train_loss(x, wts, ae.as_dict(), pc.as_dict(), torch.float64)
    total.backward()
    g = training.TrainGraph(ae, pc, wts, cuda)
    out = g.forward_backward(dev(x, cuda))
    torch.cuda.synchronize()
    assert torch.equal(g.last['symbols'].cpu(), comps['symbols']), 'symbol flip between fp32 and fp64: pick another seed'
    assert_close(g.last['z'], comps['z'].detach(), 'z (training-mode BN)', 1e-4)
    assert_close(g.last['bc'], comps['bc'].detach(), 'bit cost', 1e-4)
    assert_close(g.last['x_out'], comps['x_out'].detach(), 'x_out', 1e-4)
    assert abs(out['d_loss_scaled'] - float(comps['d_loss_scaled'])) < 1e-3 * abs(float(comps['d_loss_scaled']))
    assert abs(out['pc_loss'] - float(comps['pc_loss'])) < 1e-3 * abs(float(comps['pc_loss'])) and out['pc_loss'] > 0
    assert abs(g.regularization_loss() - float(comps['reg'])) < 1e-4 * float(comps['reg'])
    worst = ('', 0.0)
    for name, ref in p.items():
        if ref.grad is None:
            continue
        e = true_rel_err(g.grads[name], ref.grad)          # of max|ref| itself, no clamp at 1: 73 of the 219 are below 1
        if e > worst[1]:
            worst = (name, e)
        assert e <= GTOL, 'gradient of {}: error {:.3e} of max|ref|'.format(name, e)
    assert len([n for n in p if p[n].grad is not None]) == len(g.grads) == 219
    print('worst gradient error', worst)


@pytest.mark.parametrize('label,ae_name,pc_name,heatmap,seed', [
    ('hi training step', 'hi', 'res_shallow_64', True, 3),
    ('no-heatmap training step', 'med', 'res_shallow', False, 2),
])
def test_training_step_untested_configs_match_oracle(cuda, label, ae_name, pc_name, heatmap, seed):
    """one step (batch 2, 32x32, MSE distortion, rate term active) of the two configurations no other training test builds:
    the high-rate pair cvpr/hi + res_shallow_64 (C = 64, to_bn emits 65 channels, k = 64 context model) and cvpr/med without the
    importance map (autoencoder.py:236-242: z = to_bn's output; train.py:306-309: H_mask = H_real).  Symbols equal to the float64
    oracle's (the seeds keep every z >= 1.5e-4 away from a decision midpoint in the oracle), z / bit cost / x_out, the scalar
    losses and EVERY parameter gradient against its autograd."""
    from imgcomp_cvpr_amd import training, config_parser as cp, weights as W
    from oracle import train_oracle as T
    ae, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', ae_name))
    pc, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', pc_name))
    ae.distortion_to_minimize = 'mse'
    ae.H_target = 0.5                                     # keep the rate term active
    ae.heatmap = heatmap
    wts = W.synthetic_weights(ae, pc)
    assert np.asarray(wts['autoencoder/encoder/to_bn/weights']).shape[-1] == int(ae.num_chan_bn) + int(heatmap)
    x = W.synthetic_image((2, 3, 32, 32), 'natural', seed)
    total, comps, p = T.train_loss(x, wts, ae.as_dict(), pc.as_dict(), torch.float64)
    total.backward()
    assert (comps['heatmap'] is None) == (not heatmap)
    g = training.TrainGraph(ae, pc, wts, cuda)
    out = g.forward_backward(dev(x, cuda))
    torch.cuda.synchronize()
    assert (g.last['heatmap'] is None) == (not heatmap)
    assert torch.equal(g.last['symbols'].cpu(), comps['symbols']), 'symbol flip between fp32 and fp64: pick another seed'
    assert_close(g.last['z'], comps['z'].detach(), label + ': z', 1e-4)
    assert_close(g.last['bc'], comps['bc'].detach(), label + ': bit cost', 1e-4)
    assert_close(g.last['x_out'], comps['x_out'].detach(), label + ': x_out', 1e-4)
    assert abs(out['d_loss_scaled'] - float(comps['d_loss_scaled'])) < 1e-3 * abs(float(comps['d_loss_scaled']))
    assert abs(out['pc_loss'] - float(comps['pc_loss'])) < 1e-3 * abs(float(comps['pc_loss'])) and out['pc_loss'] > 0
    assert abs(out['H_real'] - float(comps['H_real'])) < 1e-4 * abs(float(comps['H_real']))
    assert abs(out['H_mask'] - float(comps['H_mask'])) < 1e-4 * abs(float(comps['H_mask']))
    if not heatmap:
        assert out['H_mask'] == out['H_real']
    assert abs(g.regularization_loss() - float(comps['reg'])) < 1e-4 * float(comps['reg'])
    n_ref = 0
    for name, ref in p.items():
        if ref.grad is None:
            continue
        n_ref += 1
        assert_close(g.grads[name], ref.grad, label + ': every gradient', GTOL)
    assert n_ref == len(g.grads)


def test_ms_ssim_loss_module(cuda):
    """the torch MS-SSIM loss (ms_ssim.py) on the device equals the oracle's restatement, value and gradient."""
    from imgcomp_cvpr_amd import ms_ssim, weights as W
    from oracle import train_oracle as T
    a = W.synthetic_image((2, 3, 128, 128), 'natural', 1)
    b = np.clip(a.astype(np.float64) + np.random.RandomState(0).normal(0, 6, a.shape), 0, 255)
    tb = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    ref = T.ms_ssim(torch.as_tensor(a).double(), tb)
    ref.backward()
    gb = dev(b, cuda).requires_grad_(True)
    v = ms_ssim.multiscale_ssim(dev(a, cuda), gb)
    v.backward()
    assert abs(float(v) - float(ref)) < 1e-5
    # max|ref| is 4.9e-7 here (no K; measured 7.3e-5 of it): GTOL of that, where 1e-3 of max(1, max|ref|) would have passed a gradient of zero
    assert_close(gb.grad, tb.grad, 'torch MS-SSIM module gradient', GTOL)


@pytest.mark.parametrize('shape', [(2, 3, 128, 128), (3, 3, 64, 64), (1, 3, 160, 160), (2, 3, 72, 136), (1, 3, 33, 47), (1, 2, 17, 19), (1, 3, 320, 160), (2, 3, 40, 20)])
def test_hip_ms_ssim_distortion_value_and_gradient(cuda, shape):
    """csrc/msssim.hip (ic_msssim_loss_grad_f32) against the oracle's float64 restatement of code/ms_ssim.py under autograd:
    K (1 - MS-SSIM) and its gradient with respect to the reconstruction, on the training shapes (128 and the config's 160 crops),
    the small-scale REFLECT pads (64: two scales narrower than the window), non-square, odd sizes (the (0,1) REFLECT pad of
    the 2x2 box), the smallest image with five scales, and tall crops whose coarsest scale is narrower than the window (320 x 160,
    40 x 20: the reference derives the REFLECT pad from the WIDTH -- shape[2] of its NHWC tensor, ms_ssim.py:19 / :160-162 -- and
    applies it to both axes; the transposed shapes have no valid output there, in the reference as here).
    Two calls are bit-identical (fixed-order float64 means)."""
    from imgcomp_cvpr_amd import training, config_parser as cp, weights as W
    from oracle import train_oracle as T
    ae, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'med'))
    rs = np.random.RandomState(shape[2])
    a = (W.synthetic_image((shape[0], 3, shape[2], shape[3]), 'natural', 1)[:, :shape[1]]).astype(np.float64)
    b = np.clip(a + rs.normal(0, 9, a.shape), 0, 255)
    tb = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    K = float(ae.K_ms_ssim)
    ref = K * (1.0 - T.ms_ssim(torch.as_tensor(a).double(), tb))
    ref.backward()
    hd = training._HipMsSsimDistortion(ae, shape, cuda)
    d = hd.launch(dev(a, cuda), dev(b, cuda))
    d2 = hd.launch(dev(a, cuda), dev(b, cuda))
    torch.cuda.synchronize()
    assert torch.equal(d.grad, d2.grad) and torch.equal(d.scalars[:13], d2.scalars[:13])
    assert 0.0 < float(d.ms_ssim) <= 1.0
    assert abs(float(d.ms_ssim) - (1.0 - float(ref) / K)) < 1e-5, (float(d.ms_ssim), 1.0 - float(ref) / K)
    assert abs(float(d.d_loss_scaled) - float(ref)) < 1e-5 * K
    # GTOL of max|ref| (1e-3 .. 1.4e-1 on these shapes; tests/test_gpu_msssim_grad.py has the per-scale checks)
    assert_close(d.grad, tb.grad, 'MS-SSIM distortion gradient {}x{}'.format(shape[2], shape[3]), GTOL)
    # the autograd form the plugin call sites use
    xo = dev(b, cuda).requires_grad_(True)
    dd = hd(dev(a, cuda), xo)
    (dd.d_loss_scaled * 2.0).backward()
    assert torch.equal(xo.grad, d.grad * 2.0) and float(dd.ms_ssim) == float(d.ms_ssim)
    assert lib_unsupported_below_five_scales()


def lib_unsupported_below_five_scales():
    from imgcomp_cvpr_amd import _lib as L
    assert L.lib.ic_msssim_plan_bytes(320, 160) > 0 and L.lib.ic_msssim_plan_bytes(160, 320) == 0      # pad from the width
    return L.lib.ic_msssim_plan_bytes(16, 16) == 0 and L.lib.ic_msssim_workspace_bytes(1, 3, 16, 64) == 0 and L.lib.ic_msssim_plan_bytes(17, 17) > 0


def test_optimizer_and_schedule(cuda):
    from imgcomp_cvpr_amd import training, config_parser as cp
    ae, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    assert training.learning_rate(ae, 0, 100) == pytest.approx(8e-5)
    assert training.learning_rate(ae, 199, 100) == pytest.approx(8e-5)
    assert training.learning_rate(ae, 200, 100) == pytest.approx(8e-6)      # staircase x0.1 every 2 epochs
    # TF Adam: first step moves every coordinate by ~lr regardless of the gradient's scale
    p = torch.ones(4, device=cuda)
    gr = torch.tensor([1.0, -2.0, 1e-3, 50.0], device=cuda)
    opt = training.TFAdam([p], [gr], lr=0.1)
    opt.step()
    m, v = 0.1 * gr, 0.001 * gr * gr
    lr_t = 0.1 * np.sqrt(1 - 0.999) / (1 - 0.9)
    assert torch.allclose(p, 1 - lr_t * m / (v.sqrt() + 1e-8), atol=1e-6)


def test_two_steps_reduce_loss(cuda):
    """a few optimiser steps on a fixed batch lower the loss (plumbing: grads reach the right variables)."""
    from imgcomp_cvpr_amd import training, config_parser as cp, weights as W
    ae, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    ae.distortion_to_minimize = 'mse'
    ae.lr_initial = 1e-3
    tr = training.Trainer(ae, pc, W.synthetic_weights(ae, pc), cuda, num_itr_per_epoch=1000)
    x = dev(W.synthetic_image((4, 3, 64, 64), 'natural', 2), cuda)
    losses = [tr.step(x)['d_loss_scaled'] for _ in range(6)]
    assert losses[-1] < losses[0], losses
    assert all(np.isfinite(losses))


@pytest.mark.parametrize('kind', ['SGD', 'MOMENTUM'])
def test_trainer_honours_the_configs_optimizer(cuda, kind):
    """ae_configs / pc_configs `optimizer = SGD | MOMENTUM` (training_helpers.py:42-48) reach the trainer: the variables move by
    exactly the rule's update of the step's gradients, the checkpoint carries the rule's slots under the optimiser's NAME
    (`<var>/Adam_AE` for Momentum's accumulator, nothing for SGD, no beta powers), and a restore continues the accumulators."""
    from imgcomp_cvpr_amd import training, config_parser as cp, weights as W
    ae, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    ae.distortion_to_minimize = 'mse'
    ae.optimizer = pc.optimizer = kind
    ae.lr_initial, pc.lr_initial = 1e-5, 2e-5
    wts = W.synthetic_weights(ae, pc)
    tr = training.Trainer(ae, pc, wts, cuda, num_itr_per_epoch=1000)
    assert tr.opt_ae.kind == kind and tr.opt_pc.kind == kind
    x = dev(W.synthetic_image((2, 3, 64, 64), 'natural', 4), cuda)
    n_ae, n_pc = 'autoencoder/decoder/h12/weights', 'probclass3d/logits/res1/conv3d_conv1_mask/weights'
    before = {n: tr.graph.params[n].clone() for n in (n_ae, n_pc)}
    tr.step(x)
    g1 = {n: tr.graph.grads[n].clone() for n in (n_ae, n_pc)}
    mom = 0.9 if kind == 'MOMENTUM' else 0.0
    for n, lr in ((n_ae, 1e-5), (n_pc, 2e-5)):
        want = before[n] - lr * g1[n] - lr * mom * g1[n]          # first step: accum = grad
        assert_close(tr.graph.params[n], want, '{} first step {}'.format(kind, n.split('/')[-2]), 1e-6)
    tr.step(x)
    state = tr.state_weights()
    assert 'beta1_power' not in state and (n_ae + '/Adam_AE_1') not in state
    assert ((n_ae + '/Adam_AE') in state) == (kind == 'MOMENTUM') and ((n_pc + '/Adam_PC') in state) == (kind == 'MOMENTUM')
    tr2 = training.Trainer(ae, pc, {k: v for k, v in state.items() if k in wts}, cuda, num_itr_per_epoch=1000)
    assert tr2.restore_training_state(state) == 2
    o1, o2 = tr.step(x), tr2.step(x)
    assert o1 == o2 and torch.equal(tr.graph.params[n_ae], tr2.graph.params[n_ae])


def _param_digest(tr):
    import hashlib
    h = hashlib.sha1()
    for g in ('pc', 'dec', 'enc'):
        h.update(tr.graph.flat_params[g].detach().cpu().numpy().tobytes())
    return h.hexdigest()


@pytest.mark.parametrize('sync_between_steps', [False, True])
def test_twenty_ms_ssim_steps_range_identity_determinism(cuda, sync_between_steps):
    """the multi-step gate of the training loop (train.py:216-266 runs thousands of steps): 20 optimiser steps of cfg3 (cvpr/med,
    32 crops of 128 x 128, MS-SSIM distortion) on one fixed batch, as `bench.py --mode train` issues them (nothing between the
    steps) and with a device-wide synchronize between them.  Every step: 0 < MS-SSIM <= 1 (Cauchy-Schwarz; round 3 printed 1.157),
    d_loss_scaled == K (1 - MS-SSIM) (train.py:379-390), the loss goes down, and the trajectory -- every step's scalars and the
    variables after the last step, bit for bit -- repeats in a second fresh run and does not depend on the synchronisation."""
    from imgcomp_cvpr_amd import training, config_parser as cp, weights as W
    ae, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'med'))
    pc, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    assert ae.distortion_to_minimize == 'ms_ssim'
    x = dev(W.synthetic_image((32, 3, 128, 128), 'natural', 0), cuda)
    K = float(ae.K_ms_ssim)

    def run(sync):
        tr = training.Trainer(ae, pc, W.synthetic_weights(ae, pc), cuda, num_itr_per_epoch=1000)
        rows = []
        for _ in range(20):
            rows.append(tr.step(x))
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return rows, _param_digest(tr)
    rows, digest = run(sync_between_steps)
    for i, r in enumerate(rows):
        assert 0.0 < r['ms_ssim'] <= 1.0, 'step {}: MS-SSIM {} outside (0, 1]'.format(i, r['ms_ssim'])
        assert abs(r['d_loss_scaled'] - K * (1.0 - r['ms_ssim'])) <= 2e-3 + 1e-6 * K, (i, r)
        assert all(np.isfinite(v) for v in r.values()), (i, r)
    ms = [r['ms_ssim'] for r in rows]
    assert ms[-1] > ms[0] + 0.3, 'twenty Adam steps on one batch must raise MS-SSIM: {}'.format(ms)
    rows2, digest2 = run(sync_between_steps)
    assert rows == rows2 and digest == digest2, 'the trajectory does not repeat'
    rows3, digest3 = run(not sync_between_steps)
    assert rows == rows3 and digest == digest3, 'the trajectory depends on host / device synchronisation'


def test_three_ms_ssim_steps_follow_the_oracle(cuda):
    """steps 1-3 of the loop against oracle/train_oracle.train_steps (autograd + TF-Adam on the CPU): per-step MS-SSIM, rate
    terms and bpp, and the direction every large tensor has moved in.
    Step 1 is compared with the float64 oracle (tight).  From step 2 on the reference is the oracle evaluated in float32: Adam's
    first steps move every coordinate by ~lr * sign(gradient), so the float32 rounding of the gradients (MS-SSIM's
    E[b^2] - mu^2 cancellation scaled by K = 5000 feeds all of them) changes the trajectory visibly -- the float32 oracle itself
    is 1.4e-2 away from the float64 one in MS-SSIM after ONE update (0.4249 vs 0.4103), while the device follows the float32
    oracle within 3e-4.  The float64 distance is recorded in the parity report with that loose bound."""
    from imgcomp_cvpr_amd import training, config_parser as cp, weights as W
    from oracle import train_oracle as T
    ae, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'med'))
    pc, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    ae.H_target = 0.5                                     # keep the rate term active on synthetic weights
    wts = W.synthetic_weights(ae, pc)
    x = W.synthetic_image((8, 3, 64, 64), 'natural', 3)
    torch.set_num_threads(16)
    hist64, _ = T.train_steps(x, wts, ae.as_dict(), pc.as_dict(), 3, torch.float64)
    hist32, final32 = T.train_steps(x, wts, ae.as_dict(), pc.as_dict(), 3, torch.float32)
    tr = training.Trainer(ae, pc, wts, cuda, num_itr_per_epoch=1000)
    xd = dev(x, cuda)
    rows = [tr.step(xd) for _ in range(3)]
    torch.cuda.synchronize()
    from tests import util
    for i, (r, h64, h32) in enumerate(zip(rows, hist64, hist32)):
        assert 0.0 < r['ms_ssim'] <= 1.0
        for k, tol1, tol in (('ms_ssim', 2e-5, 2e-3), ('H_real', 2e-5, 2e-3), ('H_mask', 2e-5, 2e-3), ('bpp', 2e-5, 2e-3)):
            if i == 0:
                e = abs(r[k] - h64[k]) / max(1.0, abs(h64[k]))
                util.REPORT.append(('train step 1 {} vs float64 oracle'.format(k), abs(r[k] - h64[k]), e, tol1))
                assert e <= tol1, 'step 1 {}: {} vs float64 oracle {}'.format(k, r[k], h64[k])
            else:
                e = abs(r[k] - h32[k]) / max(1.0, abs(h32[k]))
                util.REPORT.append(('train step {} {} vs float32 oracle'.format(i + 1, k), abs(r[k] - h32[k]), e, tol))
                assert e <= tol, 'step {} {}: {} vs float32 oracle {}'.format(i + 1, k, r[k], h32[k])
                e64 = abs(r[k] - h64[k]) / max(1.0, abs(h64[k]))
                util.REPORT.append(('train step {} {} vs float64 oracle (float32 oracle: {:.1e})'.format(
                    i + 1, k, abs(h32[k] - h64[k]) / max(1.0, abs(h64[k]))), abs(r[k] - h64[k]), e64, 5e-2))
                assert e64 <= 5e-2
        K = float(ae.K_ms_ssim)
        assert abs(r['d_loss_scaled'] - K * (1.0 - r['ms_ssim'])) <= 2e-3 + 1e-6 * K
    for n in ('autoencoder/encoder/h2/weights', 'autoencoder/encoder/res_block_enc_2/enc_2_2/conv1/weights',
              'autoencoder/decoder/res_block_dec_0/dec_0_1/conv1/weights', 'autoencoder/decoder/h12/weights',
              'probclass3d/logits/res1/conv3d_conv1_mask/weights'):
        d_dev = tr.graph.params[n].detach().double().cpu().numpy().ravel() - np.asarray(wts[n], np.float64).ravel()
        d_ref = final32[n].ravel() - np.asarray(wts[n], np.float64).ravel()
        cos = float(d_dev @ d_ref / (np.linalg.norm(d_dev) * np.linalg.norm(d_ref)))
        util.REPORT.append(('train 3 steps displacement cosine ' + n.replace('autoencoder/', 'ae/'), 1.0 - cos, 1.0 - cos, 0.1))
        assert cos > 0.9, '{}: cosine {} between the device and the float32 oracle displacement after 3 steps'.format(n, cos)


def test_train_entry_point(cuda, tmp_path):
    """python -m imgcomp_cvpr_amd.train on synthetic crops: runs, logs, writes TF-1 bundle checkpoints + var_names.pkl
    in the reference's ckpts/ layout; val.py restores the newest / a given iteration; --restore continues from them."""
    from imgcomp_cvpr_amd import train, config_parser as cp, val, autoencoder
    ae_p = cp.builtin_config_path('ae_configs', 'cvpr', 'low')
    pc_p = cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow')
    ae_over = tmp_path / 'ae_configs' / 'tiny'
    ae_over.parent.mkdir()
    ae_over.write_text('use {}\nbatch_size = 4\ncrop_size = (64, 64)\ndistortion_to_minimize = mse\n'.format(ae_p))

    def loader_fn(ae_config, batch, rank):
        return train.CropLoader(None, ae_config.crop_size, batch, seed=rank, synthetic=True)
    tr, hist, log_dir = train.train(str(ae_over), pc_p, str(tmp_path / 'logs'), loader_fn, max_itr=3, log_interval=1,
                                    save_interval=2, device=str(cuda), verbose=False)
    assert len(hist) == 3 and all(np.isfinite(h['d_loss_scaled']) for h in hist)
    from imgcomp_cvpr_amd import tf_checkpoint as T
    ckpts = os.path.join(log_dir, 'ckpts')
    assert sorted(os.listdir(ckpts)) == ['ckpt-2.data-00000-of-00001', 'ckpt-2.index', 'ckpt-3.data-00000-of-00001',
                                         'ckpt-3.index', 'var_names.pkl']
    assert [i for i, _ in T.all_ckpts_with_iterations(ckpts)] == [2, 3]
    assert int(T.read_bundle(os.path.join(ckpts, 'ckpt-3'), names=['global_step'], verify=True)['global_step']) == 3
    wts = val.load_weights_for_job(log_dir, None, tr.graph.ae_config, tr.graph.pc_config)
    assert set(wts) == set(tr.graph.params)
    final = tr.state_weights()
    assert all(np.array_equal(wts[k], final[k]) for k in wts)
    w2 = val.load_weights_for_job(log_dir, None, tr.graph.ae_config, tr.graph.pc_config, restore_itr=2)
    assert any(not np.array_equal(w2[k], final[k]) for k in w2)              # the earlier checkpoint
    tr2, hist2, _ = train.train(str(ae_over), pc_p, None, loader_fn, max_itr=1, restore=log_dir, device=str(cuda), verbose=False)
    assert np.isfinite(hist2[0]['d_loss_scaled'])
    assert tr2.global_step == 4 and tr2.opt_ae.t == 4                          # continued: step counter and Adam's beta powers
    # the reference's restore flags (restore_manager.py:23-58): an iteration, --from_identity (no global_step, no *Adam*),
    # --restore_continue (same log dir), and the test-in-train evaluation every --log_interval_test iterations
    tr3, hist3, ld3 = train.train(str(ae_over), pc_p, str(tmp_path / 'logs'), loader_fn, max_itr=2, restore=log_dir, restore_itr=2,
                                  restore_continue=True, device=str(cuda), verbose=False, log_interval_test=1)
    assert ld3 == log_dir and tr3.global_step == 4
    assert all(np.isfinite(h['test_bpp']) and np.isfinite(h['test_psnr']) for h in hist3)
    assert hist3[0]['test_bpp'] != hist3[1]['test_bpp'], 'test-in-train did not see the updated variables'
    tr4, _, _ = train.train(str(ae_over), pc_p, None, loader_fn, max_itr=1, from_identity=log_dir, device=str(cuda), verbose=False)
    assert tr4.global_step == 1 and tr4.opt_ae.t == 1 and float(tr4.opt_ae.m[0].abs().max()) > 0
    with pytest.raises(ValueError):
        train.train(str(ae_over), pc_p, None, loader_fn, max_itr=1, restore=os.path.join(str(tmp_path), 'nope'), device=str(cuda), verbose=False)
    ae = autoencoder.get_network_cls(tr.graph.ae_config)(tr.graph.ae_config).load_weights(wts, cuda)
    enc = ae.encode(torch.zeros((1, 3, 64, 64), device=cuda), is_training=False)       # inference on the trained variables
    assert bool(torch.isfinite(enc.z).all())


def test_gradient_buckets_over_rccl_single_rank(cuda, configs, syn_weights):
    """the RCCL path on the real device: a one-rank `nccl` process group, every bucket all-reduced asynchronously while
    backward continues (stream ordering between the HIP kernels on torch's current stream and RCCL's stream) -- the
    gradients must equal those of the run without any exchange."""
    import torch.distributed as dist
    from imgcomp_cvpr_amd import training, weights as W
    ae_cfg, pc_cfg = configs
    x = dev(W.synthetic_image((4, 3, 64, 64), 'natural', seed=5), cuda)
    g0 = training.TrainGraph(ae_cfg, pc_cfg, syn_weights, device=str(cuda))
    g0.forward_backward(x)
    ref = {k: v.clone() for k, v in g0.flat_grads.items()}
    if not dist.is_initialized():
        dist.init_process_group('nccl', init_method='tcp://127.0.0.1:29531', rank=0, world_size=1,
                                device_id=torch.device(cuda))
    try:
        g1 = training.TrainGraph(ae_cfg, pc_cfg, syn_weights, device=str(cuda))
        g1.buckets.always_reduce = True
        out = g1.forward_backward(x)
        torch.cuda.synchronize()
        assert np.isfinite(out['d_loss_scaled'])
        for k in ref:
            assert torch.equal(g1.flat_grads[k], ref[k]), k
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('Cin,Cout,relu_mask,with_res', [(24, 24, True, True), (24, 6, False, False), (24, 24, True, False),
                                                         (64, 64, True, True), (64, 6, False, False)])
def test_pc_data_gradient_matrix_core_path(cuda, Cin, Cout, relu_mask, with_res):
    """data gradient of a masked conv3d layer: the matrix-core path (adjoint layer: mirrored taps, transposed filter,
    zero-padded gradient) against torch autograd in float64 and against the any-shape VALU kernel."""
    import torch.nn.functional as F
    from oracle import oracle as O
    L = _L()
    rs = np.random.RandomState(Cin + Cout)
    N, OD, OH, OW = 2, 3, 9, 21
    g = rs.normal(0, 1, (N, Cout, OD, OH, OW)).astype(np.float32)
    w = rs.normal(0, 0.1, (2, 3, 3, Cin, Cout)).astype(np.float32)
    act = rs.normal(0, 1, (N, Cin, OD + 1, OH + 2, OW + 2)).astype(np.float32)
    res = rs.normal(0, 1, (N, Cin, OD - 1, OH - 2, OW - 2)).astype(np.float32)
    _, other = O.pc_masks(3)
    xt = torch.zeros((N, Cin, OD + 1, OH + 2, OW + 2), dtype=torch.float64, requires_grad=True)
    wm = (torch.as_tensor(w).double() * torch.as_tensor(other, dtype=torch.float64)[..., None, None]).permute(4, 3, 0, 1, 2)
    F.conv3d(xt, wm).backward(torch.as_tensor(g).double())
    ref = xt.grad.clone()
    if with_res:
        ref[:, :, 2:2 + OD - 1, 2:2 + OH - 2, 2:2 + OW - 2] += torch.as_tensor(res).double()
    if relu_mask:
        ref = ref * (torch.as_tensor(act) > 0)
    d = lambda a: dev(a, cuda)
    gd, wd_, actd, resd = d(g), d(w), d(act), d(res)
    outs = []
    need = L.lib.ic_pc_bwd_data_workspace_bytes(N, Cin, Cout, OD, OH, OW)
    assert need > 0
    for use_ws in (True, False):
        dx = torch.full((N, Cin, OD + 1, OH + 2, OW + 2), float('nan'), device=cuda)
        ws = torch.empty(need, dtype=torch.uint8, device=cuda) if use_ws else None
        L.check(L.lib.ic_pc_bwd_data_f32(L.ptr(gd), L.ptr(wd_), L.ptr(resd) if with_res else None,
                                         L.ptr(actd) if relu_mask else None, L.ptr(dx), N, Cin, Cout, OD, OH, OW, 0,
                                         int(relu_mask), L.ptr(ws), need if use_ws else 0, L.current_stream()))
        torch.cuda.synchronize()
        assert_close(dx, ref, 'pc data gradient, matrix cores {}'.format(use_ws), 1e-5)
        outs.append(dx)
    assert not torch.equal(outs[0], outs[1])          # really two different kernels
    assert L.lib.ic_pc_bwd_data_workspace_bytes(N, 8, 24, OD, OH, OW) == 0      # uncovered shape -> VALU kernel only


def test_reference_training_call_sites(cuda):
    """code/train.py:101-127 ported line by line onto the plugin surface: ae.encode(x, True), ae.decode(enc.qbar, True),
    pc.bitcost(stop_gradient(qbar), symbols, True, pad_value), Distortions, get_loss, backward of total_loss; then the
    test-in-train evaluation with is_training=False on the SAME (training) variables.  The gradients must equal those of
    TrainGraph.forward_backward bit for bit (one code path), and the inference calls must follow the optimiser's updates."""
    from imgcomp_cvpr_amd import autoencoder, probclass, bits, training, config_parser as cp, weights as W
    ae_config, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc_config, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    ae_config.distortion_to_minimize = 'mse'
    ae_config.H_target = 0.5
    wts = W.synthetic_weights(ae_config, pc_config)
    x_train = dev(W.synthetic_image((2, 3, 64, 64), 'natural', 3), cuda)
    x_test = dev(W.synthetic_image((1, 3, 64, 96), 'natural', 4), cuda)
    # reference run: the monolithic step
    g_ref = training.TrainGraph(ae_config, pc_config, wts, cuda)
    out_ref = g_ref.forward_backward(x_train)
    # ---- train.py:86-106 ----
    ae_cls = autoencoder.get_network_cls(ae_config)
    pc_cls = probclass.get_network_cls(pc_config)
    ae = ae_cls(ae_config)
    pc = pc_cls(pc_config, num_centers=ae_config.num_centers)
    with pytest.raises(ValueError):
        ae.encode(x_train, is_training=True)                       # no graph owns the variables yet
    trainer = training.Trainer(ae_config, pc_config, wts, cuda, num_itr_per_epoch=1000)
    trainer.graph.bind(ae, pc)                                      # (TF: the variable store + the gradient graph)
    enc_out_train = ae.encode(x_train, is_training=True)            # qbar is masked by the heatmap
    x_out_train = ae.decode(enc_out_train.qbar, is_training=True)
    pc_in = enc_out_train.qbar.detach()                             # tf.stop_gradient
    bc_train = pc.bitcost(pc_in, enc_out_train.symbols, is_training=True, pad_value=pc.auto_pad_value(ae))
    bpp_train = bits.bitcost_to_bpp(bc_train, x_train)
    d_train = training.Distortions(ae_config, x_train, x_out_train, is_training=True)
    total_loss, H_real, pc_comps, ae_comps = training.get_loss(ae_config, ae, pc, d_train.d_loss_scaled, bc_train,
                                                                enc_out_train.heatmap)
    total_loss.backward()
    trainer.graph.finish_backward()
    torch.cuda.synchronize()
    for k in g_ref.flat_grads:
        assert torch.equal(trainer.graph.flat_grads[k], g_ref.flat_grads[k]), 'bucket {} differs from forward_backward'.format(k)
    assert float(d_train.d_loss_scaled) == out_ref['d_loss_scaled'] and float(dict(pc_comps)['pc_loss']) == out_ref['pc_loss']
    assert abs(float(bpp_train) - out_ref['bpp']) < 1e-6
    assert abs(float(dict(ae_comps)['reg_enc_dec']) + float(dict(pc_comps)['reg']) - trainer.graph.regularization_loss()) < 1e-4
    assert float(total_loss) > float(d_train.d_loss_scaled)          # distortion + rate + regularisers
    # ---- train.py:115-127: test-in-train on the training variables ----
    def evaluate():
        enc_out_test = ae.encode(x_test, is_training=False)
        x_out_test = ae.decode(enc_out_test.qhard, is_training=False)
        bc_test = pc.bitcost(enc_out_test.qhard, enc_out_test.symbols, is_training=False, pad_value=pc.auto_pad_value(ae))
        return x_out_test.clone(), float(bits.bitcost_to_bpp(bc_test, x_test)), training.Distortions(ae_config, x_test, x_out_test, False)
    xo0, bpp0, d0 = evaluate()
    ref_ae = ae_cls(ae_config).load_weights(trainer.state_weights(training_state=False), cuda)
    assert torch.equal(xo0, ref_ae.decode(ref_ae.encode(x_test, False).qhard, False)), 'inference on a bound object != a fresh load'
    assert np.isfinite(float(d0.psnr)) and d0.ms_ssim is None and 0 < bpp0 < 10
    trainer.apply_gradients()                                        # get_train_op: both Adam updates
    xo1, bpp1, _ = evaluate()
    assert not torch.equal(xo0, xo1) and bpp0 != bpp1, 'is_training=False did not pick up the updated variables'
    assert float(pc.auto_pad_value(ae)) == float(trainer.graph.params['autoencoder/encoder/centers'][0])
    # continuing a run: global_step and the Adam slots travel through a checkpoint
    state = trainer.state_weights()
    assert int(state['global_step']) == 1 and 'autoencoder/encoder/h1/weights/Adam_AE_1' in state and 'beta2_power_1' in state and 'beta1_power' in state
    tr2 = training.Trainer(ae_config, pc_config, {k: v for k, v in state.items() if k in wts}, cuda, num_itr_per_epoch=1000)
    assert tr2.restore_training_state(state) == 1 and tr2.opt_ae.t == 1 and tr2.opt_pc.t == 1
    a = trainer.step(x_train)
    b = tr2.step(x_train)
    assert a == b, 'a restored run does not continue like the original'
    for n, t in trainer.graph.params.items():
        assert torch.equal(t, tr2.graph.params[n]), n


def test_sync_bn_halves_equal_full_batch(cuda):
    """The cross-replica BatchNorm entry points on one device: the float64 moments of two half batches, summed (what the
    all-reduce does), give the statistics, the output and the data gradient of the full batch -- the full-batch fused calls
    are reproduced to fp32 rounding, the one-rank split path bit for bit."""
    L = _L()
    rs = np.random.RandomState(4)
    N, C, H, W = 4, 37, 6, 10
    x = dev(rs.normal(0.3, 2.0, (N, C, H, W)), cuda)
    dy = dev(rs.normal(0, 1, (N, C, H, W)), cuda)
    gamma, beta = dev(rs.uniform(0.5, 1.5, C), cuda), dev(rs.normal(0, 0.3, C), cuda)
    ws = torch.empty(L.lib.ic_bn_workspace_bytes(C), dtype=torch.uint8, device=cuda)
    st = L.current_stream()
    mk = lambda: torch.empty(C, device=cuda)
    for relu in (0, 1):
        mm0, mv0 = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
        mean, invstd, scale, shift = mk(), mk(), mk(), mk()
        L.check(L.lib.ic_bn_train_stats_f32(L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(mm0), L.ptr(mv0), 0.9, 1e-5, L.ptr(mean), L.ptr(invstd),
                                            L.ptr(scale), L.ptr(shift), N, C, H * W, L.ptr(ws), st))
        dx_ref, dg_ref, db_ref = torch.empty_like(x), mk(), mk()
        L.check(L.lib.ic_bn_backward_f32(L.ptr(dy), L.ptr(x), L.ptr(scale), L.ptr(shift), L.ptr(mean), L.ptr(invstd), L.ptr(gamma),
                                         L.ptr(dx_ref), L.ptr(dg_ref), L.ptr(db_ref), N, C, H * W, relu, L.ptr(ws), st))
        for parts in (1, 2):
            n = N // parts
            xs, dys = [x[i * n:(i + 1) * n].contiguous() for i in range(parts)], [dy[i * n:(i + 1) * n].contiguous() for i in range(parts)]
            sums = torch.zeros(2 * C, dtype=torch.float64, device=cuda)
            for xi in xs:
                part = torch.empty(2 * C, dtype=torch.float64, device=cuda)
                L.check(L.lib.ic_bn_moments_f32(L.ptr(xi), L.ptr(part), n, C, H * W, L.ptr(ws), st))
                sums += part
            mm1, mv1 = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
            m2, i2, s2, h2 = mk(), mk(), mk(), mk()
            L.check(L.lib.ic_bn_train_fold_moments_f32(L.ptr(sums), N * H * W, L.ptr(gamma), L.ptr(beta), L.ptr(mm1), L.ptr(mv1), 0.9, 1e-5,
                                                       L.ptr(m2), L.ptr(i2), L.ptr(s2), L.ptr(h2), C, st))
            gsums = torch.zeros(2 * C, dtype=torch.float64, device=cuda)
            dgs, dbs = [], []
            for xi, dyi in zip(xs, dys):
                part, dg, db = torch.empty(2 * C, dtype=torch.float64, device=cuda), mk(), mk()
                L.check(L.lib.ic_bn_backward_reduce_f32(L.ptr(dyi), L.ptr(xi), L.ptr(s2), L.ptr(h2), L.ptr(m2), L.ptr(i2), L.ptr(part), L.ptr(dg),
                                                        L.ptr(db), n, C, H * W, relu, L.ptr(ws), st))
                gsums += part
                dgs.append(dg)
                dbs.append(db)
            dxs = []
            for xi, dyi in zip(xs, dys):
                dxi = torch.empty_like(xi)
                L.check(L.lib.ic_bn_backward_apply_f32(L.ptr(dyi), L.ptr(xi), L.ptr(s2), L.ptr(h2), L.ptr(m2), L.ptr(i2), L.ptr(gamma), L.ptr(gsums),
                                                       N * H * W, L.ptr(dxi), n, C, H * W, relu, st))
                dxs.append(dxi)
            torch.cuda.synchronize()
            dx = torch.cat(dxs, 0)
            if parts == 1:
                for a, b in ((m2, mean), (i2, invstd), (s2, scale), (h2, shift), (mm1, mm0), (mv1, mv0), (dx, dx_ref), (dgs[0], dg_ref), (dbs[0], db_ref)):
                    assert torch.equal(a, b), 'the split path on one rank is not the fused path'
            else:
                assert_close(m2, mean, 'sync bn mean', 1e-6)
                assert_close(s2, scale, 'sync bn scale', 1e-6)
                assert_close(mv1, mv0, 'sync bn moving variance', 1e-6)
                assert_close(dx, dx_ref, 'sync bn dx', 1e-6)
                assert_close(dgs[0] + dgs[1], dg_ref, 'sync bn dgamma (sum over ranks)', 1e-6)
                assert_close(dbs[0] + dbs[1], db_ref, 'sync bn dbeta (sum over ranks)', 1e-6)


def _two_rank_worker(rank, world, port, x_np, wts, ae_over, sync_bn, out_q):
    import os
    import torch.distributed as dist
    from imgcomp_cvpr_amd import training, config_parser as cp
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)       # both ranks share the one GPU of the box: RCCL needs a device per rank
    try:
        ae, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
        pc, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
        for k, v in ae_over.items():
            setattr(ae, k, v)
        g = training.TrainGraph(ae, pc, wts, 'cuda:0', sync_bn=sync_bn)
        n = x_np.shape[0] // world
        x = torch.as_tensor(x_np[rank * n:(rank + 1) * n]).float().cuda()
        out = g.forward_backward(x)
        torch.cuda.synchronize()
        if rank == 0:
            out_q.put(({k: v.cpu().numpy() for k, v in g.flat_grads.items()}, out,
                       g.params['autoencoder/encoder/h2/BatchNorm/moving_variance'].cpu().numpy()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_rank_training_step_equals_single_rank(cuda):
    """BASELINE configs[2] splits one batch over the GPUs of a node.  Two ranks (two processes sharing this box's one GPU,
    gloo for the collectives) with batch 2 each and cross-replica BatchNorm must produce, after the gradient all-reduce,
    the gradients of ONE rank running the whole batch of 4 -- the reference's single-device semantics (autoencoder.py:115-125).
    With local statistics (sync_bn=False) they must not."""
    import torch.multiprocessing as mp
    from imgcomp_cvpr_amd import training, config_parser as cp, weights as W
    ae, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    over = {'distortion_to_minimize': 'mse', 'H_target': 0.5}
    for k, v in over.items():
        setattr(ae, k, v)
    wts = W.synthetic_weights(ae, pc)
    x_np = W.synthetic_image((4, 3, 64, 64), 'natural', 9)
    g = training.TrainGraph(ae, pc, wts, cuda)
    out1 = g.forward_backward(dev(x_np, cuda))
    torch.cuda.synchronize()
    ref = {k: v.cpu().numpy() for k, v in g.flat_grads.items()}
    ref_mv = g.params['autoencoder/encoder/h2/BatchNorm/moving_variance'].cpu().numpy()
    ctx = mp.get_context('spawn')
    results = {}
    for sync_bn, port in ((True, 29541), (False, 29542), ('p2p', 29543)):
        q = ctx.Queue()
        procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, x_np, wts, over, sync_bn, q)) for r in range(2)]
        for p_ in procs:
            p_.start()
        results[sync_bn] = q.get(timeout=600)
        for p_ in procs:
            p_.join(timeout=120)
            assert p_.exitcode == 0
    grads, out2, mv = results[True]
    worst = max(true_rel_err(torch.as_tensor(grads[k]), torch.as_tensor(ref[k]).double()) for k in ref)
    assert worst < 5e-5, 'sync BatchNorm: 2 x 2 != 1 x 4, worst bucket error {:.3e}'.format(worst)
    assert np.allclose(mv, ref_mv, rtol=1e-5, atol=1e-7)               # the moving averages see the whole batch too
    assert abs(out2['pc_loss'] - out1['pc_loss']) < 5e-2 * abs(out1['pc_loss']) + 1e-3      # (losses are per-rank means over half the batch)
    # the hand-written exchange over peer-mapped memory (peer.py) sums the same float64 moments in rank order: same result
    grads_p, _, mv_p = results['p2p']
    worst_p = max(true_rel_err(torch.as_tensor(grads_p[k]), torch.as_tensor(ref[k]).double()) for k in ref)
    assert worst_p < 5e-5 and np.allclose(mv_p, ref_mv, rtol=1e-5, atol=1e-7), 'p2p sync BatchNorm: worst bucket error {:.3e}'.format(worst_p)
    assert all(np.array_equal(grads_p[k], grads[k]) for k in ref), 'p2p exchange and all-reduce disagree (both sum in rank order)'
    grads_l, _, mv_l = results[False]
    worst_l = max(true_rel_err(torch.as_tensor(grads_l[k]), torch.as_tensor(ref[k]).double()) for k in ref)
    assert worst_l > 10 * worst and not np.allclose(mv_l, ref_mv, rtol=1e-5), 'local statistics reproduce the full batch?'


def test_inference_pad_value_follows_the_optimiser(cuda):
    """the context model's pad value is centers[0] (probclass.py:59-61), a by-value argument of the C ABI that the
    plugin object caches on the host.  The optimiser updates the centres through a raw pointer -- neither the storage nor
    torch's version counter changes -- so the cache must follow the training graph's version, and an unbound object's cache
    must not survive a load_weights whose new centres land on the recycled address."""
    from imgcomp_cvpr_amd import autoencoder, probclass, training, config_parser as cp, weights as W
    ae_config, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc_config, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    ae_config.distortion_to_minimize = 'mse'
    ae_config.H_target = 0.5
    wts = W.synthetic_weights(ae_config, pc_config)
    x = dev(W.synthetic_image((2, 3, 64, 64), 'natural', 3), cuda)
    ae = autoencoder.get_network_cls(ae_config)(ae_config)
    pc = probclass.get_network_cls(pc_config)(pc_config, num_centers=ae_config.num_centers)
    trainer = training.Trainer(ae_config, pc_config, wts, cuda, num_itr_per_epoch=1000)
    trainer.graph.bind(ae, pc)
    enc = ae.encode(x, is_training=False)
    used = []
    for _ in range(3):
        pv = pc._pad_value_as_float(pc.auto_pad_value(ae))
        c0 = float(trainer.graph.params['autoencoder/encoder/centers'][0])
        assert pv == c0, 'inference bitcost pads with {} while centers[0] is {}'.format(pv, c0)
        # ... and that value is what the kernel sees: the tensor form and the by-value form give the same bits
        b_t = pc.bitcost(enc.qhard, enc.symbols, is_training=False, pad_value=pc.auto_pad_value(ae))
        b_f = pc.bitcost(enc.qhard, enc.symbols, is_training=False, pad_value=c0)
        assert torch.equal(b_t, b_f)
        used.append(pv)
        trainer.step(x)
    assert len(set(used)) == 3, 'centers[0] did not move in three optimiser steps: the test would not notice a stale cache'
    # unbound objects: a fresh set of centres (same shape: the allocator may hand out the same address, version 0 again)
    ae2 = autoencoder.get_network_cls(ae_config)(ae_config).load_weights(wts, cuda)
    pc2 = probclass.get_network_cls(pc_config)(pc_config, num_centers=ae_config.num_centers).load_weights(wts, cuda)
    assert pc2._pad_value_as_float(pc2.auto_pad_value(ae2)) == float(wts['autoencoder/encoder/centers'][0])
    w2 = dict(wts)
    w2['autoencoder/encoder/centers'] = (wts['autoencoder/encoder/centers'] + 0.125).astype(np.float32)
    ae2.load_weights(w2, cuda)
    assert pc2._pad_value_as_float(pc2.auto_pad_value(ae2)) == float(w2['autoencoder/encoder/centers'][0])


def _peer_worker(rank, world, port, backend, device_index, out_q):
    import torch.distributed as dist
    from imgcomp_cvpr_amd import peer
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.cuda.set_device(device_index)
    dev_ = torch.device('cuda', device_index)
    if backend == 'nccl':
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev_)
    else:
        dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        px = peer.PeerExchange(dev_)
        ok = True
        last = None
        for it in range(200):
            n = 1 + (it * 37) % px.max_values
            t = torch.arange(n, dtype=torch.float64, device=dev_) * (rank + 1) + it * 0.5 + rank * 1e-3
            want = sum(torch.arange(n, dtype=torch.float64) * (r + 1) + it * 0.5 + r * 1e-3 for r in range(world))
            px.allreduce_f64(t)
            if it % 20 == 0:
                px.check_status()                          # a time-out ends the test at once instead of 200 bounded spins
            got = t.cpu()
            ok = ok and bool(torch.equal(got, want))       # float64 sums in rank order: exactly the host's sum in the same order
            last = got
        px.check_status()
        out_q.put((rank, ok, last.numpy()))
        dist.barrier()
        px.close()
    finally:
        dist.destroy_process_group()


def _run_peer(world, backend, devices, port):
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_peer_worker, args=(r, world, port, backend, devices[r], q)) for r in range(world)]
    for p_ in procs:
        p_.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    for p_ in procs:
        p_.join(timeout=120)
        assert p_.exitcode == 0
    assert all(ok for _, ok, _ in res), 'a peer exchange returned a wrong sum'
    assert all(np.array_equal(res[0][2], r[2]) for r in res), 'ranks hold different sums'


def test_peer_exchange_two_processes_one_gpu(cuda):
    """csrc/peer_exchange.hip between two PROCESSES (inter-process memory handles, flags, slot rotation, 200 exchanges of varying
    length): both ranks on this box's one GPU -- the protocol and the mapping are the ones used between GPUs, the fabric is not."""
    _run_peer(2, 'gloo', [0, 0], 29551)


def test_peer_exchange_timeout_sets_status_not_a_fault(cuda):
    """the time-out path of csrc/peer_exchange.hip (round 3 shipped it as a null store): rank 0 of a world of two exchanges
    while rank 1 never calls -- the bounded spin must end, raise the status word, leave the values as they were, and the device
    must stay usable; the late rank's call with the same sequence number then completes with the right sums.  Both regions live
    in this process (a region pointer is a region pointer to the kernel).  NULL status is refused by the ABI."""
    import ctypes
    from imgcomp_cvpr_amd import _lib as L
    lib = L.lib
    regs = (ctypes.c_void_p * 2)()
    handles = []
    for r in range(2):
        own, h = ctypes.c_void_p(), (ctypes.c_ubyte * 64)()
        L.check(lib.ic_peer_region_create(ctypes.byref(own), h))
        regs[r] = own
        handles.append(own)
    st = L.current_stream(cuda)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    v0 = torch.arange(5, dtype=torch.float64, device=cuda) + 1.0
    keep = v0.clone()
    assert lib.ic_peer_allreduce_f64_bounded(L.ptr(v0), 5, regs, 0, 2, 1, 2000, None, st) != 0, 'NULL status must be refused'
    assert lib.ic_peer_allreduce_f64(L.ptr(v0), 5, regs, 0, 2, 1, None, st) != 0
    L.check(lib.ic_peer_allreduce_f64_bounded(L.ptr(v0), 5, regs, 0, 2, 1, 2000, L.ptr(status), st))
    torch.cuda.synchronize()                                  # a memory fault would surface here
    assert int(status.item()) == 1, 'the time-out did not raise the status word'
    assert torch.equal(v0, keep), 'a timed-out exchange must leave the local values unchanged'
    # the late rank: rank 0's contribution and flag for sequence 1 are in its region already
    status.zero_()
    v1 = torch.arange(5, dtype=torch.float64, device=cuda) * 10.0
    L.check(lib.ic_peer_allreduce_f64_bounded(L.ptr(v1), 5, regs, 1, 2, 1, 2000, L.ptr(status), st))
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert torch.equal(v1, keep + torch.arange(5, dtype=torch.float64, device=cuda) * 10.0)
    for h in handles:
        lib.ic_peer_region_destroy(h)


def _peer_timeout_worker(rank, world, port, device_index, out_q):
    import torch.distributed as dist
    from imgcomp_cvpr_amd import peer, _lib as L
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.cuda.set_device(device_index)
    dev_ = torch.device('cuda', device_index)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        # exchange 1 with the library's default bound (seconds): the two processes share ONE GPU here and a process's first launch of
        # the kernel also loads its code object -- with the short bound of exchange 2 rank 0 gave up on a rank 1 that was merely
        # late, once in five full runs of round 5 (the failure this test is NOT about)
        px = peer.PeerExchange(dev_, spin_limit=0)
        t = torch.ones(8, dtype=torch.float64, device=dev_) * (rank + 1)
        px.allreduce_f64(t)                                   # exchange 1: both ranks
        px.check_status()
        dist.barrier()
        px.spin_limit = 5000                                  # (read per call)
        raised = None
        if rank == 0:
            u = torch.ones(8, dtype=torch.float64, device=dev_)
            px.allreduce_f64(u)                               # exchange 2: rank 1 never arrives
            try:
                px.check_status()
                raised = False
            except L.HipLibraryError:
                raised = True
            ok = raised and bool(torch.equal(u, torch.ones(8, dtype=torch.float64, device=dev_)))
        else:
            ok = True
        out_q.put((rank, ok and bool(torch.equal(t.cpu(), torch.full((8,), 3.0, dtype=torch.float64)))))
        dist.barrier()
        px.close()
    finally:
        dist.destroy_process_group()


def test_peer_exchange_missing_rank_raises_in_check_status(cuda):
    """PeerExchange between two processes on this GPU: one rank skips an exchange -> the other's check_status() raises
    HipLibraryError (peer.py:61-64), no GPU fault, and the process group is still usable for the closing barrier."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_peer_timeout_worker, args=(r, 2, 29557, 0, q)) for r in range(2)]
    for p_ in procs:
        p_.start()
    res = dict(q.get(timeout=300) for _ in range(2))
    for p_ in procs:
        p_.join(timeout=120)
        assert p_.exitcode == 0
    assert res == {0: True, 1: True}, res


def test_peer_exchange_between_gpus(cuda):
    """the same between real GPUs over xGMI, one process per GPU (RCCL process group for the handle exchange).  Self-skipping:
    gpurun boxes have one GPU; the driver's multi-GPU node runs it."""
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip('needs >= 2 GPUs (have {})'.format(n))
    w = min(n, 8)
    _run_peer(w, 'nccl', list(range(w)), 29552)


def _sync_bn_rccl_worker(rank, world, port, x_np, wts, ae_over, mode, out_q):
    import torch.distributed as dist
    from imgcomp_cvpr_amd import training, config_parser as cp
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.cuda.set_device(rank)
    dev_ = torch.device('cuda', rank)
    dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev_)
    try:
        ae, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
        pc, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
        for k, v in ae_over.items():
            setattr(ae, k, v)
        g = training.TrainGraph(ae, pc, wts, dev_, sync_bn=mode)
        n = x_np.shape[0] // world
        g.forward_backward(torch.as_tensor(x_np[rank * n:(rank + 1) * n]).float().to(dev_))
        torch.cuda.synchronize()
        if rank == 0:
            out_q.put({k: v.cpu().numpy() for k, v in g.flat_grads.items()})
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_sync_bn_over_rccl_and_p2p_between_gpus(cuda):
    """cross-replica BatchNorm where it runs in production: one process per GPU, RCCL gradient buckets, the moments exchanged by
    RCCL all-reduce (sync_bn=True) and by the peer-memory kernel (sync_bn='p2p') -- both must reproduce the single-rank step on
    the whole batch.  Self-skipping below two GPUs."""
    if torch.cuda.device_count() < 2:
        pytest.skip('needs >= 2 GPUs')
    import torch.multiprocessing as mp
    from imgcomp_cvpr_amd import training, config_parser as cp, weights as W
    ae, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'low'))
    pc, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', 'res_shallow'))
    over = {'distortion_to_minimize': 'mse', 'H_target': 0.5}
    for k, v in over.items():
        setattr(ae, k, v)
    wts = W.synthetic_weights(ae, pc)
    x_np = W.synthetic_image((4, 3, 64, 64), 'natural', 9)
    g = training.TrainGraph(ae, pc, wts, cuda)
    g.forward_backward(dev(x_np, cuda))
    torch.cuda.synchronize()
    ref = {k: v.cpu().numpy() for k, v in g.flat_grads.items()}
    ctx = mp.get_context('spawn')
    for mode, port in ((True, 29571), ('p2p', 29572)):
        q = ctx.Queue()
        procs = [ctx.Process(target=_sync_bn_rccl_worker, args=(r, 2, port, x_np, wts, over, mode, q)) for r in range(2)]
        for p_ in procs:
            p_.start()
        grads = q.get(timeout=600)
        for p_ in procs:
            p_.join(timeout=120)
            assert p_.exitcode == 0
        worst = max(true_rel_err(torch.as_tensor(grads[k]), torch.as_tensor(ref[k]).double()) for k in ref)
        assert worst < 5e-5, 'sync_bn={!r} over {} GPUs: worst bucket error {:.3e}'.format(mode, 2, worst)
