"""-m gpu: every C-ABI op of libimgcomp_hip.so against the CPU oracle on seeded inputs."""
import zlib

import numpy as np
import pytest
import torch

from tests.util import RTOL, assert_close, dev, rel_err

pytestmark = pytest.mark.gpu


def _lib():
    from imgcomp_cvpr_amd import _lib
    return _lib


def _bn(rs, c):
    scale = rs.uniform(0.5, 1.5, c).astype(np.float32)
    shift = rs.normal(0, 0.3, c).astype(np.float32)
    return scale, shift


def _ref_conv(x, w, scale, shift, stride, relu, transposed=False, res=(), norm=False, denorm=False):
    from oracle import oracle as O
    xt = torch.as_tensor(x).double()
    if norm:
        xt = O.normalize(xt)
    y = O.conv2d_transpose_same(xt, w, 2) if transposed else O.conv2d_same(xt, w, stride)
    y = y * torch.as_tensor(scale).double().view(1, -1, 1, 1) + torch.as_tensor(shift).double().view(1, -1, 1, 1)
    if relu:
        y = torch.relu(y)
    for r in res:
        y = y + torch.as_tensor(r).double()
    if denorm:
        y = torch.clamp(O.denormalize(y), 0, 255)
    return y


@pytest.mark.parametrize('name,N,Cin,H,W,Cout,K,stride,relu,norm', [
    ('h1', 1, 3, 40, 56, 64, 5, 2, 1, True),
    ('h1_odd', 2, 3, 37, 71, 64, 5, 2, 1, True),
    ('h1_wide', 1, 3, 18, 150, 64, 5, 2, 0, False),
    ('h2', 2, 64, 20, 28, 128, 5, 2, 1, False),
    ('to_bn', 1, 128, 10, 14, 33, 5, 2, 0, False),
    ('odd_sizes', 1, 5, 13, 9, 7, 3, 1, 1, False),
    ('odd_s2', 1, 4, 11, 15, 18, 5, 2, 0, False),
])
def test_conv2d_direct(cuda, name, N, Cin, H, W, Cout, K, stride, relu, norm):
    L = _lib()
    rs = np.random.RandomState(zlib.crc32(name.encode()) % 1000)
    x = (rs.uniform(0, 255, (N, Cin, H, W)) if norm else rs.normal(0, 1, (N, Cin, H, W))).astype(np.float32)
    w = rs.normal(0, 0.1, (K, K, Cin, Cout)).astype(np.float32)
    scale, shift = _bn(rs, Cout)
    OH, OW = -(-H // stride), -(-W // stride)
    res1 = rs.normal(0, 1, (N, Cout, OH, OW)).astype(np.float32)
    y = torch.empty((N, Cout, OH, OW), device=cuda)
    from oracle import oracle as O
    mean, std = O.norm_consts(torch.float32)
    d = lambda a: dev(a, cuda)
    tens = [d(x), d(w), d(scale), d(shift), d(res1)]
    m_d, s_d = (d(mean.flatten()), d(std.flatten())) if norm else (None, None)
    L.check(L.lib.ic_conv2d_bn_act_f32(L.ptr(tens[0]), L.ptr(tens[1]), L.ptr(tens[2]), L.ptr(tens[3]),
                                       L.ptr(tens[4]), None, L.ptr(y), N, Cin, H, W, Cout, K, K, stride, relu,
                                       L.ptr(m_d), L.ptr(s_d), L.current_stream()))
    torch.cuda.synchronize()
    ref = _ref_conv(x, w, scale, shift, stride, relu, res=(res1,), norm=norm)
    assert_close(y, ref, 'conv2d ' + name)


@pytest.mark.parametrize('name,N,Cin,H,W,Cout,K,relu,denorm', [
    ('from_bn', 1, 32, 6, 9, 128, 3, 1, False),
    ('from_bn_tiles', 2, 32, 7, 37, 128, 3, 1, False),
    ('from_bn_hi', 1, 64, 5, 18, 128, 3, 0, False),
    ('h12', 1, 128, 10, 12, 64, 5, 1, False),
    ('h13', 2, 64, 12, 20, 3, 5, 0, True),
    ('h13_tiles', 1, 64, 19, 35, 3, 5, 1, False),
    ('h13_cout4', 1, 64, 8, 16, 4, 5, 0, False),
    ('h13_cin32', 1, 32, 8, 16, 3, 5, 0, True),
    ('odd', 1, 3, 5, 7, 5, 5, 0, False),
])
def test_deconv2d(cuda, name, N, Cin, H, W, Cout, K, relu, denorm):
    L = _lib()
    rs = np.random.RandomState(zlib.crc32(name.encode()) % 1000 + 1)
    x = rs.normal(0, 1, (N, Cin, H, W)).astype(np.float32)
    w = rs.normal(0, 0.1, (K, K, Cout, Cin)).astype(np.float32)
    scale, shift = _bn(rs, Cout)
    y = torch.empty((N, Cout, 2 * H, 2 * W), device=cuda)
    from oracle import oracle as O
    mean, std = O.norm_consts(torch.float32)
    d = lambda a: dev(a, cuda)
    tens = [d(x), d(w), d(scale), d(shift)]
    m_d, s_d = (d(mean.flatten()), d(std.flatten())) if denorm else (None, None)
    L.check(L.lib.ic_deconv2d_bn_act_f32(L.ptr(tens[0]), L.ptr(tens[1]), L.ptr(tens[2]), L.ptr(tens[3]), L.ptr(y),
                                         N, Cin, H, W, Cout, K, K, relu, L.ptr(m_d), L.ptr(s_d), 0, L.current_stream()))
    torch.cuda.synchronize()
    ref = _ref_conv(x, w, scale, shift, 2, relu, transposed=True, denorm=denorm)
    assert_close(y, ref, 'deconv2d ' + name)


@pytest.mark.parametrize('name,N,Cin,H,W,Cout,transposed,relu', [
    ('h2', 1, 64, 24, 40, 128, 0, 1),
    ('h2_ragged', 2, 64, 14, 22, 128, 0, 1),
    ('to_bn', 1, 128, 12, 20, 33, 0, 0),
    ('to_bn_hi', 1, 128, 10, 18, 65, 0, 0),
    ('h12', 1, 128, 9, 13, 64, 1, 1),
    ('h12_b', 2, 128, 8, 32, 64, 1, 1),
    ('from_bn_adjoint_k3', 2, 128, 12, 20, 32, 0, 0),
    ('from_bn_adjoint_k3_odd', 1, 128, 11, 17, 64, 0, 1),
])
def test_conv2d_mfma_strided(cuda, name, N, Cin, H, W, Cout, transposed, relu):
    """matrix-core path of h2 / to_bn / h12 (packed filters, transposed conv as four phases) and of the 3x3 / 2 conv
    that is from_bn's data gradient."""
    L = _lib()
    K = 3 if '_k3' in name else 5
    rs = np.random.RandomState(zlib.crc32(name.encode()) % 1000 + 7)
    x = rs.normal(0, 1, (N, Cin, H, W)).astype(np.float32)
    wshape = (K, K, Cout, Cin) if transposed else (K, K, Cin, Cout)
    w = rs.normal(0, 0.05, wshape).astype(np.float32)
    scale, shift = _bn(rs, Cout)
    n = L.lib.ic_conv2d_mfma_packed_floats(K, K, Cin, Cout, 2, transposed)
    assert n > 0
    d = lambda a: dev(a, cuda)
    xd, wd, sd, hd = d(x), d(w), d(scale), d(shift)
    wp = torch.empty(n, device=cuda)
    L.check(L.lib.ic_pack_conv2d_mfma_f32(L.ptr(wd), L.ptr(wp), K, K, Cin, Cout, 2, transposed, L.current_stream()))
    oshape = (N, Cout, 2 * H, 2 * W) if transposed else (N, Cout, -(-H // 2), -(-W // 2))
    y = torch.full(oshape, float('nan'), device=cuda)
    L.check(L.lib.ic_conv2d_mfma_bn_act_f32(L.ptr(xd), L.ptr(wp), L.ptr(sd), L.ptr(hd), L.ptr(y), N, Cin, H, W, Cout,
                                            K, K, 2, transposed, relu, L.current_stream()))
    torch.cuda.synchronize()
    ref = _ref_conv(x, w, scale, shift, 2, relu, transposed=bool(transposed))
    assert_close(y, ref, 'conv2d mfma ' + name)
    # unsupported shapes say so instead of computing something else
    assert L.lib.ic_conv2d_mfma_packed_floats(3, 3, 32, 128, 2, 1) == 0
    assert L.lib.ic_conv2d_mfma_bn_act_f32(L.ptr(xd), L.ptr(wp), L.ptr(sd), L.ptr(hd), L.ptr(y), N, 32, H, W, 128,
                                           3, 3, 2, 1, relu, L.current_stream()) == -2


NUM_VARIANTS = 10


@pytest.mark.parametrize('variant', list(range(NUM_VARIANTS)) + [-1])
@pytest.mark.parametrize('N,H,W', [(1, 16, 32), (2, 13, 21), (1, 7, 5)])
def test_conv3x3_c128_mfma(cuda, variant, N, H, W):
    """the MFMA kernel, every tile variant, full and ragged tiles, with/without ReLU and residuals."""
    L = _lib()
    rs = np.random.RandomState(100 + H)
    x = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    w = rs.normal(0, 0.05, (3, 3, 128, 128)).astype(np.float32)
    scale, shift = _bn(rs, 128)
    r1 = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    r2 = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    d = lambda a: dev(a, cuda)
    xd, wd, sd, hd, r1d, r2d = d(x), d(w), d(scale), d(shift), d(r1), d(r2)
    wp = torch.empty(L.lib.ic_conv3x3_c128_packed_floats(), device=cuda)
    L.check(L.lib.ic_pack_conv3x3_c128_f32(L.ptr(wd), L.ptr(wp), L.current_stream()))
    flags = L.conv3_direct_variant(variant) if variant >= 0 else 0
    for relu, res in ((1, ()), (0, (r1d,)), (0, (r1d, r2d))):
        y = torch.full((N, 128, H, W), float('nan'), device=cuda)
        L.check(L.lib.ic_conv3x3_c128_bn_act_f32(
            L.ptr(xd), L.ptr(wp), L.ptr(sd), L.ptr(hd), L.ptr(res[0]) if len(res) > 0 else None,
            L.ptr(res[1]) if len(res) > 1 else None, L.ptr(y), N, H, W, relu, flags, L.current_stream()))
        torch.cuda.synchronize()
        ref = _ref_conv(x, w, scale, shift, 1, relu, res=[r.cpu().numpy() for r in res])
        assert_close(y, ref, 'conv3x3 mfma variant {} relu {} nres {}'.format(variant, relu, len(res)))


@pytest.mark.parametrize('shape', ['auto', 'wholek', 'wholek_pw', 'ksplit', 't16', 'seg1', 'seg2', 'seg3', 'seg3_pk', 'pair'])
@pytest.mark.parametrize('N,H,W', [(1, 16, 64), (2, 13, 21), (1, 7, 5), (1, 40, 72), (3, 10, 34)])
def test_conv3x3_c128_winograd(cuda, shape, N, H, W):
    """the Winograd F(2x2,3x3) form of the same layer: interior and border groups, odd sizes, ReLU / residuals,
    and the adjoint packing (data gradient) against the adjoint of the oracle's conv."""
    L = _lib()
    if shape in ('t16', 'pair') and not L.lib.ic_build_has_tuning_forms():
        # the forms the plan never picks are compiled into tuning builds only (make -C imgcomp_cvpr_amd/csrc TUNING=1): the shipped
        # library must refuse them instead of silently running something else
        x1 = torch.zeros((1, 128, 8, 32), device=cuda)
        wp1 = torch.zeros(L.lib.ic_wino3x3_c128_packed_floats(), device=cuda)
        one = torch.ones(128, device=cuda)
        rc = L.lib.ic_wino3x3_c128_bn_act_f32(L.ptr(x1), L.ptr(wp1), L.ptr(one), L.ptr(one), None, None, L.ptr(torch.empty_like(x1)), 1, 8, 32,
                                              0, L.CONV3_WINO_T16 if shape == 't16' else L.CONV3_WINO_PAIR, L.current_stream())
        assert rc != 0
        pytest.skip('tuning-build form (make TUNING=1)')
    rs = np.random.RandomState(300 + H)
    x = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    w = rs.normal(0, 0.05, (3, 3, 128, 128)).astype(np.float32)
    scale, shift = _bn(rs, 128)
    r1 = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    r2 = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    d = lambda a: dev(a, cuda)
    xd, wd, sd, hd, r1d, r2d = d(x), d(w), d(scale), d(shift), d(r1), d(r2)
    wp = torch.empty(L.lib.ic_wino3x3_c128_packed_floats(), device=cuda)
    L.check(L.lib.ic_pack_wino3x3_c128_f32(L.ptr(wd), L.ptr(wp), 0, L.current_stream()))
    # the decomposition is a per-call flag (odd widths have the per-wave whole-K and the K-split kernels: the even-width
    # forms fall back to whole-K there, which the library does by itself)
    flags = {'auto': 0, 'wholek': L.CONV3_WINO_WHOLEK, 'wholek_pw': L.CONV3_WINO_WHOLEK_PW, 'ksplit': L.CONV3_WINO_KSPLIT,
             't16': L.CONV3_WINO_T16, 'seg1': L.CONV3_WINO_SEG1, 'seg2': L.CONV3_WINO_SEG2, 'seg3': L.CONV3_WINO_SEG3,
             'seg3_pk': L.CONV3_WINO_SEG3 | L.CONV3_PACKED_TRANSFORM, 'pair': L.CONV3_WINO_PAIR}[shape]
    for relu, res in ((1, ()), (0, (r1d,)), (0, (r1d, r2d))):
        y = torch.full((N, 128, H, W), float('nan'), device=cuda)
        L.check(L.lib.ic_wino3x3_c128_bn_act_f32(
            L.ptr(xd), L.ptr(wp), L.ptr(sd), L.ptr(hd), L.ptr(res[0]) if len(res) > 0 else None,
            L.ptr(res[1]) if len(res) > 1 else None, L.ptr(y), N, H, W, relu, flags, L.current_stream()))
        torch.cuda.synchronize()
        ref = _ref_conv(x, w, scale, shift, 1, relu, res=[r.cpu().numpy() for r in res])
        assert_close(y, ref, 'winograd shape {} relu {} nres {}'.format(shape, relu, len(res)))
    # adjoint packing: conv with the flipped, channel-swapped filter
    L.check(L.lib.ic_pack_wino3x3_c128_f32(L.ptr(wd), L.ptr(wp), 1, L.current_stream()))
    ones, zeros = torch.ones(128, device=cuda), torch.zeros(128, device=cuda)
    y = torch.full((N, 128, H, W), float('nan'), device=cuda)
    L.check(L.lib.ic_wino3x3_c128_bn_act_f32(L.ptr(xd), L.ptr(wp), L.ptr(ones), L.ptr(zeros), None, None, L.ptr(y),
                                             N, H, W, 0, flags, L.current_stream()))
    torch.cuda.synchronize()
    w_adj = np.ascontiguousarray(w[::-1, ::-1].transpose(0, 1, 3, 2))
    ref = _ref_conv(x, w_adj, np.ones(128, np.float32), np.zeros(128, np.float32), 1, 0)
    assert_close(y, ref, 'winograd adjoint shape {}'.format(shape))


# one F(4x4) layer amplifies fp32 rounding more than F(2x2) (transform constants up to 8 x 8): 4-8e-6 of the tensor scale measured
# against 3-5e-7; through the whole network it does not show (tools/wino_f4_numerics.py, test_gpu_network.py)
W4_RTOL = 2e-5


@pytest.mark.parametrize('N,H,W', [(1, 16, 64), (2, 13, 20), (1, 7, 4), (1, 40, 72), (3, 10, 36), (1, 128, 192), (4, 32, 32), (2, 21, 28),
                                   (30, 40, 40)])
def test_conv3x3_c128_winograd_f4(cuda, N, H, W):
    """Winograd F(4x4,3x3) (csrc/conv3x3_wino4.hip) against the float64 conv: interior and border segments, heights that are
    not multiples of 4, widths with tiles beyond the map, ReLU / one / two residuals, the adjoint packing; odd widths refuse.
    (30, 40, 40) is the reference's training crop geometry (30 x 160 x 160 crops -> 40 x 40 maps)."""
    L = _lib()
    torch.set_num_threads(16)
    assert L.lib.ic_wino4_3x3_c128_supported(N, H, W) == 1 and L.lib.ic_wino4_3x3_c128_supported(N, H, W + 1) == 0
    rs = np.random.RandomState(400 + H)
    x = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    w = rs.normal(0, 0.05, (3, 3, 128, 128)).astype(np.float32)
    scale, shift = _bn(rs, 128)
    r1 = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    r2 = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    d = lambda a: dev(a, cuda)
    xd, wd, sd, hd, r1d, r2d = d(x), d(w), d(scale), d(shift), d(r1), d(r2)
    wp = torch.empty(L.lib.ic_wino4_3x3_c128_packed_floats(), device=cuda)
    L.check(L.lib.ic_pack_wino4_3x3_c128_f32(L.ptr(wd), L.ptr(wp), 0, L.current_stream()))
    for relu, res in ((1, ()), (0, (r1d,)), (0, (r1d, r2d))):
        y = torch.full((N, 128, H, W), float('nan'), device=cuda)
        L.check(L.lib.ic_wino4_3x3_c128_bn_act_f32(L.ptr(xd), L.ptr(wp), L.ptr(sd), L.ptr(hd), L.ptr(res[0]) if res else None,
                                                   L.ptr(res[1]) if len(res) > 1 else None, L.ptr(y), N, H, W, relu, 0, L.current_stream()))
        torch.cuda.synchronize()
        ref = _ref_conv(x, w, scale, shift, 1, relu, res=[r.cpu().numpy() for r in res])
        assert_close(y, ref, 'winograd F(4x4) {}x{} relu {} nres {}'.format(H, W, relu, len(res)), W4_RTOL)
    L.check(L.lib.ic_pack_wino4_3x3_c128_f32(L.ptr(wd), L.ptr(wp), 1, L.current_stream()))
    ones, zeros = torch.ones(128, device=cuda), torch.zeros(128, device=cuda)
    y = torch.full((N, 128, H, W), float('nan'), device=cuda)
    L.check(L.lib.ic_wino4_3x3_c128_bn_act_f32(L.ptr(xd), L.ptr(wp), L.ptr(ones), L.ptr(zeros), None, None, L.ptr(y), N, H, W, 0, 0,
                                               L.current_stream()))
    torch.cuda.synchronize()
    w_adj = np.ascontiguousarray(w[::-1, ::-1].transpose(0, 1, 3, 2))
    assert_close(y, _ref_conv(x, w_adj, np.ones(128, np.float32), np.zeros(128, np.float32), 1, 0), 'winograd F(4x4) adjoint', W4_RTOL)
    assert L.lib.ic_wino4_3x3_c128_bn_act_f32(L.ptr(xd), L.ptr(wp), L.ptr(ones), L.ptr(zeros), None, None, L.ptr(y), N, H, W + 1, 0, 0,
                                              L.current_stream()) != 0


# h2 / h12 as F(4x4) over phases: a 3x3 layer with K = 256 x 9 (h2) resp. the same transform constants on 5x5 filters; the float32
# emulation (tools/phase_conv_check.py) gives 1.1e-5 / 8.0e-6 of the tensor scale on N(0, 1) input
W5_RTOL = 3e-5


@pytest.mark.parametrize('N,H,W', [(1, 8, 16), (2, 13, 20), (1, 5, 4), (1, 32, 48), (1, 128, 192)])
def test_conv5s2_layers_as_winograd_over_phases(cuda, N, H, W):
    """h2 (5x5 / stride-2 conv 64 -> 128) and h12 (5x5 / stride-2 transposed conv 128 -> 64) on the F(4x4,3x3) kernel -- one 3x3
    convolution over the four phases of the input / to the four phases of the output (csrc/conv3x3_wino4.hip, packing modes 2 / 3)
    -- against the oracle's own strided convolutions (TF SAME pads 1 / 2, the transposed crop rule), BN + ReLU folded in."""
    L = _lib()
    assert L.lib.ic_wino4_conv5s2_supported(N, H, W) == 1 and L.lib.ic_wino4_conv5s2_supported(N, H, W + 2) == 0
    rs = np.random.RandomState(900 + H)
    st = L.current_stream()
    # ---- h2
    x = rs.normal(0, 1, (N, 64, 2 * H, 2 * W)).astype(np.float32)
    w = rs.normal(0, 0.03, (5, 5, 64, 128)).astype(np.float32)
    scale, shift = _bn(rs, 128)
    xd, wd, sd, hd = dev(x, cuda), dev(w, cuda), dev(scale, cuda), dev(shift, cuda)
    xs = torch.empty((N, 4 * 64, H, W), device=cuda)
    L.check(L.lib.ic_space_to_depth2_f32(L.ptr(xd), L.ptr(xs), N, 64, 2 * H, 2 * W, st))
    torch.cuda.synchronize()
    assert torch.equal(xs.view(N, 2, 2, 64, H, W), xd.view(N, 64, H, 2, W, 2).permute(0, 3, 5, 1, 2, 4))
    wp = torch.empty(L.lib.ic_wino4_conv5s2_packed_floats(), device=cuda)
    L.check(L.lib.ic_pack_wino4_conv5s2_f32(L.ptr(wd), L.ptr(wp), 0, st))
    for relu in (1, 0):
        y = torch.full((N, 128, H, W), float('nan'), device=cuda)
        L.check(L.lib.ic_wino4_conv5s2_c64_c128_bn_act_f32(L.ptr(xs), L.ptr(wp), L.ptr(sd), L.ptr(hd), L.ptr(y), N, H, W, relu, 0, st))
        torch.cuda.synchronize()
        assert_close(y, _ref_conv(x, w, scale, shift, 2, relu), 'h2 as F(4x4) over phases {}x{} relu {}'.format(H, W, relu), W5_RTOL)
    # ---- h12
    x = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    w = rs.normal(0, 0.03, (5, 5, 64, 128)).astype(np.float32)              # TF transposed layout [kh][kw][out][in]
    scale, shift = _bn(rs, 64)
    xd, wd, sd, hd = dev(x, cuda), dev(w, cuda), dev(scale, cuda), dev(shift, cuda)
    L.check(L.lib.ic_pack_wino4_conv5s2_f32(L.ptr(wd), L.ptr(wp), 1, st))
    for relu in (1, 0):
        y = torch.full((N, 64, 2 * H, 2 * W), float('nan'), device=cuda)
        L.check(L.lib.ic_wino4_deconv5s2_c128_c64_bn_act_f32(L.ptr(xd), L.ptr(wp), L.ptr(sd), L.ptr(hd), L.ptr(y), N, H, W, relu, 0, st))
        torch.cuda.synchronize()
        assert_close(y, _ref_conv(x, w, scale, shift, 2, relu, transposed=True), 'h12 as F(4x4) to phases {}x{} relu {}'.format(H, W, relu), W5_RTOL)


def test_conv5s2_phase_forms_agree_with_the_direct_kernels_on_random_shapes(cuda):
    """fuzz: h2 / h12 in F(4x4)-over-phases form against the direct MFMA kernels of the same layers (each is checked against the oracle
    above) on random map sizes -- odd heights, widths of one to many 4-pixel tiles, both segment shapes, batches."""
    L = _lib()
    rs = np.random.RandomState(77)
    st = L.current_stream()
    w = torch.as_tensor(rs.normal(0, 0.03, (5, 5, 64, 128)).astype(np.float32)).to(cuda)
    wp4 = torch.empty(L.lib.ic_wino4_conv5s2_packed_floats(), device=cuda)
    shapes = [(1, 1, 4), (2, 3, 8), (1, 9, 36), (3, 16, 32)] + [(int(rs.randint(1, 4)), int(rs.randint(1, 40)), 4 * int(rs.randint(1, 20))) for _ in range(10)]
    for tr in (0, 1):
        cin, cout = (128, 64) if tr else (64, 128)
        sc, sh = torch.rand(cout, device=cuda) + 0.5, torch.randn(cout, device=cuda) * 0.1
        wpm = torch.empty(L.lib.ic_conv2d_mfma_packed_floats(5, 5, cin, cout, 2, tr), device=cuda)
        L.check(L.lib.ic_pack_conv2d_mfma_f32(L.ptr(w), L.ptr(wpm), 5, 5, cin, cout, 2, tr, st))
        L.check(L.lib.ic_pack_wino4_conv5s2_f32(L.ptr(w), L.ptr(wp4), tr, st))
        for N, H, W in shapes:
            if tr:
                x = torch.randn((N, 128, H, W), device=cuda)
                y_d, y_w = torch.full((N, 64, 2 * H, 2 * W), float('nan'), device=cuda), torch.full((N, 64, 2 * H, 2 * W), float('nan'), device=cuda)
                L.check(L.lib.ic_conv2d_mfma_bn_act_f32(L.ptr(x), L.ptr(wpm), L.ptr(sc), L.ptr(sh), L.ptr(y_d), N, 128, H, W, 64, 5, 5, 2, 1, 1, st))
                L.check(L.lib.ic_wino4_deconv5s2_c128_c64_bn_act_f32(L.ptr(x), L.ptr(wp4), L.ptr(sc), L.ptr(sh), L.ptr(y_w), N, H, W, 1, 0, st))
            else:
                x = torch.randn((N, 64, 2 * H, 2 * W), device=cuda)
                xs = torch.empty((N, 256, H, W), device=cuda)
                y_d, y_w = torch.full((N, 128, H, W), float('nan'), device=cuda), torch.full((N, 128, H, W), float('nan'), device=cuda)
                L.check(L.lib.ic_space_to_depth2_f32(L.ptr(x), L.ptr(xs), N, 64, 2 * H, 2 * W, st))
                L.check(L.lib.ic_conv2d_mfma_bn_act_f32(L.ptr(x), L.ptr(wpm), L.ptr(sc), L.ptr(sh), L.ptr(y_d), N, 64, 2 * H, 2 * W, 128, 5, 5, 2, 0, 1, st))
                L.check(L.lib.ic_wino4_conv5s2_c64_c128_bn_act_f32(L.ptr(xs), L.ptr(wp4), L.ptr(sc), L.ptr(sh), L.ptr(y_w), N, H, W, 1, 0, st))
            torch.cuda.synchronize()
            assert bool(torch.isfinite(y_w).all()), (tr, N, H, W)
            err = float((y_w - y_d).abs().max()) / max(1.0, float(y_d.abs().max()))
            assert err < W5_RTOL, 'transposed {} shape {}: {}'.format(tr, (N, H, W), err)


def test_wino4_batched_packer_equals_the_single_one(cuda):
    """ic_pack_wino4_3x3_c128_batch_f32 (every 3x3 filter of a network in one launch, forward and adjoint) writes the fragments
    ic_pack_wino4_3x3_c128_f32 writes layer by layer."""
    L = _lib()
    g = torch.Generator().manual_seed(11)
    ws = [(torch.randn((3, 3, 128, 128), generator=g) * 0.05).to(cuda) for _ in range(3)]
    table = torch.tensor([w.data_ptr() for w in ws], dtype=torch.int64, device=cuda)
    n = L.lib.ic_wino4_3x3_c128_packed_floats()
    for backward in (0, 1):
        batch = torch.full((3, n), float('nan'), device=cuda)
        L.check(L.lib.ic_pack_wino4_3x3_c128_batch_f32(L.ptr(table), L.ptr(batch), 3, backward, L.current_stream()))
        for l, w in enumerate(ws):
            one = torch.full((n,), float('nan'), device=cuda)
            L.check(L.lib.ic_pack_wino4_3x3_c128_f32(L.ptr(w), L.ptr(one), backward, L.current_stream()))
            torch.cuda.synchronize()
            assert torch.equal(batch[l], one), 'layer {} backward {}'.format(l, backward)


W4_FULL_LOAD_CASES = [
    # (label, N, H, W): which instantiation of wino4_3x3_kernel the launch runs (WT = write-through stores: <= 512 work-groups)
    ('c128 1x16 segments, several rounds', 6, 128, 192),       # <WT=0, RES, 128, 128, SHUF=0, SEG2=0>: 1152 work-groups
    ('c128 2x8 segments (training crops)', 72, 32, 32),        # <.., SEG2=1>: 576 work-groups
    ('c128 one round, write-through', 2, 128, 192),            # <WT=1, ..>: 384 work-groups, two per CU on half the chip
]


@pytest.mark.parametrize('label,N,H,W', W4_FULL_LOAD_CASES)
@pytest.mark.parametrize('n_res', [0, 2])
def test_conv3x3_c128_winograd_f4_full_load_is_deterministic(cuda, label, N, H, W, n_res):
    """Two waves per SIMD is where round 4's failure showed (wrong values in lanes 12..15 of a 16-lane row).  Root cause, round 5
    (profiles/r05_w4_rootcause.md): the register allocator's spills / copies of VGPR-resident accumulators next to inline-asm
    MFMAs, without the matrix-pipe wait states -- ruled out at build time by csrc/isa_audit.py.  This is the run-time half: every
    instantiation of the 128 -> 128 kernel (segment shapes, store modes, RES = 1 / 2 epilogues) at two work-groups per CU, 12 launches
    back to back bit-identical to the first, the first within the bound of the float64 conv."""
    L = _lib()
    g = torch.Generator().manual_seed(3)
    x = torch.relu(torch.randn((N, 128, H, W), generator=g)) * 1.5
    w = torch.randn((3, 3, 128, 128), generator=g) * 0.03
    sc, sh = torch.rand(128, generator=g) * 0.6 + 0.5, torch.randn(128, generator=g) * 0.1
    res = [torch.randn((N, 128, H, W), generator=g) for _ in range(n_res)]
    xd, wd, scd, shd = x.to(cuda), w.to(cuda), sc.to(cuda), sh.to(cuda)
    resd = [r.to(cuda) for r in res]
    wp = torch.empty(L.lib.ic_wino4_3x3_c128_packed_floats(), device=cuda)
    L.check(L.lib.ic_pack_wino4_3x3_c128_f32(L.ptr(wd), L.ptr(wp), 0, L.current_stream()))
    assert int(L.lib.ic_wino4_3x3_c128_workgroups(N, H, W)) >= 384
    ys = []
    for _ in range(12):
        y = torch.empty((N, 128, H, W), device=cuda)
        L.check(L.lib.ic_wino4_3x3_c128_bn_act_f32(L.ptr(xd), L.ptr(wp), L.ptr(scd), L.ptr(shd), L.ptr(resd[0]) if n_res else None,
                                                   L.ptr(resd[1]) if n_res > 1 else None, L.ptr(y), N, H, W, 1, 0, L.current_stream()))
        ys.append(y)
    torch.cuda.synchronize()
    for k in range(1, 12):
        assert torch.equal(ys[0], ys[k]), '{}: launch {} differs from launch 0 in {} values'.format(label, k, int((ys[0] != ys[k]).sum()))
    torch.set_num_threads(16)
    n_ref = min(N, 2)
    ref = torch.relu(torch.nn.functional.conv2d(torch.nn.functional.pad(x[:n_ref].double(), (1, 1, 1, 1)), w.double().permute(3, 2, 0, 1))
                     * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
    for r in res:
        ref = ref + r[:n_ref].double()
    assert_close(ys[0][:n_ref], ref, 'winograd F(4x4) full load', W4_RTOL)


@pytest.mark.parametrize('N,H,W,n_res', [(1, 128, 192, 1), (2, 37, 68, 2), (1, 64, 64, 0), (6, 128, 192, 1), (1, 540, 960, 2), (3, 100, 192, 1)])
def test_conv3x3_c128_winograd_f4_eight_wave_form_is_bit_identical(cuda, N, H, W, n_res):
    """IC_CONV3_WINO4_WG8 (round 6): ONE 8-wave work-group per segment covers all 128 output channels, the input transform is made
    once per segment, the ring's hazards are kept by LDS counters instead of a barrier.  Same values in the same order as the
    4-wave form -- bit-identical, 8 launches back to back (a lost or early counter hand-off would show as a stale B operand),
    single-round (write-through) and multi-round launches, ragged borders, 0 / 1 / 2 residuals; and the plan: 8 waves when asked
    for or from 2048 four-wave work-groups on, never on maps with 2 x 8-tile segments, never with IC_CONV3_WINO4_WG4."""
    L = _lib()
    waves = lambda n, h, w, f: int(L.lib.ic_wino4_3x3_c128_waves(n, h, w, f))
    assert waves(1, 128, 192, 0) == 4 and waves(1, 128, 192, L.CONV3_WINO4_WG8) == 8 and waves(1, 540, 960, 0) == 8
    assert waves(1, 540, 960, L.CONV3_WINO4_WG4) == 4 and waves(32, 32, 32, L.CONV3_WINO4_WG8) == 4 and waves(1, 128, 190, 0) == 0
    g = torch.Generator().manual_seed(11 + H)
    x = (torch.relu(torch.randn((N, 128, H, W), generator=g)) * 1.5).to(cuda)
    w = (torch.randn((3, 3, 128, 128), generator=g) * 0.03).to(cuda)
    sc, sh = (torch.rand(128, generator=g) * 0.6 + 0.5).to(cuda), (torch.randn(128, generator=g) * 0.1).to(cuda)
    res = [torch.randn((N, 128, H, W), generator=g).to(cuda) for _ in range(n_res)]
    wp = torch.empty(L.lib.ic_wino4_3x3_c128_packed_floats(), device=cuda)
    L.check(L.lib.ic_pack_wino4_3x3_c128_f32(L.ptr(w), L.ptr(wp), 0, L.current_stream()))

    def run(flags):
        y = torch.full((N, 128, H, W), float('nan'), device=cuda)
        L.check(L.lib.ic_wino4_3x3_c128_bn_act_f32(L.ptr(x), L.ptr(wp), L.ptr(sc), L.ptr(sh), L.ptr(res[0]) if n_res else None,
                                                   L.ptr(res[1]) if n_res > 1 else None, L.ptr(y), N, H, W, 1, flags, L.current_stream()))
        return y
    y4 = run(L.CONV3_WINO4_WG4)
    ys = [run(L.CONV3_WINO4_WG8) for _ in range(8)]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y4).all())
    for k, y in enumerate(ys):
        assert torch.equal(y4, y), 'launch {} of the 8-wave form differs from the 4-wave form in {} values'.format(k, int((y4 != y).sum()))


@pytest.mark.parametrize('transposed', [0, 1])
@pytest.mark.parametrize('N,H,W', [(4, 128, 192), (48, 32, 32)])
def test_conv5s2_as_winograd_full_load_is_deterministic(cuda, transposed, N, H, W):
    """the same for the <256,128> (h2 over its input's phases) and <128,256,SHUF> (h12 to its output's phases) instantiations, 1 x 16
    and 2 x 8 segments, at two work-groups per CU: 12 launches bit-identical (the values themselves:
    test_conv5s2_layers_as_winograd_over_phases)."""
    L = _lib()
    g = torch.Generator().manual_seed(5)
    st = L.current_stream()
    cin = 128 if transposed else 256
    x = (torch.relu(torch.randn((N, cin, H, W), generator=g)) * 1.2).to(cuda)
    w = (torch.randn((5, 5, 64, 128), generator=g) * 0.03).to(cuda)
    cout = 64 if transposed else 128
    sc, sh = (torch.rand(cout, generator=g) * 0.6 + 0.5).to(cuda), (torch.randn(cout, generator=g) * 0.1).to(cuda)
    wp = torch.empty(L.lib.ic_wino4_conv5s2_packed_floats(), device=cuda)
    L.check(L.lib.ic_pack_wino4_conv5s2_f32(L.ptr(w), L.ptr(wp), transposed, st))
    assert int(L.lib.ic_wino4_conv5s2_workgroups(N, H, W, transposed)) >= 384
    ys = []
    for _ in range(12):
        y = torch.empty((N, 64, 2 * H, 2 * W) if transposed else (N, 128, H, W), device=cuda)
        if transposed:
            L.check(L.lib.ic_wino4_deconv5s2_c128_c64_bn_act_f32(L.ptr(x), L.ptr(wp), L.ptr(sc), L.ptr(sh), L.ptr(y), N, H, W, 1, 0, st))
        else:
            L.check(L.lib.ic_wino4_conv5s2_c64_c128_bn_act_f32(L.ptr(x), L.ptr(wp), L.ptr(sc), L.ptr(sh), L.ptr(y), N, H, W, 1, 0, st))
        ys.append(y)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ys[0]).all())
    for k in range(1, 12):
        assert torch.equal(ys[0], ys[k]), 'launch {} differs from launch 0 in {} values'.format(k, int((ys[0] != ys[k]).sum()))


def test_conv3x3_c128_auto_selection(cuda):
    """one packed blob, both forms: Winograd wherever its 31-bit addressing reaches, the direct form beyond; the
    override works, and both give the oracle's result through the same entry point."""
    L = _lib()
    # direct fragments + the Winograd fragments in both layouts (32-channel tiles | 16-channel tiles)
    # ... + the F(4x4) fragments (36 positions)
    assert L.lib.ic_conv3x3_c128_both_packed_floats() == 9 * 128 * 128 + 2 * 16 * 128 * 128 + 36 * 128 * 128
    assert L.lib.ic_conv3x3_c128_pick_algo(1, 16, 16, 0) == 1              # K-split work-groups serve small maps
    assert L.lib.ic_conv3x3_c128_pick_algo(1, 128, 192, 0) == 1
    assert L.lib.ic_conv3x3_c128_pick_algo(32, 32, 32, 0) == 1
    assert L.lib.ic_conv3x3_c128_pick_algo(1, 4096, 2048, 0) == 0          # beyond 31-bit offsets: direct form
    assert L.lib.ic_conv3x3_c128_pick_algo(1, 4096, 2048, L.CONV3_WINO) == 0
    N, H, W = 1, 24, 40
    rs = np.random.RandomState(7)
    x = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    w = rs.normal(0, 0.05, (3, 3, 128, 128)).astype(np.float32)
    scale, shift = _bn(rs, 128)
    xd, wd, sd, hd = dev(x, cuda), dev(w, cuda), dev(scale, cuda), dev(shift, cuda)
    wp = torch.empty(L.lib.ic_conv3x3_c128_both_packed_floats(), device=cuda)
    L.check(L.lib.ic_pack_conv3x3_c128_both_f32(L.ptr(wd), L.ptr(wp), 0, L.current_stream()))
    ref = _ref_conv(x, w, scale, shift, 1, 1)
    # which of the three kernels: F(4x4) from 160 work-groups (a Kodak map has 192), with launches in flight beside it from 384
    # together, where the map fills its 16-tile segments; F(2x2) otherwise, and always against an explicit F(2x2) form or IC_CONV3_NO_WINO4
    pf = L.lib.ic_conv3x3_c128_pick_form
    assert pf(1, 128, 192, 0) == 2 and pf(1, 128, 128, 0) == 1 and pf(8, 128, 192, 0) == 2 and pf(1, 512, 512, 0) == 2
    assert pf(1, 128, 192, L.CONV3_IN_FLIGHT(6)) == 2 and pf(1, 32, 32, L.CONV3_IN_FLIGHT(6)) == 1
    assert pf(200, 12, 12, 0) == 1 and pf(30, 40, 40, 0) == 2              # 800 work-groups 28 % full; 600 work-groups 62 % full
    assert pf(8, 128, 192, L.CONV3_NO_WINO4) == 1 and pf(8, 128, 192, L.CONV3_WINO) == 2 and pf(8, 128, 190, 0) == 1
    assert pf(1, 16, 16, L.CONV3_WINO4) == 2 and pf(1, 4096, 2048, 0) == 0
    outs = []
    for algo, flags in ((0, L.CONV3_DIRECT), (1, L.CONV3_WINO), (1, L.CONV3_WINO4)):
        assert L.lib.ic_conv3x3_c128_pick_algo(N, H, W, flags) == algo
        y = torch.full((N, 128, H, W), float('nan'), device=cuda)
        L.check(L.lib.ic_conv3x3_c128_auto_f32(L.ptr(xd), L.ptr(wp), L.ptr(sd), L.ptr(hd), None, None, L.ptr(y),
                                               N, H, W, 1, flags, L.current_stream()))
        torch.cuda.synchronize()
        assert_close(y, ref, 'auto entry, flags {:#x}'.format(flags), W4_RTOL if flags == L.CONV3_WINO4 else RTOL)
        outs.append(y)
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2]), 'the per-call form flag did not switch kernels'


def test_conv3x3_mfma_matches_direct_kernel(cuda):
    """the two implementations of the same op agree (independent code paths on the device)."""
    L = _lib()
    rs = np.random.RandomState(7)
    N, H, W = 1, 24, 40
    d = lambda a: dev(a, cuda)
    x = d(rs.normal(0, 1, (N, 128, H, W)))
    w = d(rs.normal(0, 0.05, (3, 3, 128, 128)))
    s, h = (d(a) for a in _bn(rs, 128))
    wp = torch.empty(L.lib.ic_conv3x3_c128_packed_floats(), device=cuda)
    L.check(L.lib.ic_pack_conv3x3_c128_f32(L.ptr(w), L.ptr(wp), L.current_stream()))
    y1 = torch.empty((N, 128, H, W), device=cuda)
    y2 = torch.empty_like(y1)
    L.check(L.lib.ic_conv3x3_c128_bn_act_f32(L.ptr(x), L.ptr(wp), L.ptr(s), L.ptr(h), None, None, L.ptr(y1),
                                             N, H, W, 1, 0, L.current_stream()))
    L.check(L.lib.ic_conv2d_bn_act_f32(L.ptr(x), L.ptr(w), L.ptr(s), L.ptr(h), None, None, L.ptr(y2),
                                       N, 128, H, W, 128, 3, 3, 1, 1, None, None, L.current_stream()))
    torch.cuda.synchronize()
    assert rel_err(y1, y2) < 1e-5


def test_quantize_bit_exact_symbols(cuda):
    """symbols / qhard are bit-exact given identical z; includes exact ties and boundary values."""
    from imgcomp_cvpr_amd import quantizer
    from oracle import oracle as O
    rs = np.random.RandomState(3)
    for centers in (np.linspace(-2, 2, 6).astype(np.float32),
                    np.sort(np.random.RandomState(666).uniform(-2, 2, 6)).astype(np.float32)):
        z = rs.normal(0, 1.5, (2, 8, 16, 24)).astype(np.float32)
        mids = ((centers[1:] + centers[:-1]) / 2).astype(np.float32)
        flat = z.reshape(-1)
        flat[:5] = mids                                   # exact midpoints -> ties
        flat[5:10] = np.nextafter(mids, np.float32(10))   # one ulp above
        flat[10:15] = np.nextafter(mids, np.float32(-10)) # one ulp below
        flat[15:21] = centers
        flat[21] = 0.0
        flat[22:24] = [1e6, -1e6]
        qs, qh, sym = quantizer.quantize(dev(z, cuda), dev(centers, cuda), 1.0)
        rs32, rh32, rsym = O.quantize(torch.as_tensor(z), centers, 1.0)
        assert sym.dtype == torch.int64
        assert torch.equal(sym.cpu(), rsym), 'symbols differ from the oracle'
        assert torch.equal(qh.cpu(), rh32), 'qhard differs from the oracle'
        rs64, _, _ = O.quantize(torch.as_tensor(z).double(), centers.astype(np.float64), 1.0)
        assert_close(qs, rs64, 'qsoft', rtol=1e-6)


def test_heatmap_quantize(cuda):
    from oracle import oracle as O
    L = _lib()
    rs = np.random.RandomState(5)
    N, C, h, w = 2, 32, 9, 13
    bott = rs.normal(0, 2, (N, C + 1, h, w)).astype(np.float32)
    centers = np.linspace(-2, 2, 6).astype(np.float32)
    bd, cd = dev(bott, cuda), dev(centers, cuda)
    mk = lambda: torch.empty((N, C, h, w), device=cuda)
    hm, z, qs, qh, qb = mk(), mk(), mk(), mk(), mk()
    sym = torch.empty((N, C, h, w), dtype=torch.int64, device=cuda)
    L.check(L.lib.ic_heatmap_quantize_f32(L.ptr(bd), L.ptr(cd), 6, 1.0, L.ptr(hm), L.ptr(z), L.ptr(qs), L.ptr(qh),
                                          L.ptr(qb), L.ptr(sym), N, C, h, w, L.current_stream()))
    torch.cuda.synchronize()
    b64 = torch.as_tensor(bott).double()
    hm64 = O.heatmap3d(b64)
    assert_close(hm, hm64, 'heatmap', rtol=1e-5)
    assert_close(z, hm64 * b64[:, 1:], 'z', rtol=1e-5)
    # quantiser outputs must be exactly the oracle's on the kernel's own z
    _, rh, rsym = O.quantize(z.cpu(), centers, 1.0)
    assert torch.equal(sym.cpu(), rsym) and torch.equal(qh.cpu(), rh)
    assert torch.equal(qb.cpu(), (qs + (qh - qs)).cpu())


def _pc_setup(cuda, configs, syn_weights, k_cfg='res_shallow'):
    from imgcomp_cvpr_amd import probclass, config_parser as cp
    ae_cfg, pc_cfg = configs
    if k_cfg != 'res_shallow':
        pc_cfg, _ = cp.parse(cp.builtin_config_path('pc_configs', 'cvpr', k_cfg))
    pc = probclass.get_network_cls(pc_cfg)(pc_cfg, num_centers=ae_cfg.num_centers)
    return pc, pc_cfg


@pytest.mark.parametrize('N,C,h,w', [(1, 32, 8, 8), (2, 5, 7, 11), (1, 1, 1, 1)])
def test_pc_bitcost_and_logits(cuda, configs, syn_weights, N, C, h, w):
    from oracle import oracle as O
    pc, _ = _pc_setup(cuda, configs, syn_weights)
    pc.load_weights(syn_weights, cuda)
    centers = syn_weights['autoencoder/encoder/centers']
    rs = np.random.RandomState(11)
    sym = rs.randint(0, 6, (N, C, h, w)).astype(np.int64)
    q = centers[sym]
    bits, logits = pc.bitcost(dev(q, cuda), dev(sym, cuda, torch.int64), False, pad_value=float(centers[0]),
                              return_logits=True)
    torch.cuda.synchronize()
    rb, rl = O.bitcost(torch.as_tensor(q).double(), torch.as_tensor(sym), syn_weights, float(centers[0]))
    assert_close(logits, rl, 'pc logits')
    assert_close(bits, rb, 'pc bits')
    # logits() on a pre-padded volume gives the same numbers bit-for-bit
    qp = O.pad_for_probclass3d(torch.as_tensor(q), 9, float(centers[0]))
    l2 = pc.logits(dev(qp.numpy(), cuda), False)
    assert torch.equal(l2, logits)


def test_pc_k64(cuda, configs):
    """res_shallow_64 (arch_param__k = 64) goes through the same kernels."""
    from imgcomp_cvpr_amd import weights as W
    from oracle import oracle as O
    ae_cfg, _ = configs
    pc, pc_cfg = _pc_setup(cuda, configs, None, 'res_shallow_64')
    wts = W.synthetic_weights(ae_cfg, pc_cfg)
    pc.load_weights(wts, cuda)
    centers = wts['autoencoder/encoder/centers']
    sym = np.random.RandomState(2).randint(0, 6, (1, 6, 5, 9)).astype(np.int64)
    q = centers[sym]
    bits = pc.bitcost(dev(q, cuda), dev(sym, cuda, torch.int64), False, pad_value=float(centers[0]))
    rb, _ = O.bitcost(torch.as_tensor(q).double(), torch.as_tensor(sym), wts, float(centers[0]))
    assert_close(bits, rb, 'pc bits k=64')


def test_pc_causality(cuda, configs, syn_weights):
    """perturbing symbol i leaves logits at raster indices <= i unchanged (masks, probclass.py:150-176)."""
    pc, _ = _pc_setup(cuda, configs, syn_weights)
    pc.load_weights(syn_weights, cuda)
    centers = syn_weights['autoencoder/encoder/centers']
    rs = np.random.RandomState(4)
    C, h, w = 6, 7, 9
    sym = rs.randint(0, 6, (1, C, h, w))
    base = pc.logits_unpadded(dev(centers[sym], cuda), float(centers[0])).cpu().reshape(-1, 6)
    for idx in (0, 17, C * h * w // 2, C * h * w - 2):
        s2 = sym.copy().reshape(-1)
        s2[idx] = (s2[idx] + 3) % 6
        out = pc.logits_unpadded(dev(centers[s2.reshape(1, C, h, w)], cuda), float(centers[0])).cpu().reshape(-1, 6)
        assert torch.equal(out[:idx + 1], base[:idx + 1]), 'logits before/at the perturbed symbol changed'
        assert not torch.equal(out[idx + 1:], base[idx + 1:])


def test_sum_and_bpp(cuda):
    from imgcomp_cvpr_amd import bits
    rs = np.random.RandomState(9)
    bc = rs.uniform(0, 3, (2, 32, 16, 24)).astype(np.float32)
    x = torch.zeros((2, 3, 128, 192), device=cuda)
    bpp = bits.bitcost_to_bpp(dev(bc, cuda), x)
    ref = bc.astype(np.float64).sum() / (2 * 128 * 192)
    assert abs(float(bpp) - ref) / ref < 1e-6
    # deterministic
    assert float(bits.bitcost_to_bpp(dev(bc, cuda), x)) == float(bpp)
    # every image of a batch in one call: the same bits as a call per image
    bcd = dev(bc, cuda)
    per = bits.bitcost_to_bpp_per_image(bcd, x)
    assert tuple(per.shape) == (2,)
    for i in range(2):
        assert torch.equal(per[i], bits.bitcost_to_bpp(bcd[i:i + 1], x[i:i + 1]))


def test_error_codes(cuda):
    """argument errors come back as codes, never as aborts; the Python shim raises."""
    L = _lib()
    assert L.lib.ic_conv2d_bn_act_f32(None, None, None, None, None, None, None, 1, 1, 1, 1, 1, 1, 1, 1, 0,
                                      None, None, None) == -1
    x = torch.zeros(8, device=cuda)
    assert L.lib.ic_quantize_f32(L.ptr(x), L.ptr(x), 17, 1.0, None, None, None, 8, None) == -2
    assert L.lib.ic_pc_logits_f32(L.ptr(x), L.ptr_table([x] * 8 + [None]), 24, 6, 0.0, L.ptr(x), 1, 1, 1, 1,
                                  L.ptr(x), 4, None) == -3
    with pytest.raises(L.HipLibraryError):
        L.check(-2, 'demo')
    with pytest.raises(L.HipLibraryError):
        from imgcomp_cvpr_amd import quantizer
        quantizer.quantize(torch.zeros(1, 1, 2, 2), torch.zeros(6), 1.0)     # CPU tensors: no fallback
    # a workspace one byte short of the size query's answer: IC_ERR_WORKSPACE (-3), decided on the host before any launch
    st = L.current_stream()
    f = lambda *shape: torch.zeros(shape, device=cuda)
    ws = lambda n: torch.zeros(n, dtype=torch.uint8, device=cuda)
    u8 = torch.zeros((1, 3, 17, 23), dtype=torch.uint8, device=cuda)
    need = L.lib.ic_val_metrics_workspace_bytes(1, 3, 17, 23)
    out6 = torch.zeros(6, dtype=torch.float64, device=cuda)
    assert need > 0 and L.lib.ic_val_metrics_u8_f64(L.ptr(u8), L.ptr(u8), 1, 3, 17, 23, L.ptr(out6), L.ptr(ws(need)), need - 1, st) == -3
    need, nplan = L.lib.ic_msssim_workspace_bytes(1, 2, 17, 19), L.lib.ic_msssim_plan_bytes(17, 19)
    assert need > 0 and nplan > 0
    assert L.lib.ic_msssim_loss_grad_f32(L.ptr(f(1, 2, 17, 19)), L.ptr(f(1, 2, 17, 19)), 1, 2, 17, 19, 1.0, L.ptr(ws(nplan)), None, L.ptr(f(16)),
                                         L.ptr(ws(need)), need - 1, st) == -3
    need = L.lib.ic_conv2d_wgrad_workspace_bytes(1, 3, 3, 5, 6, 3, 3)
    assert need > 0 and L.lib.ic_conv2d_wgrad_f32(L.ptr(f(1, 3, 5, 6)), L.ptr(f(1, 3, 5, 6)), L.ptr(f(3, 3, 3, 3)), 1, 3, 5, 6, 3, 3, 3, 1, None, 0.0,
                                                  L.ptr(ws(need)), need - 1, st) == -3
    need = L.lib.ic_conv3x3_c128_wgrad_workspace_bytes(1, 8, 16)
    assert need > 0 and L.lib.ic_conv3x3_c128_wgrad_f32(L.ptr(f(1, 128, 8, 16)), L.ptr(f(1, 128, 8, 16)), L.ptr(f(3, 3, 128, 128)), 1, 8, 16, None, 0.0,
                                                        L.ptr(ws(need)), need - 1, st) == -3
    need = L.lib.ic_pc_bwd_data_workspace_bytes(1, 24, 24, 1, 1, 1)
    assert need > 0 and L.lib.ic_pc_bwd_data_f32(L.ptr(f(1, 24, 1, 1, 1)), L.ptr(f(2, 3, 3, 24, 24)), None, None, L.ptr(f(1, 24, 2, 3, 3)), 1, 24, 24,
                                                 1, 1, 1, 0, 0, L.ptr(ws(need)), need - 1, st) == -3
    need = L.lib.ic_pc_wgrad_workspace_bytes(1, 24, 6, 1, 2, 2)
    assert need > 0 and L.lib.ic_pc_wgrad_f32(L.ptr(f(1, 24, 2, 4, 4)), None, 0.0, L.ptr(f(1, 6, 1, 2, 2)), L.ptr(f(2, 3, 3, 24, 6)), 1, 24, 6, 1, 2, 2, 0,
                                              L.ptr(ws(need)), need - 1, st) == -3
    need = L.lib.ic_ae_res_stack_workspace_bytes(1, 5, 7)
    wp, one = f(L.lib.ic_conv3x3_c128_both_packed_floats()), torch.ones(128, device=cuda)
    assert need > 0 and L.lib.ic_ae_res_stack_f32(L.ptr(f(1, 128, 5, 7)), L.ptr_table([wp, one, one] * 2), 0, L.ptr(f(1, 128, 5, 7)), 1, 5, 7,
                                                  L.ptr(ws(need)), need - 1, 0, st) == -3
    torch.cuda.synchronize()


def test_conv3x3_c128_forms_agree_on_random_shapes(cuda):
    """fuzz: direct form and every Winograd decomposition on 24 random (N, H, W) incl. odd and tiny maps, with ReLU and one
    residual -- all within fp32 rounding of the direct form (the oracle comparison of each form is done above), and the
    Winograd decompositions bit-identical to each other (the same operations per output, only the job shape differs)."""
    L = _lib()
    rs = np.random.RandomState(2024)
    w = rs.normal(0, 0.05, (3, 3, 128, 128)).astype(np.float32)
    scale, shift = _bn(rs, 128)
    wd, sd, hd = dev(w, cuda), dev(scale, cuda), dev(shift, cuda)
    wp = torch.empty(L.lib.ic_conv3x3_c128_both_packed_floats(), device=cuda)
    L.check(L.lib.ic_pack_conv3x3_c128_both_f32(L.ptr(wd), L.ptr(wp), 0, L.current_stream()))
    shapes = [(1, 1, 1), (1, 2, 3), (3, 5, 33), (1, 31, 65), (2, 4, 32), (2, 7, 66), (5, 2, 34), (1, 9, 68), (2, 21, 4), (1, 3, 132)] + \
             [(int(rs.randint(1, 4)), int(rs.randint(1, 70)), int(rs.randint(1, 100))) for _ in range(17)]
    forms = [L.CONV3_DIRECT, L.CONV3_WINO_WHOLEK, L.CONV3_WINO_KSPLIT, L.CONV3_WINO_WHOLEK_PW,
             L.CONV3_WINO_SEG1, L.CONV3_WINO_SEG2, L.CONV3_WINO_SEG3, L.CONV3_WINO_SEG3 | L.CONV3_PACKED_TRANSFORM,
             L.CONV3_WINO_SEG3 | L.CONV3_NO_XCD_RUNS, L.CONV3_AUTO, L.CONV3_WINO4]
    if L.lib.ic_build_has_tuning_forms():                             # make TUNING=1: the forms the plan never picks
        forms += [L.CONV3_WINO_T16, L.CONV3_WINO_PAIR, L.CONV3_WINO_PAIR | L.CONV3_NO_XCD_RUNS]
    for N, H, W in shapes:
        x = torch.randn((N, 128, H, W), device=cuda)
        r = torch.randn((N, 128, H, W), device=cuda)
        outs = []
        for flags in forms:
            y = torch.full((N, 128, H, W), float('nan'), device=cuda)
            L.check(L.lib.ic_conv3x3_c128_auto_f32(L.ptr(x), L.ptr(wp), L.ptr(sd), L.ptr(hd), L.ptr(r), None, L.ptr(y),
                                                   N, H, W, 1, flags, L.current_stream()))
            outs.append(y)
        torch.cuda.synchronize()
        scale_ = max(1.0, float(outs[0].abs().max()))
        for k in range(1, len(forms)):
            assert bool(torch.isfinite(outs[k]).all()), 'shape {} form {:#x}'.format((N, H, W), forms[k])
            err = float((outs[k] - outs[0]).abs().max()) / scale_
            assert err < 2e-5, 'shape {} form {:#x}: {}'.format((N, H, W), forms[k], err)
        for k in range(2, len(forms)):
            if forms[k] in (L.CONV3_WINO_KSPLIT, L.CONV3_AUTO, L.CONV3_WINO4):
                continue                      # K-split (which the automatic plan may pick) sums four partial chains, F(4x4)
                                              # (widths that are multiples of 4; F(2x2) otherwise) is another algorithm: same
                                              # value up to fp32 rounding, not the same bits
            assert torch.equal(outs[1], outs[k]), 'shape {} form {:#x} is not bit-identical to whole-K'.format((N, H, W), forms[k])


def test_edge_layers_random_shapes(cuda):
    """fuzz: the matrix-core edge layers (h1, from_bn, h13 in conv_edge.hip) on random (N, H, W) -- tile borders, widths that
    are not multiples of the 16-byte staging moves, single rows -- against the float64 reference convolution."""
    L = _lib()
    from oracle import oracle as O
    rs = np.random.RandomState(77)
    mean, std = O.norm_consts(torch.float32)
    m_d, s_d = dev(mean.flatten(), cuda), dev(std.flatten(), cuda)
    d = lambda a: dev(a, cuda)
    st = L.current_stream()
    for it in range(10):
        N, H, W = int(rs.randint(1, 3)), int(rs.randint(1, 40)), int(rs.randint(1, 75))
        # h1: 5x5 / 2 conv 3 -> 64, input normalisation, ReLU
        x = rs.uniform(0, 255, (N, 3, H, W)).astype(np.float32)
        w = rs.normal(0, 0.1, (5, 5, 3, 64)).astype(np.float32)
        sc, sh = _bn(rs, 64)
        y = torch.full((N, 64, -(-H // 2), -(-W // 2)), float('nan'), device=cuda)
        t = [d(x), d(w), d(sc), d(sh)]
        L.check(L.lib.ic_conv2d_bn_act_f32(L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), L.ptr(t[3]), None, None, L.ptr(y), N, 3, H, W, 64,
                                           5, 5, 2, 1, L.ptr(m_d), L.ptr(s_d), st))
        torch.cuda.synchronize()
        assert_close(y, _ref_conv(x, w, sc, sh, 2, 1, norm=True), 'h1 {}'.format((N, H, W)))
        # from_bn: 3x3 / 2 transposed conv 32 -> 128, ReLU
        x = rs.normal(0, 1, (N, 32, H, W)).astype(np.float32)
        w = rs.normal(0, 0.1, (3, 3, 128, 32)).astype(np.float32)
        sc, sh = _bn(rs, 128)
        y = torch.full((N, 128, 2 * H, 2 * W), float('nan'), device=cuda)
        t = [d(x), d(w), d(sc), d(sh)]
        L.check(L.lib.ic_deconv2d_bn_act_f32(L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), L.ptr(t[3]), L.ptr(y), N, 32, H, W, 128, 3, 3, 1,
                                             None, None, 0, st))
        torch.cuda.synchronize()
        assert_close(y, _ref_conv(x, w, sc, sh, 2, 1, transposed=True), 'from_bn {}'.format((N, H, W)))
        # h13: 5x5 / 2 transposed conv 64 -> 3, de-normalise + clip
        x = rs.normal(0, 1, (N, 64, H, W)).astype(np.float32)
        w = rs.normal(0, 0.1, (5, 5, 3, 64)).astype(np.float32)
        sc, sh = _bn(rs, 3)
        y = torch.full((N, 3, 2 * H, 2 * W), float('nan'), device=cuda)
        t = [d(x), d(w), d(sc), d(sh)]
        for tpw in (0, 1, 3):
            y.fill_(float('nan'))
            L.check(L.lib.ic_deconv2d_bn_act_f32(L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), L.ptr(t[3]), L.ptr(y), N, 64, H, W, 3, 5, 5, 0,
                                                 L.ptr(m_d), L.ptr(s_d), L.edge_tiles_per_wg(tpw), st))
            torch.cuda.synchronize()
            assert_close(y, _ref_conv(x, w, sc, sh, 2, 0, transposed=True, denorm=True), 'h13 {} tpw {}'.format((N, H, W), tpw))


@pytest.mark.parametrize('N,H,W', [(1, 136, 240), (2, 136, 240)])
def test_winograd_hybrid_plan(cuda, N, H, W):
    """272 / 544 tile groups next to a CU-range stream (IC_CONV3_LEAVE_IDLE_CUS): the full rounds of 256 run whole-K, the
    remainder (16 / 32 groups) K-split, in two launches of one call; every output tile is written exactly once and agrees
    with the single-form launches."""
    L = _lib()
    rs = np.random.RandomState(5)
    w = rs.normal(0, 0.05, (3, 3, 128, 128)).astype(np.float32)
    scale, shift = _bn(rs, 128)
    wd, sd, hd = dev(w, cuda), dev(scale, cuda), dev(shift, cuda)
    wp = torch.empty(L.lib.ic_wino3x3_c128_packed_floats(), device=cuda)
    L.check(L.lib.ic_pack_wino3x3_c128_f32(L.ptr(wd), L.ptr(wp), 0, L.current_stream()))
    x = torch.randn((N, 128, H, W), device=cuda)
    r = torch.randn((N, 128, H, W), device=cuda)
    groups = N * -(-H // 4) * -(-W // 32)
    assert groups % 256 in (16, 32)
    assert int(L.lib.ic_wino3x3_c128_workgroups(N, H, W, L.CONV3_LEAVE_IDLE_CUS)) == groups - groups % 256 + 4 * (groups % 256)
    outs = []
    for flags in (L.CONV3_LEAVE_IDLE_CUS, L.CONV3_WINO_WHOLEK, L.CONV3_WINO_KSPLIT, L.CONV3_AUTO):
        y = torch.full((N, 128, H, W), float('nan'), device=cuda)
        L.check(L.lib.ic_wino3x3_c128_bn_act_f32(L.ptr(x), L.ptr(wp), L.ptr(sd), L.ptr(hd), L.ptr(r), None, L.ptr(y), N, H, W, 1,
                                                 flags, L.current_stream()))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y).all())
        outs.append(y)
    scale_ = float(outs[1].abs().max())
    assert float((outs[0] - outs[1]).abs().max()) / scale_ < 2e-5
    assert float((outs[2] - outs[1]).abs().max()) / scale_ < 2e-5
    assert float((outs[3] - outs[1]).abs().max()) / scale_ < 2e-5
    # the whole-K part of the hybrid launch is the whole-K launch's own output, bit for bit
    gw = groups - groups % 256
    rows_w = (gw // (-(-W // 32))) % (-(-H // 4))       # tile-group rows of the last image fully inside the whole-K part
    if N == 1:
        assert torch.equal(outs[0][:, :, :4 * rows_w], outs[1][:, :, :4 * rows_w])


def test_two_host_threads_drive_the_library_concurrently(cuda):
    """the C ABI is re-entrant and keeps no process-wide mutable state.  Two host threads, each with its own
    stream and buffers, issue the same layer with DIFFERENT per-call plan flags at the same time; every result equals the
    single-threaded result of the same flags bit for bit (a shared tuning variable would let one thread's form leak into the
    other's launches: direct vs Winograd differ in the last bits)."""
    import threading
    L = _lib()
    rs = np.random.RandomState(11)
    w = rs.normal(0, 0.05, (3, 3, 128, 128)).astype(np.float32)
    scale, shift = _bn(rs, 128)
    wd, sd, hd = dev(w, cuda), dev(scale, cuda), dev(shift, cuda)
    wp = torch.empty(L.lib.ic_conv3x3_c128_both_packed_floats(), device=cuda)
    L.check(L.lib.ic_pack_conv3x3_c128_both_f32(L.ptr(wd), L.ptr(wp), 0, L.current_stream()))
    N, H, W = 1, 40, 72
    x = torch.randn((N, 128, H, W), device=cuda)
    forms = [L.CONV3_DIRECT, L.CONV3_WINO_SEG3, L.CONV3_WINO_WHOLEK | L.CONV3_LEAVE_IDLE_CUS, L.CONV3_WINO_KSPLIT]
    ref = []
    for f in forms:
        y = torch.empty_like(x)
        L.check(L.lib.ic_conv3x3_c128_auto_f32(L.ptr(x), L.ptr(wp), L.ptr(sd), L.ptr(hd), None, None, L.ptr(y), N, H, W, 1, f,
                                               L.current_stream()))
        ref.append(y)
    torch.cuda.synchronize()
    assert not torch.equal(ref[0], ref[1])
    errors = []

    def worker(tid):
        try:
            st = torch.cuda.Stream(device=cuda)
            ys = [torch.empty_like(x) for _ in forms]
            for it in range(200):
                k = (it + tid) % len(forms)
                rc = L.lib.ic_conv3x3_c128_auto_f32(L.ptr(x), L.ptr(wp), L.ptr(sd), L.ptr(hd), None, None, L.ptr(ys[k]), N, H, W, 1,
                                                    forms[k], st.cuda_stream)
                if rc != 0:
                    errors.append((tid, it, rc))
                    return
                if it % 50 == 49:
                    st.synchronize()
                    for j in range(len(forms)):
                        if it >= len(forms) and not torch.equal(ys[j], ref[j]):
                            errors.append((tid, it, 'form {:#x} differs'.format(forms[j])))
                            return
            st.synchronize()
        except Exception as e:                                             # noqa: BLE001 -- reported through the list
            errors.append((tid, repr(e)))
    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
