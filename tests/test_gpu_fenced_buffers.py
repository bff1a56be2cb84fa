"""-m gpu: every convolution, training and metric kernel once more through the C ABI with ALL device buffers from tests/fenced.py --
inputs between fences of NaN bit patterns, outputs and workspaces between fences of 0xA5, workspaces exactly *_workspace_bytes
long and handed over dirty.  The parity tests beside this file look inside the tensors; this one looks at where a kernel reads
and writes.  Every case asserts, in this order: the return code; the fences of every buffer; no NaN left in the output and the
float64 reference of the kernel's own parity test within that test's bound; where a workspace is taken, bit-identical outputs
over a 0xFF- and a 0x00-filled workspace; where workspace_bytes is taken, the refusal of one byte less with nothing touched.

Shapes are the smallest at which a kernel still has its ragged cases (tile rows of one or two valid rows, tiles beyond the map,
odd widths, more than one image).  The coverage manifest in tests/fenced.py names every entry point exercised here."""
import functools
import zlib

import numpy as np
import pytest
import torch

from tests import fenced as F
from tests.fenced import IN_FENCE, OUT_FENCE, ZERO_FENCE, check_fences, fenced, poison, same_bits
from tests.test_gpu_ops import NUM_VARIANTS, W4_RTOL, W5_RTOL, _bn, _ref_conv
from tests.util import HEATMAP_RTOL, RTOL, assert_close

pytestmark = pytest.mark.gpu

IC_OK, IC_ERR_WORKSPACE = 0, -3


def _L():
    from imgcomp_cvpr_amd import _lib
    return _lib


class Bufs(object):
    """the fenced buffers of one case: fin() an input (NaN fences), out() an output or workspace (0xA5 fences); done() is the
    first two assertions of every case"""

    def __init__(self, cuda):
        self.cuda, self.all = cuda, []

    def fin(self, a, name, dtype=torch.float32, fill=IN_FENCE):
        if a is None:
            return None
        v = fenced(a, dtype, self.cuda, fill, name)
        self.all.append(v)
        return v

    def out(self, shape, name, dtype=torch.float32):
        v = fenced(shape, dtype, self.cuda, OUT_FENCE, name)
        self.all.append(v)
        return v

    def ws(self, nbytes, name='workspace'):
        return self.out((int(nbytes),), name, torch.uint8)

    def done(self, rc, what=''):
        assert rc == IC_OK, '{}: return code {}'.format(what, rc)
        torch.cuda.synchronize()
        check_fences(*self.all)


def _written(y, what):
    assert not bool(torch.isnan(y).any()), '{}: {} output values are NaN (not written, or fed from a fence)'.format(what, int(torch.isnan(y).sum()))


def _close(y, ref, what, rtol):
    _written(y, what)
    assert_close(y, ref, 'fenced ' + what, rtol)


def _refill(*outs):
    for o in outs:
        if o is not None:
            if o.dtype.is_floating_point:
                o.fill_(float('nan'))
            else:
                poison(o, OUT_FENCE)


class _Poisoned(object):
    """a call over a dirty workspace, in the order every case keeps: constructing it fills the workspace with 0xFF, launches and checks
    the return code and the fences; the case then compares the values; again() fills the workspace with 0x00, launches once more, checks
    code and fences and asserts that the outputs have the bits of the first run.  The bytes from keep_from on are the
    caller-initialised part of a workspace and stay as prepared.  again() -> clones of the outputs"""

    def __init__(self, B, ws, outs, launch, what, keep_from=None):
        self.B, self.ws, self.launch, self.what, self.keep_from = B, ws, launch, what, keep_from
        self.outs = [o for o in outs if o is not None]
        self.first = self._run(0xFF)

    def _run(self, byte):
        poison(self.ws if self.keep_from is None else self.ws[:self.keep_from], byte)
        _refill(*self.outs)
        self.B.done(self.launch(), '{} over a {:#04x} workspace'.format(self.what, byte))
        return [o.clone() for o in self.outs]

    def again(self):
        second = self._run(0x00)
        for o, a, b in zip(self.outs, self.first, second):
            assert same_bits(a, b), '{}: {} depends on what the workspace held before the call'.format(self.what, o._fence[3])
        return second


def _one_byte_short(B, launch_short, what):
    """a workspace_bytes one less than needed: the workspace code, and every buffer and fence byte for byte as it was"""
    torch.cuda.synchronize()
    snap = F.snapshot(*B.all)
    rc = launch_short()
    torch.cuda.synchronize()
    assert rc == IC_ERR_WORKSPACE, '{}: a workspace one byte short returned {}'.format(what, rc)
    F.unchanged(snap, *B.all)


# ---- direct and edge convolutions -------------------------------------------------------------------------------------------

def _norm_consts():
    from oracle import oracle as O
    mean, std = O.norm_consts(torch.float32)
    return mean.flatten(), std.flatten()


@pytest.mark.parametrize('name,N,Cin,H,W,Cout,K,stride,relu,norm', [
    ('h1_odd', 2, 3, 37, 71, 64, 5, 2, 1, True),
    ('h1_1x1', 1, 3, 1, 1, 64, 5, 2, 1, True),
    ('odd_sizes', 1, 5, 13, 9, 7, 3, 1, 1, False),
    ('to_bn', 1, 128, 10, 14, 33, 5, 2, 0, False),
])
def test_conv2d_direct_and_h1(cuda, name, N, Cin, H, W, Cout, K, stride, relu, norm):
    L, B = _L(), Bufs(cuda)
    rs = np.random.RandomState(zlib.crc32(name.encode()) % 1000)
    x = (rs.uniform(0, 255, (N, Cin, H, W)) if norm else rs.normal(0, 1, (N, Cin, H, W))).astype(np.float32)
    w = rs.normal(0, 0.1, (K, K, Cin, Cout)).astype(np.float32)
    scale, shift = _bn(rs, Cout)
    OH, OW = -(-H // stride), -(-W // stride)
    res1 = rs.normal(0, 1, (N, Cout, OH, OW)).astype(np.float32)
    mean, std = _norm_consts()
    xd, wd, sd, hd, rd = B.fin(x, 'x'), B.fin(w, 'filter'), B.fin(scale, 'scale'), B.fin(shift, 'shift'), B.fin(res1, 'res1')
    md, td = (B.fin(mean, 'mean'), B.fin(std, 'std')) if norm else (None, None)
    y = B.out((N, Cout, OH, OW), 'y')
    B.done(L.lib.ic_conv2d_bn_act_f32(L.ptr(xd), L.ptr(wd), L.ptr(sd), L.ptr(hd), L.ptr(rd), None, L.ptr(y), N, Cin, H, W, Cout, K, K,
                                      stride, relu, L.ptr(md), L.ptr(td), L.current_stream()), name)
    _close(y, _ref_conv(x, w, scale, shift, stride, relu, res=(res1,), norm=norm), 'conv2d ' + name, RTOL)


@pytest.mark.parametrize('name,N,Cin,H,W,Cout,K,relu,denorm,tpws', [
    ('from_bn_tiles', 2, 32, 7, 37, 128, 3, 1, False, (0,)),
    ('h13_tiles', 1, 64, 19, 35, 3, 5, 0, True, (0, 1, 3)),
    ('h13_1x3', 1, 64, 1, 3, 3, 5, 0, True, (0, 1, 3)),
    ('odd', 1, 3, 5, 7, 5, 5, 0, False, (0,)),
])
def test_deconv2d_edge_layers(cuda, name, N, Cin, H, W, Cout, K, relu, denorm, tpws):
    L, B = _L(), Bufs(cuda)
    rs = np.random.RandomState(zlib.crc32(name.encode()) % 1000 + 1)
    x = rs.normal(0, 1, (N, Cin, H, W)).astype(np.float32)
    w = rs.normal(0, 0.1, (K, K, Cout, Cin)).astype(np.float32)
    scale, shift = _bn(rs, Cout)
    mean, std = _norm_consts()
    xd, wd, sd, hd = B.fin(x, 'x'), B.fin(w, 'filter'), B.fin(scale, 'scale'), B.fin(shift, 'shift')
    md, td = (B.fin(mean, 'mean'), B.fin(std, 'std')) if denorm else (None, None)
    y = B.out((N, Cout, 2 * H, 2 * W), 'y')
    ref = _ref_conv(x, w, scale, shift, 2, relu, transposed=True, denorm=denorm)
    for tpw in tpws:
        _refill(y)
        B.done(L.lib.ic_deconv2d_bn_act_f32(L.ptr(xd), L.ptr(wd), L.ptr(sd), L.ptr(hd), L.ptr(y), N, Cin, H, W, Cout, K, K, relu,
                                            L.ptr(md), L.ptr(td), L.edge_tiles_per_wg(tpw), L.current_stream()), name)
        _close(y, ref, 'deconv2d {} tiles per work-group {}'.format(name, tpw), RTOL)


# ---- strided matrix-core convolutions ------------------------------------------------------------------------------------------

def _pack(B, L, fn, w_np, n, *args):
    """a packer into a 0xA5-fenced output, fences checked; -> the fragments as a NaN-fenced input"""
    wd = B.fin(w_np, 'filter (TF layout)')
    wp = B.out((int(n),), 'packed filter (output of the packer)')
    B.done(fn(L.ptr(wd), L.ptr(wp), *args, L.current_stream()), 'packer')
    _written(wp, 'packed filter')
    return B.fin(wp, 'packed filter')


@pytest.mark.parametrize('name,N,Cin,H,W,Cout,transposed,relu', [
    ('h2_ragged', 2, 64, 14, 22, 128, 0, 1),
    ('to_bn_hi', 1, 128, 10, 18, 65, 0, 0),
    ('h12', 1, 128, 9, 13, 64, 1, 1),
    ('from_bn_adjoint_k3_odd', 1, 128, 11, 17, 64, 0, 1),
])
def test_conv2d_mfma_strided(cuda, name, N, Cin, H, W, Cout, transposed, relu):
    L, B = _L(), Bufs(cuda)
    K = 3 if '_k3' in name else 5
    rs = np.random.RandomState(zlib.crc32(name.encode()) % 1000 + 7)
    x = rs.normal(0, 1, (N, Cin, H, W)).astype(np.float32)
    w = rs.normal(0, 0.05, (K, K, Cout, Cin) if transposed else (K, K, Cin, Cout)).astype(np.float32)
    scale, shift = _bn(rs, Cout)
    n = L.lib.ic_conv2d_mfma_packed_floats(K, K, Cin, Cout, 2, transposed)
    assert n > 0
    wp = _pack(B, L, L.lib.ic_pack_conv2d_mfma_f32, w, n, K, K, Cin, Cout, 2, transposed)
    xd, sd, hd = B.fin(x, 'x'), B.fin(scale, 'scale'), B.fin(shift, 'shift')
    y = B.out((N, Cout, 2 * H, 2 * W) if transposed else (N, Cout, -(-H // 2), -(-W // 2)), 'y')
    B.done(L.lib.ic_conv2d_mfma_bn_act_f32(L.ptr(xd), L.ptr(wp), L.ptr(sd), L.ptr(hd), L.ptr(y), N, Cin, H, W, Cout, K, K, 2,
                                           transposed, relu, L.current_stream()), name)
    _close(y, _ref_conv(x, w, scale, shift, 2, relu, transposed=bool(transposed)), 'conv2d mfma ' + name, RTOL)


# ---- the 3x3 128 -> 128 layer in its forms ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _c3_inputs(N, H, W):
    rs = np.random.RandomState(5000 + 100 * N + 10 * H + W)
    x = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    w = rs.normal(0, 0.05, (3, 3, 128, 128)).astype(np.float32)
    scale, shift = _bn(rs, 128)
    r1 = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    r2 = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    return dict(x=x, w=w, scale=scale, shift=shift, r1=r1, r2=r2)


@functools.lru_cache(maxsize=None)
def _c3_raw64(N, H, W):
    """the float64 convolution of a map, made once and left unchanged; the epilogues are applied to it"""
    from oracle import oracle as O
    torch.set_num_threads(16)
    d = _c3_inputs(N, H, W)
    return O.conv2d_same(torch.as_tensor(d['x']).double(), d['w'], 1)


def _c3_ref64(N, H, W, relu, n_res):
    d = _c3_inputs(N, H, W)
    y = _c3_raw64(N, H, W) * torch.as_tensor(d['scale']).double().view(1, -1, 1, 1) + torch.as_tensor(d['shift']).double().view(1, -1, 1, 1)
    if relu:
        y = torch.relu(y)
    for r in (d['r1'], d['r2'])[:n_res]:
        y = y + torch.as_tensor(r).double()
    return y


EPILOGUES = ((1, 0), (0, 1), (0, 2))             # (relu, residuals)


def _c3_run(cuda, entry, packer, pack_floats, pack_args, N, H, W, flags, rtol, what, epilogues=EPILOGUES, inputs=None, ref=None):
    """one map through a 3x3 entry point (x, packed filter, scale, shift, residuals, y: all fenced) with each epilogue.  (Where a
    caller hands over an entry point that no case calls by name, it wraps it in a lambda that does: tests/test_cpu_fenced.py looks for
    `lib.<name>(` in this file.)"""
    L, B = _L(), Bufs(cuda)
    d = inputs or _c3_inputs(N, H, W)
    wp = _pack(B, L, packer, d['w'], pack_floats, *pack_args)
    xd, sd, hd = B.fin(d['x'], 'x'), B.fin(d['scale'], 'scale'), B.fin(d['shift'], 'shift')
    rd = [B.fin(d['r1'], 'res1'), B.fin(d['r2'], 'res2')]
    y = B.out((N, 128, H, W), 'y')
    for relu, n_res in epilogues:
        _refill(y)
        B.done(entry(L.ptr(xd), L.ptr(wp), L.ptr(sd), L.ptr(hd), L.ptr(rd[0]) if n_res >= 1 else None, L.ptr(rd[1]) if n_res >= 2 else None,
                     L.ptr(y), N, H, W, relu, flags, L.current_stream()), what)
        r64 = ref(relu, n_res) if ref is not None else _c3_ref64(N, H, W, relu, n_res)
        _close(y, r64, '{} {}x{}x{} relu {} res {}'.format(what, N, H, W, relu, n_res), rtol)


@pytest.mark.parametrize('variant,N,H,W', [(v, 1, 7, 5) for v in list(range(NUM_VARIANTS)) + [-1]] + [(-1, 2, 13, 21)])
def test_conv3x3_direct_mfma(cuda, variant, N, H, W):
    L = _L()
    flags = L.conv3_direct_variant(variant) if variant >= 0 else 0
    _c3_run(cuda, L.lib.ic_conv3x3_c128_bn_act_f32, (lambda *a: L.lib.ic_pack_conv3x3_c128_f32(*a)), L.lib.ic_conv3x3_c128_packed_floats(), (),
            N, H, W, flags, RTOL, 'conv3x3 mfma variant {}'.format(variant))


@pytest.mark.parametrize('form', ['auto', 'wholek', 'wholek_pw', 'ksplit', 'seg1', 'seg2', 'seg3', 'seg3_pk'])
@pytest.mark.parametrize('N,H,W', [(1, 7, 5), (2, 13, 21), (3, 10, 34)])
def test_conv3x3_winograd_f2(cuda, form, N, H, W):
    """ReLU without a residual, and two residuals, in every decomposition the shipped library has (t16 / pair: tuning builds)"""
    L = _L()
    flags = {'auto': 0, 'wholek': L.CONV3_WINO_WHOLEK, 'wholek_pw': L.CONV3_WINO_WHOLEK_PW, 'ksplit': L.CONV3_WINO_KSPLIT,
             'seg1': L.CONV3_WINO_SEG1, 'seg2': L.CONV3_WINO_SEG2, 'seg3': L.CONV3_WINO_SEG3,
             'seg3_pk': L.CONV3_WINO_SEG3 | L.CONV3_PACKED_TRANSFORM}[form]
    _c3_run(cuda, L.lib.ic_wino3x3_c128_bn_act_f32, L.lib.ic_pack_wino3x3_c128_f32, L.lib.ic_wino3x3_c128_packed_floats(), (0,),
            N, H, W, flags, RTOL, 'winograd F(2x2) ' + form, epilogues=((1, 0), (0, 2)))


def _adjoint_ref64(N, H, W):
    d = _c3_inputs(N, H, W)
    w_adj = np.ascontiguousarray(d['w'][::-1, ::-1].transpose(0, 1, 3, 2))
    return _ref_conv(d['x'], w_adj, np.ones(128, np.float32), np.zeros(128, np.float32), 1, 0)


def test_conv3x3_adjoint_packings(cuda):
    """both packings of ic_pack_wino3x3_c128_f32 / ic_pack_wino4_3x3_c128_f32 and ic_pack_conv3x3_c128_bwd_f32: the adjoint filter
    through each form's kernel against the conv with the flipped, channel-swapped filter (1 x 7 x 4: F(4x4) takes W % 4 == 0)"""
    L = _L()
    N, H, W = 1, 7, 4
    d = dict(_c3_inputs(N, H, W), scale=np.ones(128, np.float32), shift=np.zeros(128, np.float32))
    ref = _adjoint_ref64(N, H, W)
    for what, entry, packer, n, args, rtol in (
            ('direct', L.lib.ic_conv3x3_c128_bn_act_f32, (lambda *a: L.lib.ic_pack_conv3x3_c128_bwd_f32(*a)), L.lib.ic_conv3x3_c128_packed_floats(), (), RTOL),
            ('F(2x2)', L.lib.ic_wino3x3_c128_bn_act_f32, L.lib.ic_pack_wino3x3_c128_f32, L.lib.ic_wino3x3_c128_packed_floats(), (1,), RTOL),
            ('F(4x4)', (lambda *a: L.lib.ic_wino4_3x3_c128_bn_act_f32(*a)), L.lib.ic_pack_wino4_3x3_c128_f32, L.lib.ic_wino4_3x3_c128_packed_floats(), (1,), W4_RTOL)):
        _c3_run(cuda, entry, packer, n, args, N, H, W, 0, rtol, 'adjoint packing ' + what, epilogues=((0, 0),), inputs=d,
                ref=lambda relu, n_res: ref)


@pytest.mark.parametrize('f4', [0, 1])
@pytest.mark.parametrize('backward', [0, 1])
def test_batched_packers(cuda, f4, backward):
    """ic_pack_wino3x3_c128_batch_f32 / ic_pack_wino4_3x3_c128_batch_f32: three filters and the device table of their pointers
    fenced, the (3, n) output fenced; bit for bit the single packer's fragments (whose values the cases above check)"""
    L, B = _L(), Bufs(cuda)
    lib, st = L.lib, L.current_stream()
    rs = np.random.RandomState(11 + f4)
    ws = [B.fin(rs.normal(0, 0.05, (3, 3, 128, 128)).astype(np.float32), 'filter {}'.format(i)) for i in range(3)]
    # the pointer table is an integer input: it cannot hold a NaN, and a pointer read from either fill of its fence faults or reads
    # foreign memory -- 0x00 fences (a NULL pointer) and 0xFF fences must give the same fragments
    table = B.fin(torch.tensor([w.data_ptr() for w in ws], dtype=torch.int64), 'pointer table', torch.int64, ZERO_FENCE)
    n = lib.ic_wino4_3x3_c128_packed_floats() if f4 else lib.ic_wino3x3_c128_packed_floats()
    batch = B.out((3, n), 'packed batch')
    got = []
    for fill in (ZERO_FENCE, IN_FENCE):
        F.refence(table, fill)
        _refill(batch)
        if f4:
            B.done(lib.ic_pack_wino4_3x3_c128_batch_f32(L.ptr(table), L.ptr(batch), 3, backward, st), 'batched F(4x4) packer')
        else:
            B.done(lib.ic_pack_wino3x3_c128_batch_f32(L.ptr(table), L.ptr(batch), 3, backward, st), 'batched F(2x2) packer')
        _written(batch, 'packed batch')
        got.append(batch.clone())
    assert same_bits(got[0], got[1])
    for l, w in enumerate(ws):
        one = B.out((n,), 'packed single {}'.format(l))
        if f4:
            B.done(lib.ic_pack_wino4_3x3_c128_f32(L.ptr(w), L.ptr(one), backward, st), 'single packer')
        else:
            B.done(lib.ic_pack_wino3x3_c128_f32(L.ptr(w), L.ptr(one), backward, st), 'single packer')
        assert same_bits(batch[l], one), 'layer {}'.format(l)


# ---- F(4x4) ------------------------------------------------------------------------------------------------------------------

def _w4_maps():
    from tests import wino4_small_cases as C
    return C.C128_MAPS + [('7x4', 1, 7, 4, None)]


@pytest.mark.parametrize('m', _w4_maps(), ids=[m[0] for m in _w4_maps()])
def test_conv3x3_winograd_f4(cuda, m):
    """the maps of tests/wino4_small_cases.py (their inputs and float64 references) and 1 x 7 x 4: ReLU alone and two residuals"""
    from tests import wino4_small_cases as C
    L = _L()
    name, N, H, W, form = m
    flags = getattr(L, form) if form else L.CONV3_WINO4_WG4
    assert int(L.lib.ic_wino4_3x3_c128_waves(N, H, W, flags)) == (8 if form else 4)
    if name == '7x4':
        inputs, ref = None, None
    else:
        inputs, ref = C.c128_inputs(m), (lambda relu, n_res: C.c128_ref64(m, n_res, relu))
    _c3_run(cuda, (lambda *a: L.lib.ic_wino4_3x3_c128_bn_act_f32(*a)), L.lib.ic_pack_wino4_3x3_c128_f32, L.lib.ic_wino4_3x3_c128_packed_floats(), (0,),
            N, H, W, flags, W4_RTOL, 'winograd F(4x4) ' + name, epilogues=((1, 0), (0, 2)), inputs=inputs, ref=ref)


@pytest.mark.parametrize('m', _w4_maps(), ids=['{}x{}x{}'.format(*m[1:4]) for m in _w4_maps()])
def test_conv3x3_winograd_f4_stats_epilogue(cuda, m):
    """the training forward: raw output and the (128, parts, 2) per-segment sums, both fenced, on the same maps.  The stats entry has
    the 4-wave form only (csrc/conv3x3_wino4.hip, w4_launch_stats: of `flags` it reads IC_CONV3_NO_XCD_RUNS and nothing else), so the
    map that the plain entry runs with 8 waves is here one more 1 x 16-tile map and flags are 0 throughout."""
    from tests import wino4_small_cases as C
    L, B = _L(), Bufs(cuda)
    name, N, H, W, _ = m
    flags = 0
    d = _c3_inputs(N, H, W) if name == '7x4' else C.c128_inputs(m)
    raw64 = _c3_raw64(N, H, W) if name == '7x4' else C.c128_raw64(m)
    wp = _pack(B, L, L.lib.ic_pack_wino4_3x3_c128_f32, d['w'], L.lib.ic_wino4_3x3_c128_packed_floats(), 0)
    xd = B.fin(d['x'], 'x')
    parts = int(L.lib.ic_wino4_3x3_c128_stats_parts(N, H, W))
    assert parts >= 1
    raw, cst = B.out((N, 128, H, W), 'raw y'), B.out((128, parts, 2), 'stats')
    B.done(L.lib.ic_wino4_3x3_c128_raw_stats_f32(L.ptr(xd), L.ptr(wp), L.ptr(raw), L.ptr(cst), N, H, W, flags, L.current_stream()), name)
    _close(raw, raw64, 'winograd F(4x4) stats/raw ' + name, W4_RTOL)
    _written(cst, 'stats')
    tot = cst.double().sum(dim=1).cpu()
    assert_close(tot[:, 0], raw.double().sum(dim=(0, 2, 3)).cpu(), 'fenced F(4x4) stats: channel sums ' + name, 1e-6)
    assert_close(tot[:, 1], (raw.double() ** 2).sum(dim=(0, 2, 3)).cpu(), 'fenced F(4x4) stats: channel sums of squares ' + name, 1e-6)


# ---- 5x5 / 2 layers over phases -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,H,W', [(1, 5, 4), (2, 13, 20), (1, 8, 64)])
def test_conv5s2_over_phases(cuda, N, H, W):
    L = _L()
    lib, st = L.lib, L.current_stream()
    assert lib.ic_wino4_conv5s2_supported(N, H, W) == 1
    rs = np.random.RandomState(900 + H)
    # ---- h2: space to depth, then the 3x3 over the phases
    B = Bufs(cuda)
    x = rs.normal(0, 1, (N, 64, 2 * H, 2 * W)).astype(np.float32)
    w = rs.normal(0, 0.03, (5, 5, 64, 128)).astype(np.float32)
    scale, shift = _bn(rs, 128)
    xd = B.fin(x, 'x')
    xs = B.out((N, 4 * 64, H, W), 'x as phases')
    B.done(lib.ic_space_to_depth2_f32(L.ptr(xd), L.ptr(xs), N, 64, 2 * H, 2 * W, st), 'space to depth')
    assert torch.equal(xs.view(N, 2, 2, 64, H, W), xd.view(N, 64, H, 2, W, 2).permute(0, 3, 5, 1, 2, 4))
    xs_in = B.fin(xs, 'x as phases (input)')
    wp = _pack(B, L, lib.ic_pack_wino4_conv5s2_f32, w, lib.ic_wino4_conv5s2_packed_floats(), 0)
    sd, hd = B.fin(scale, 'scale'), B.fin(shift, 'shift')
    y = B.out((N, 128, H, W), 'y')
    for relu in (1, 0):
        _refill(y)
        B.done(lib.ic_wino4_conv5s2_c64_c128_bn_act_f32(L.ptr(xs_in), L.ptr(wp), L.ptr(sd), L.ptr(hd), L.ptr(y), N, H, W, relu, 0, st), 'h2')
        _close(y, _ref_conv(x, w, scale, shift, 2, relu), 'h2 over phases {}x{}x{} relu {}'.format(N, H, W, relu), W5_RTOL)
    # ---- h12
    B = Bufs(cuda)
    x = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    w = rs.normal(0, 0.03, (5, 5, 64, 128)).astype(np.float32)
    scale, shift = _bn(rs, 64)
    wp = _pack(B, L, lib.ic_pack_wino4_conv5s2_f32, w, lib.ic_wino4_conv5s2_packed_floats(), 1)
    xd, sd, hd = B.fin(x, 'x'), B.fin(scale, 'scale'), B.fin(shift, 'shift')
    y = B.out((N, 64, 2 * H, 2 * W), 'y')
    for relu in (1, 0):
        _refill(y)
        B.done(lib.ic_wino4_deconv5s2_c128_c64_bn_act_f32(L.ptr(xd), L.ptr(wp), L.ptr(sd), L.ptr(hd), L.ptr(y), N, H, W, relu, 0, st), 'h12')
        _close(y, _ref_conv(x, w, scale, shift, 2, relu, transposed=True), 'h12 to phases {}x{}x{} relu {}'.format(N, H, W, relu), W5_RTOL)


@pytest.mark.parametrize('transposed', [0, 1])
def test_conv5s2_both_packer(cuda, transposed):
    """ic_pack_conv5s2_both_f32: the blob is ic_pack_conv2d_mfma_f32's fragments followed by ic_pack_wino4_conv5s2_f32's, bit for bit
    (the values of each: the strided and the phase cases above)"""
    L, B = _L(), Bufs(cuda)
    lib, st = L.lib, L.current_stream()
    w = np.random.RandomState(31 + transposed).normal(0, 0.03, (5, 5, 64, 128)).astype(np.float32)
    cin, cout = (128, 64) if transposed else (64, 128)
    nm, n4 = lib.ic_conv2d_mfma_packed_floats(5, 5, cin, cout, 2, transposed), lib.ic_wino4_conv5s2_packed_floats()
    assert lib.ic_conv5s2_both_packed_floats(transposed) == nm + n4
    wd = B.fin(w, 'filter')
    both, pm, p4 = B.out((nm + n4,), 'both'), B.out((nm,), 'mfma fragments'), B.out((n4,), 'phase fragments')
    B.done(lib.ic_pack_conv5s2_both_f32(L.ptr(wd), L.ptr(both), transposed, st), 'both packer')
    B.done(lib.ic_pack_conv2d_mfma_f32(L.ptr(wd), L.ptr(pm), 5, 5, cin, cout, 2, transposed, st), 'mfma packer')
    B.done(lib.ic_pack_wino4_conv5s2_f32(L.ptr(wd), L.ptr(p4), transposed, st), 'phase packer')
    _written(both, 'both')
    assert same_bits(both[:nm], pm) and same_bits(both[nm:], p4)


# ---- the automatic 3x3 entry ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('form', ['AUTO', 'WINO4'])
@pytest.mark.parametrize('N,H,W', [(1, 1, 1), (1, 2, 3), (2, 7, 66)])
def test_conv3x3_auto_entry(cuda, form, N, H, W):
    """the `both` blob (direct | F(2x2) | F(4x4) fragments) through ic_conv3x3_c128_auto_f32; IC_CONV3_WINO4 on a width that is no
    multiple of 4 falls to F(2x2) by the library's own rule"""
    L = _L()
    flags = getattr(L, 'CONV3_' + form)
    f4 = L.lib.ic_conv3x3_c128_pick_form(N, H, W, flags) == 2
    _c3_run(cuda, L.lib.ic_conv3x3_c128_auto_f32, (lambda *a: L.lib.ic_pack_conv3x3_c128_both_f32(*a)), L.lib.ic_conv3x3_c128_both_packed_floats(), (0,),
            N, H, W, flags, W4_RTOL if f4 else RTOL, 'auto entry ' + form)


# ---- quantiser, sums, frequency tables ----------------------------------------------------------------------------------------

CENTERS6 = np.linspace(-2, 2, 6).astype(np.float32)
COUNTS = [1, 255, 257, 2048 * 256 + 3]          # one thread, a partial block, a block and one, the grid-stride loop's tail


@pytest.mark.parametrize('count', COUNTS)
def test_quantize(cuda, count):
    """ic_quantize_f32, every output present, then each alone (the others NULL): symbols and qhard exactly the oracle's on the same
    z, qsoft within the bound of test_quantize_bit_exact_symbols"""
    from oracle import oracle as O
    L, B = _L(), Bufs(cuda)
    z = np.random.RandomState(count % 1000).normal(0, 1.5, count).astype(np.float32)
    _, rh, rsym = O.quantize(torch.as_tensor(z), CENTERS6, 1.0)
    rs64, _, _ = O.quantize(torch.as_tensor(z).double(), CENTERS6.astype(np.float64), 1.0)
    zd, cd = B.fin(z, 'z'), B.fin(CENTERS6, 'centers')
    qs, qh, sym = B.out((count,), 'qsoft'), B.out((count,), 'qhard'), B.out((count,), 'symbols', torch.int64)
    full = None
    for want in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        _refill(qs, qh, sym)
        B.done(L.lib.ic_quantize_f32(L.ptr(zd), L.ptr(cd), 6, 1.0, L.ptr(qs) if want[0] else None, L.ptr(qh) if want[1] else None,
                                     L.ptr(sym) if want[2] else None, count, L.current_stream()), 'quantize')
        if want == (1, 1, 1):
            assert torch.equal(sym.cpu(), rsym) and torch.equal(qh.cpu(), rh)
            _close(qs, rs64, 'qsoft count {}'.format(count), 1e-6)
            full = [t.clone() for t in (qs, qh, sym)]
        else:
            for t, f, w in zip((qs, qh, sym), full, want):
                if w:
                    assert same_bits(t, f)
                elif t.dtype.is_floating_point:
                    assert bool(torch.isnan(t).all()), 'an output passed as NULL was written'
                else:
                    assert bool((t.view(torch.uint8) == OUT_FENCE).all()), 'an output passed as NULL was written'


def _hq_outputs(B, rows, C, h, w):
    o = [B.out((rows, C, h, w), n) for n in ('heatmap', 'z', 'qsoft', 'qhard', 'qbar')]
    return o + [B.out((rows, C, h, w), 'symbols', torch.int64)]


def test_heatmap_quantize_and_cap(cuda):
    """2 x (32 + 1) x 9 x 13: ic_heatmap_quantize_f32 against the oracle as test_heatmap_quantize does; ic_heatmap_quantize_cap_f32 with
    T = 3 planes a image against tests/cap_rule.py on the uncapped kernel's heatmap, bit for bit (tests/test_gpu_codec_cap.py);
    then with the optional outputs NULL"""
    from oracle import oracle as O
    from tests import cap_rule as R
    from tests.test_gpu_codec_cap import _random_plane
    L, B = _L(), Bufs(cuda)
    N, C, h, w, T = 2, 32, 9, 13, 3
    bott = np.random.RandomState(5).normal(0, 2, (N, C + 1, h, w)).astype(np.float32)
    bd, cd = B.fin(bott, 'bottleneck'), B.fin(CENTERS6, 'centers')
    hm, z, qs, qh, qb, sym = _hq_outputs(B, N, C, h, w)
    B.done(L.lib.ic_heatmap_quantize_f32(L.ptr(bd), L.ptr(cd), 6, 1.0, L.ptr(hm), L.ptr(z), L.ptr(qs), L.ptr(qh), L.ptr(qb), L.ptr(sym),
                                         N, C, h, w, L.current_stream()), 'heatmap quantize')
    b64 = torch.as_tensor(bott).double()
    hm64 = O.heatmap3d(b64)
    _close(hm, hm64, 'heatmap', 1e-5)
    _close(z, hm64 * b64[:, 1:], 'z', 1e-5)
    _written(qs, 'qsoft')
    _, rh, rsym = O.quantize(z.cpu(), CENTERS6, 1.0)
    assert torch.equal(sym.cpu(), rsym) and torch.equal(qh.cpu(), rh)
    assert torch.equal(qb.cpu(), (qs + (qh - qs)).cpu())
    plain = [t.clone() for t in (hm, z, qs, qh, qb, sym)]
    # the importance map alone (the other outputs NULL)
    _refill(hm, z, qs, qh, qb, sym)
    B.done(L.lib.ic_heatmap_quantize_f32(L.ptr(bd), L.ptr(cd), 6, 1.0, L.ptr(hm), L.ptr(z), None, None, None, L.ptr(sym),
                                         N, C, h, w, L.current_stream()), 'heatmap quantize, NULL outputs')
    assert same_bits(hm, plain[0]) and same_bits(z, plain[1]) and same_bits(sym, plain[5])
    assert bool(torch.isnan(qs).all()) and bool(torch.isnan(qh).all()) and bool(torch.isnan(qb).all())
    # and the complement: the quantiser outputs alone (heatmap, z and the symbols NULL)
    _refill(hm, z, qs, qh, qb, sym)
    B.done(L.lib.ic_heatmap_quantize_f32(L.ptr(bd), L.ptr(cd), 6, 1.0, None, None, L.ptr(qs), L.ptr(qh), L.ptr(qb), None,
                                         N, C, h, w, L.current_stream()), 'heatmap quantize, the other outputs NULL')
    assert same_bits(qs, plain[2]) and same_bits(qh, plain[3]) and same_bits(qb, plain[4])
    assert bool(torch.isnan(hm).all()) and bool(torch.isnan(z).all()) and bool((sym.view(torch.uint8) == OUT_FENCE).all())
    # ---- the cap, T = 3
    caps = _random_plane(np.random.RandomState(103), C, N * T, h, w)
    capd = B.fin(caps, 'cap')
    o = _hq_outputs(B, N * T, C, h, w)
    B.done(L.lib.ic_heatmap_quantize_cap_f32(L.ptr(bd), L.ptr(capd), T, L.ptr(cd), 6, 1.0, *[L.ptr(t) for t in o], N, C, h, w,
                                             L.current_stream()), 'heatmap quantize cap')
    for t in o[:5]:
        _written(t, 'capped ' + t._fence[3])
    m = plain[0].cpu().numpy()
    for n in range(N):
        for t in range(T):
            i = n * T + t
            m2, z2 = R.from_heatmap(m[n:n + 1], caps[i:i + 1], bott[n:n + 1, 1:])
            assert np.array_equal(o[0][i:i + 1].cpu().numpy().view(np.uint32), m2.view(np.uint32)), (n, t)
            assert np.array_equal(o[1][i:i + 1].cpu().numpy().view(np.uint32), z2.view(np.uint32)), (n, t)
    _, rh, rsym = O.quantize(o[1].cpu(), CENTERS6, 1.0)
    assert torch.equal(o[5].cpu(), rsym) and torch.equal(o[3].cpu(), rh)
    assert torch.equal(o[4], o[2] + (o[3] - o[2]))
    full = [t.clone() for t in o]
    _refill(*o)
    B.done(L.lib.ic_heatmap_quantize_cap_f32(L.ptr(bd), L.ptr(capd), T, L.ptr(cd), 6, 1.0, None, None, None, L.ptr(o[3]), None, L.ptr(o[5]),
                                             N, C, h, w, L.current_stream()), 'heatmap quantize cap, NULL outputs')
    assert same_bits(o[3], full[3]) and same_bits(o[5], full[5])
    for t in (o[0], o[1], o[2], o[4]):
        assert bool(torch.isnan(t).all()), 'an output passed as NULL was written'
    _refill(*o)
    B.done(L.lib.ic_heatmap_quantize_cap_f32(L.ptr(bd), L.ptr(capd), T, L.ptr(cd), 6, 1.0, L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]), None, L.ptr(o[4]), None,
                                             N, C, h, w, L.current_stream()), 'heatmap quantize cap, the other outputs NULL')
    for i in (0, 1, 2, 4):
        assert same_bits(o[i], full[i])
    assert bool(torch.isnan(o[3]).all()) and bool((o[5].view(torch.uint8) == OUT_FENCE).all()), 'an output passed as NULL was written'


@pytest.mark.parametrize('count', COUNTS)
def test_sums_and_means(cuda, count):
    """ic_sum_f32, ic_mean_f32, ic_mean_rows_f32 (3 rows): the 1024-float scratch is a workspace -- exactly that long, dirty both
    ways; against the float64 sum within 1e-6 of itself (test_sum_and_bpp)"""
    L, B = _L(), Bufs(cuda)
    rows = 3
    v = np.random.RandomState(9 + count % 97).uniform(0, 3, (rows, count)).astype(np.float32)
    vd = B.fin(v, 'values')
    partial = B.out((1024,), 'partial')
    out1, out3 = B.out((1,), 'out'), B.out((rows,), 'out rows')
    st = L.current_stream()
    ref = v.astype(np.float64).sum(axis=1)
    denom = 7.0

    def near(got, want, what):
        assert abs(got - want) <= 1e-6 * abs(want), '{}: {} against {}'.format(what, got, want)
    run = _Poisoned(B, partial, [out1], lambda: L.lib.ic_sum_f32(L.ptr(vd), count, L.ptr(partial), L.ptr(out1), st), 'sum')
    _written(out1, 'sum')
    near(float(out1[0]), ref[0], 'sum of {}'.format(count))
    run.again()
    run = _Poisoned(B, partial, [out1], lambda: L.lib.ic_mean_f32(L.ptr(vd), count, denom, L.ptr(partial), L.ptr(out1), st), 'mean')
    _written(out1, 'mean')
    near(float(out1[0]), ref[0] / denom, 'mean of {}'.format(count))
    run.again()
    run = _Poisoned(B, partial, [out3], lambda: L.lib.ic_mean_rows_f32(L.ptr(vd), rows, count, denom, L.ptr(partial), L.ptr(out3), st), 'mean rows')
    _written(out3, 'mean rows')
    for r in range(rows):
        near(float(out3[r]), ref[r] / denom, 'mean of row {} of {}'.format(r, count))
    run.again()


@pytest.mark.parametrize('count', COUNTS)
def test_logits_to_freqs(cuda, count):
    """freqs = max(int64(softmax(logits) * resolution), 1), pr = softmax(logits): pr against the float64 softmax at RTOL, the tables at
    the same bar relative to the resolution; pr NULL leaves the tables' bits"""
    L, B = _L(), Bufs(cuda)
    res = 1e9
    logits = np.maximum(np.random.RandomState(count % 991).normal(0.5, 2, (count, 6)), 0).astype(np.float32)
    ld = B.fin(logits, 'logits')
    freqs, pr = B.out((count, 6), 'freqs', torch.int64), B.out((count, 6), 'pr')
    B.done(L.lib.ic_pc_logits_to_freqs_f32(L.ptr(ld), count, 6, res, L.ptr(freqs), L.ptr(pr), L.current_stream()), 'freqs')
    p64 = torch.softmax(torch.as_tensor(logits).double(), -1)
    _close(pr, p64, 'freqs: pr, count {}'.format(count), RTOL)
    assert int(freqs.min()) >= 1
    assert_close(freqs.double() / res, torch.clamp(p64, min=1.0 / res), 'fenced freqs / resolution, count {}'.format(count), RTOL)
    with_pr = freqs.clone()
    _refill(freqs, pr)
    B.done(L.lib.ic_pc_logits_to_freqs_f32(L.ptr(ld), count, 6, res, L.ptr(freqs), None, L.current_stream()), 'freqs, pr NULL')
    assert same_bits(freqs, with_pr) and bool(torch.isnan(pr).all())


# ---- context model, forward -------------------------------------------------------------------------------------------------------

def _pc_table(B, L, k, nl):
    """the eight filter / bias tensors of tests/pc_cases.py's weights fenced, and the packed fragments made by ic_pc_pack_filters_f32
    into a fenced output -> (tensors, host table with the packed filters, host table without)"""
    from tests import pc_cases as P
    wts = P.weights(k, nl)
    tabs = []
    for layer, scope in P.SCOPES.items():
        tabs += [B.fin(wts[scope + '/weights'], layer + ' filter'), B.fin(wts[scope + '/biases'], layer + ' bias')]
    n = L.lib.ic_pc_packed_floats(k, nl)
    assert n > 0
    packed = B.out((n,), 'packed filters (output of the packer)')
    B.done(L.lib.ic_pc_pack_filters_f32(L.ptr_table(tabs + [None]), k, nl, L.ptr(packed), L.current_stream()), 'pc packer')
    _written(packed, 'packed filters')
    tabs.append(B.fin(packed, 'packed filters'))
    return tabs, L.ptr_table(tabs), L.ptr_table(tabs[:8] + [None])


@pytest.mark.parametrize('shape', [(2, 5, 7, 11), (1, 1, 1, 1)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('k', [24, 64])
def test_pc_forward(cuda, k, shape):
    """ic_pc_bitcost_f32 (packed table and per-call packing), ic_pc_logits_f32 and ic_pc_logits_padded_f32 against the float64 oracle
    of tests/pc_cases.py at RTOL.  The symbols are an integer input: fences of 0x00 and of 0xFF, the same bits."""
    from oracle import oracle as O
    from tests import pc_cases as P
    L, B = _L(), Bufs(cuda)
    lib, st = L.lib, L.current_stream()
    nl = 6
    N, C, h, w = shape
    tabs, tab, tab_unpacked = _pc_table(B, L, k, nl)
    q, sym, pad = P.inputs(k, nl, shape)
    rb, rl = P.reference(k, nl, shape)
    qd = B.fin(q, 'q')
    symd = B.fin(sym, 'symbols', torch.int64, ZERO_FENCE)
    need = lib.ic_pc_workspace_bytes(N, C, h, w, k)
    ws = B.ws(need)
    logits, bits = B.out((N, C, h, w, nl), 'logits'), B.out((N, C, h, w), 'bits')
    what = 'pc k {} shape {}'.format(k, shape)
    seen = []
    for fill in (ZERO_FENCE, IN_FENCE):
        F.refence(symd, fill)
        for t in (tab, tab_unpacked):
            run = _Poisoned(B, ws, [logits, bits], lambda: lib.ic_pc_bitcost_f32(
                L.ptr(qd), L.ptr(symd), t, k, nl, pad, L.ptr(logits), L.ptr(bits), N, C, h, w, L.ptr(ws), need, st), what + ' bitcost')
            if not seen:
                _close(logits, rl, what + ' logits', RTOL)
                _close(bits, rb, what + ' bits', RTOL)
            seen.append(run.again())
    for got in seen[1:]:
        assert same_bits(got[0], seen[0][0]) and same_bits(got[1], seen[0][1]), 'bitcost: other bits with other symbol fences or per-call packing'
    _one_byte_short(B, lambda: lib.ic_pc_bitcost_f32(L.ptr(qd), L.ptr(symd), tab, k, nl, pad, L.ptr(logits), L.ptr(bits), N, C, h, w,
                                                     L.ptr(ws), need - 1, st), what + ' bitcost')
    # bits alone (logits NULL)
    keep = logits.clone()
    _refill(bits)
    B.done(lib.ic_pc_bitcost_f32(L.ptr(qd), L.ptr(symd), tab, k, nl, pad, None, L.ptr(bits), N, C, h, w, L.ptr(ws), need, st), what)
    assert same_bits(bits, seen[0][1]) and same_bits(logits, keep)
    # logits alone
    run = _Poisoned(B, ws, [logits], lambda: lib.ic_pc_logits_f32(L.ptr(qd), tab, k, nl, pad, L.ptr(logits), N, C, h, w, L.ptr(ws), need, st),
                    what + ' logits entry')
    assert same_bits(logits, seen[0][0])                  # the values: those of the bitcost entry, compared with the oracle above
    run.again()
    _one_byte_short(B, lambda: lib.ic_pc_logits_f32(L.ptr(qd), tab, k, nl, pad, L.ptr(logits), N, C, h, w, L.ptr(ws), need - 1, st), what + ' logits')
    # the pre-padded volume
    qp = O.pad_for_probclass3d(torch.as_tensor(q), 9, pad)
    assert tuple(qp.shape) == (N, C + 4, h + 8, w + 8)
    vol = B.fin(qp, 'padded volume')
    run = _Poisoned(B, ws, [logits], lambda: lib.ic_pc_logits_padded_f32(L.ptr(vol), tab, k, nl, L.ptr(logits), N, C + 4, h + 8, w + 8,
                                                                          L.ptr(ws), need, st), what + ' padded entry')
    assert same_bits(logits, seen[0][0])
    run.again()
    _one_byte_short(B, lambda: lib.ic_pc_logits_padded_f32(L.ptr(vol), tab, k, nl, L.ptr(logits), N, C + 4, h + 8, w + 8, L.ptr(ws), need - 1, st),
                    what + ' padded')


# ---- context model, backward --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,vol', [(2, 5 * 7 * 11), (1, 1)])
def test_pc_dlogits(cuda, N, vol):
    """as test_pc_dlogits of tests/test_gpu_train_kernels.py (float64 autograd, 1e-5), L = 6; the symbols with both fence fills"""
    L, B = _L(), Bufs(cuda)
    nl = 6
    rs = np.random.RandomState(nl + vol)
    pre = rs.normal(0.3, 1.5, (N, vol, nl)).astype(np.float32)
    pre[:, :, 0] = -1.0
    pre[:, :, nl - 1] = np.abs(pre[:, :, nl - 1]) + 0.1
    logits = np.maximum(pre, 0).astype(np.float32)
    sym = rs.randint(0, nl, (N, vol)).astype(np.int64)
    sym[:, ::7] = 0
    dbits = rs.normal(0, 1, (N, vol)).astype(np.float32)
    pt = torch.tensor(pre, dtype=torch.float64, requires_grad=True)
    lg = torch.log_softmax(torch.relu(pt), -1)
    nll = -torch.gather(lg, -1, torch.as_tensor(sym).unsqueeze(-1)).squeeze(-1) * float(np.log2(np.e))
    (nll * torch.as_tensor(dbits, dtype=torch.float64)).sum().backward()
    ref = pt.grad.permute(0, 2, 1)
    ld, bd = B.fin(logits, 'logits'), B.fin(dbits, 'd_bits')
    sd = B.fin(sym, 'symbols', torch.int64, ZERO_FENCE)
    g = B.out((N, nl, vol), 'g')
    got = []
    for fill in (ZERO_FENCE, IN_FENCE):
        F.refence(sd, fill)
        _refill(g)
        B.done(L.lib.ic_pc_dlogits_f32(L.ptr(ld), L.ptr(sd), L.ptr(bd), L.ptr(g), N, vol, nl, L.current_stream()), 'dlogits')
        got.append(g.clone())
    _close(g, ref, 'pc dlogits N {} vol {}'.format(N, vol), 1e-5)
    assert same_bits(got[0], got[1])


@pytest.mark.parametrize('N,OD,OH,OW', [(2, 5, 7, 11), (1, 1, 1, 1)])
@pytest.mark.parametrize('k', [24, 64])
def test_pc_data_gradient(cuda, k, N, OD, OH, OW):
    """ic_pc_bwd_data_f32, k -> k with the ReLU mask (and the residual where the volume has one): the matrix-core path over its
    workspace and the VALU kernel without one, against float64 autograd at 1e-5 (test_pc_data_gradient_matrix_core_path)"""
    import torch.nn.functional as TF
    from oracle import oracle as O
    L, B = _L(), Bufs(cuda)
    st = L.current_stream()
    rs = np.random.RandomState(k + OD)
    with_res = OD > 1
    g = rs.normal(0, 1, (N, k, OD, OH, OW)).astype(np.float32)
    w = rs.normal(0, 0.1, (2, 3, 3, k, k)).astype(np.float32)
    act = rs.normal(0, 1, (N, k, OD + 1, OH + 2, OW + 2)).astype(np.float32)
    res = rs.normal(0, 1, (N, k, OD - 1, OH - 2, OW - 2)).astype(np.float32) if with_res else None
    _, other = O.pc_masks(3)
    xt = torch.zeros((N, k, OD + 1, OH + 2, OW + 2), dtype=torch.float64, requires_grad=True)
    wm = (torch.as_tensor(w).double() * torch.as_tensor(other, dtype=torch.float64)[..., None, None]).permute(4, 3, 0, 1, 2)
    TF.conv3d(xt, wm).backward(torch.as_tensor(g).double())
    ref = xt.grad.clone()
    if with_res:
        ref[:, :, 2:2 + OD - 1, 2:2 + OH - 2, 2:2 + OW - 2] += torch.as_tensor(res).double()
    ref = ref * (torch.as_tensor(act) > 0)
    gd, wd, actd, resd = B.fin(g, 'g'), B.fin(w, 'filter'), B.fin(act, 'act'), B.fin(res, 'res')
    dx = B.out((N, k, OD + 1, OH + 2, OW + 2), 'dx')
    need = L.lib.ic_pc_bwd_data_workspace_bytes(N, k, k, OD, OH, OW)
    assert need > 0
    ws = B.ws(need)
    what = 'pc data gradient k {} {}x{}x{}x{}'.format(k, N, OD, OH, OW)

    def launch(ws_, nbytes):
        return L.lib.ic_pc_bwd_data_f32(L.ptr(gd), L.ptr(wd), L.ptr(resd), L.ptr(actd), L.ptr(dx), N, k, k, OD, OH, OW, 0, 1, L.ptr(ws_), nbytes, st)
    run = _Poisoned(B, ws, [dx], lambda: launch(ws, need), what)
    _close(dx, ref, what + ', matrix cores', 1e-5)
    run.again()
    _one_byte_short(B, lambda: launch(ws, need - 1), what)
    _refill(dx)
    B.done(launch(None, 0), what)
    _close(dx, ref, what + ', VALU', 1e-5)


@pytest.mark.parametrize('k,N,C,h,w', [(24, 1, 1, 1, 1), (64, 1, 1, 1, 1), (24, 1, 1, 2, 2), (64, 1, 1, 2, 2), (24, 2, 5, 7, 11), (64, 2, 5, 7, 11)])
def test_pc_filter_gradient(cuda, k, N, C, h, w):
    """ic_pc_wgrad_f32 in the four layer roles of test_pc_filter_gradient_layer_roles (its float64 autograd, 1e-5)"""
    import torch.nn.functional as TF
    from oracle import oracle as O
    from tests.test_gpu_train_kernels import _pc_layers
    L = _L()
    st = L.current_stream()
    nl = 6
    rs = np.random.RandomState(k * 1000 + nl * 10 + C)
    first, other = O.pc_masks(3)
    pad_value = float(CENTERS6[0])
    q = CENTERS6[rs.randint(0, 6, (N, C, h, w))]
    for role, A, Bc, VD, VH, VW, fm in _pc_layers(N, C, h, w, k, nl):
        B = Bufs(cuda)
        V = rs.normal(0, 1, (N, Bc, VD, VH, VW)).astype(np.float32)
        mask = torch.as_tensor(first if fm else other, dtype=torch.float64)[..., None, None]
        wt = torch.zeros((2, 3, 3, A, Bc), dtype=torch.float64, requires_grad=True)
        if fm:
            Ut = O.pad_for_probclass3d(torch.as_tensor(q, dtype=torch.float64), 9, pad_value).unsqueeze(1)
            Ud = None
        else:
            U = np.maximum(rs.normal(0, 1, (N, A, VD + 1, VH + 2, VW + 2)), 0).astype(np.float32)
            Ut = torch.as_tensor(U, dtype=torch.float64)
            Ud = B.fin(U, 'U')
        TF.conv3d(Ut, (wt * mask).permute(4, 3, 0, 1, 2)).backward(torch.as_tensor(V, dtype=torch.float64))
        need = L.lib.ic_pc_wgrad_workspace_bytes(N, A, Bc, VD, VH, VW)
        assert need > 0
        qd, Vd = (B.fin(q, 'q') if fm else None), B.fin(V, 'V')
        ws = B.ws(need)
        dw = B.out((2, 3, 3, A, Bc), 'dw')
        what = 'pc wgrad k {} {} {}x{}x{}x{}'.format(k, role, N, C, h, w)

        def launch(nbytes):
            return L.lib.ic_pc_wgrad_f32(L.ptr(Ud), L.ptr(qd), pad_value, L.ptr(Vd), L.ptr(dw), N, A, Bc, VD, VH, VW, fm, L.ptr(ws), nbytes, st)
        run = _Poisoned(B, ws, [dw], lambda: launch(need), what)
        dead = (mask[..., 0, 0] == 0)
        assert bool((dw.cpu()[dead] == 0).all()), '{}: a dead tap has a nonzero gradient'.format(role)
        _close(dw, wt.grad, what, 1e-5)
        run.again()
        _one_byte_short(B, lambda: launch(need - 1), what)


@pytest.mark.parametrize('N,C,M', [(1, 5, 1), (2, 64, 7), (3, 24, 12345)])
def test_channel_sum(cuda, N, C, M):
    """the workspace is ic_channel_sum_workspace_bytes(C), whatever N and M"""
    L, B = _L(), Bufs(cuda)
    x = np.random.RandomState(N * 7 + M).normal(0.5, 1, (N, C, M)).astype(np.float32)
    xd = B.fin(x, 'x')
    ws = B.ws(L.lib.ic_channel_sum_workspace_bytes(C))
    out = B.out((C,), 'sums')
    run = _Poisoned(B, ws, [out], lambda: L.lib.ic_channel_sum_f32(L.ptr(xd), L.ptr(out), N, C, M, L.ptr(ws), L.current_stream()), 'channel sum')
    _close(out, torch.as_tensor(x, dtype=torch.float64).sum(dim=(0, 2)), 'channel sum N*M={}'.format(N * M), 1e-6)
    run.again()


@pytest.mark.parametrize('heatmap,with_dhm,N,C,h,w', [(1, True, 2, 32, 9, 13), (1, False, 2, 32, 9, 13), (0, False, 2, 32, 9, 13),
                                                      (1, True, 1, 4, 363, 362)])
def test_quantizer_backward(cuda, heatmap, with_dhm, N, C, h, w):
    """ic_heatmap_quantize_bwd_f32 as test_quantizer_backward_training_size checks it (float64 autograd, 1e-5), at 2 x 9 x 13 and at
    363 x 362 > 512 x 256 positions with 4 channels: the grid-stride loop's second round over a workspace whose size depends on L only"""
    L, B = _L(), Bufs(cuda)
    nl = 6
    rs = np.random.RandomState(C + nl + 100 * heatmap + h)
    CB = C + heatmap
    bott = rs.normal(0, 1.5, (N, CB, h, w)).astype(np.float32)
    if heatmap:
        while True:                                 # keep sigmoid(z0) C out of the fp32 band of an integer (a clip edge), as the test named above
            s = torch.sigmoid(torch.as_tensor(bott[:, 0], dtype=torch.float64)).numpy() * C
            near = np.abs(s - np.round(s)) < 1e-4
            if not near.any():
                break
            bott[:, 0][near] += np.float32(1e-2)
    gq = rs.normal(0, 1, (N, C, h, w)).astype(np.float32)
    gh = rs.normal(0, 1, (N, C, h, w)).astype(np.float32) if (heatmap and with_dhm) else None
    ct = torch.tensor(CENTERS6, dtype=torch.float64, requires_grad=True)
    ar = torch.arange(C, dtype=torch.float64).view(1, C, 1, 1)
    bt = torch.tensor(bott, dtype=torch.float64, requires_grad=True)
    if heatmap:
        hm = torch.clamp(torch.clamp(torch.sigmoid(bt[:, 0:1]) * C - ar, max=1.0), min=0.0)
        z = hm * bt[:, 1:]
    else:
        z = bt
    qsoft = (torch.softmax(-(z.unsqueeze(-1) - ct) ** 2, -1) * ct).sum(-1)
    loss = (qsoft * torch.as_tensor(gq, dtype=torch.float64)).sum()
    if gh is not None:
        loss = loss + (hm * torch.as_tensor(gh, dtype=torch.float64)).sum()
    loss.backward()
    bd, cd, gqd, ghd = B.fin(bott, 'bottleneck'), B.fin(CENTERS6, 'centers'), B.fin(gq, 'd_qbar'), B.fin(gh, 'd_heatmap')
    ws = B.ws(L.lib.ic_heatmap_quantize_bwd_workspace_bytes(nl))
    db, dc = B.out((N, CB, h, w), 'd_bottleneck'), B.out((nl,), 'd_centers')
    run = _Poisoned(B, ws, [db, dc], lambda: L.lib.ic_heatmap_quantize_bwd_f32(
        L.ptr(bd), L.ptr(cd), nl, 1.0, L.ptr(gqd), L.ptr(ghd), L.ptr(db), L.ptr(dc), N, C, h, w, heatmap, L.ptr(ws), L.current_stream()),
        'quantiser backward')
    tag = 'quantiser bwd heatmap {} d_heatmap {} {}x{}x{}x{}'.format(heatmap, with_dhm, N, C, h, w)
    _close(db, bt.grad, tag + ': d bottleneck', 1e-5)
    _close(dc, ct.grad, tag + ': d centers', 1e-5)
    run.again()


@pytest.mark.parametrize('count', [1, 3, 5, 1023, 4 * 2048 * 256 + 4 * 77 + 3])
def test_fused_adam(cuda, count):
    """ic_adam_tf_f32: variable, m and v are updated in place between NaN fences, the gradient is only read (1e-6, as
    test_fused_adam_tail_and_grid_stride)"""
    L, B = _L(), Bufs(cuda)
    rs = np.random.RandomState(count % 9973)
    p, m, v = B.fin(rs.normal(0, 1, count), 'variable'), B.fin(rs.normal(0, 0.1, count), 'm'), B.fin(rs.uniform(1e-4, 1e-1, count), 'v')
    g = B.fin(rs.normal(0, 1, count), 'gradient')
    f = lambda t: float(np.float32(t))
    b1, b2, eps = f(0.9), f(0.999), f(1e-8)
    lr_t = f(3e-3 * np.sqrt(1.0 - 0.999) / (1.0 - 0.9))
    p0, m0, v0, g0 = (t.double().cpu() for t in (p, m, v, g))
    m_ref = b1 * m0 + (1.0 - b1) * g0
    v_ref = b2 * v0 + (1.0 - b2) * g0 * g0
    p_ref = p0 - lr_t * m_ref / (torch.sqrt(v_ref) + eps)
    B.done(L.lib.ic_adam_tf_f32(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), count, lr_t, b1, b2, eps, L.current_stream()), 'adam')
    _close(m, m_ref, 'fused Adam: m, count {}'.format(count), 1e-6)
    _close(v, v_ref, 'fused Adam: v, count {}'.format(count), 1e-6)
    _close(p, p_ref, 'fused Adam: variable, count {}'.format(count), 1e-6)
    assert torch.equal(g.double().cpu(), g0), 'the gradient was written'


# ---- filter gradients of the autoencoder -------------------------------------------------------------------------------------------

def _wg_cases():
    from tests.test_gpu_train_kernels import WG_CASES
    return WG_CASES


@pytest.mark.parametrize('name,A,Bc,N,H,W,K,stride,kind,wd', _wg_cases(), ids=[c[0] for c in _wg_cases()])
def test_conv2d_filter_gradient(cuda, name, A, Bc, N, H, W, K, stride, kind, wd):
    """ic_conv2d_wgrad_f32 on the plan forms of test_conv2d_filter_gradient_plan_forms (its float64 autograd, 1e-5): the slices
    workspace exactly ic_conv2d_wgrad_workspace_bytes, dirty both ways, and one byte less refused"""
    from oracle import train_oracle as T
    L, B = _L(), Bufs(cuda)
    rs = np.random.RandomState(sum(map(ord, name)))
    x = rs.normal(0, 1, (N, A if kind == 'conv' else Bc, H, W)).astype(np.float32)
    w = rs.normal(0, 0.1, (K, K, A, Bc)).astype(np.float32)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    xt = torch.tensor(x, dtype=torch.float64)
    y = T._conv(xt, wt, stride) if kind == 'conv' else T._deconv(xt, wt)
    dy = rs.normal(0, 1, tuple(y.shape)).astype(np.float32)
    y.backward(torch.tensor(dy, dtype=torch.float64))
    ref = wt.grad + (wd * wt.detach() if wd is not None else 0.0)
    if kind == 'conv':
        U, V, UH, UW = B.fin(x, 'U = x'), B.fin(dy, 'V = dy'), H, W
    else:
        U, V, UH, UW = B.fin(dy, 'U = dy'), B.fin(x, 'V = x'), 2 * H, 2 * W
    VH, VW = -(-UH // stride), -(-UW // stride)
    need = L.lib.ic_conv2d_wgrad_workspace_bytes(N, A, Bc, VH, VW, K, K)
    assert need > 0
    wdev = B.fin(w, 'filter') if wd is not None else None
    ws = B.ws(need)
    dw = B.out((K, K, A, Bc), 'dw')

    def launch(nbytes):
        return L.lib.ic_conv2d_wgrad_f32(L.ptr(U), L.ptr(V), L.ptr(dw), N, A, UH, UW, Bc, K, K, stride, L.ptr(wdev), wd or 0.0,
                                         L.ptr(ws), nbytes, L.current_stream())
    run = _Poisoned(B, ws, [dw], lambda: launch(need), 'conv2d wgrad ' + name)
    _close(dw, ref, 'conv2d wgrad ' + name, 1e-5)
    run.again()
    _one_byte_short(B, lambda: launch(need - 1), 'conv2d wgrad ' + name)


@pytest.mark.parametrize('N,H,W', [(1, 8, 16), (2, 6, 34)])
def test_winograd_filter_gradient(cuda, N, H, W):
    """ic_conv3x3_c128_wgrad_f32.  The producer's edge loads go through a buffer descriptor based two floats before x whose range
    covers those 8 bytes, so there the hardware range check does not stand in for the lane's own guard (tile column 0 has no left
    neighbour): a load that slipped through would take NaNs from the front fence of x into dw.  Everywhere else a stray offset is
    either dropped by the range check or lands on a neighbouring row inside x, which the parity test sees by its values.  What this
    case adds beyond that one place is the partials workspace: exactly ic_conv3x3_c128_wgrad_workspace_bytes, dirty both ways, fenced.
    1 x 8 x 16 is one chunk of tiles, 2 x 6 x 34 has a ragged chunk (17 tiles) and a second image; float64 autograd, 1e-5
    (test_winograd_filter_gradient)"""
    from oracle import train_oracle as T
    L, B = _L(), Bufs(cuda)
    rs = np.random.RandomState(N * 100 + H)
    x = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    dy = rs.normal(0, 1, (N, 128, H, W)).astype(np.float32)
    w = rs.normal(0, 0.1, (3, 3, 128, 128)).astype(np.float32)
    torch.set_num_threads(16)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    T._conv(torch.tensor(x, dtype=torch.float64), wt, 1).backward(torch.tensor(dy, dtype=torch.float64))
    ref = wt.grad + 0.25 * wt.detach()
    xd, dyd, wdev = B.fin(x, 'x'), B.fin(dy, 'dy'), B.fin(w, 'filter')
    need = L.lib.ic_conv3x3_c128_wgrad_workspace_bytes(N, H, W)
    assert need > 0
    ws = B.ws(need)
    dw = B.out((3, 3, 128, 128), 'dw')

    def launch(nbytes):
        return L.lib.ic_conv3x3_c128_wgrad_f32(L.ptr(xd), L.ptr(dyd), L.ptr(dw), N, H, W, L.ptr(wdev), 0.25, L.ptr(ws), nbytes, L.current_stream())
    run = _Poisoned(B, ws, [dw], lambda: launch(need), 'winograd wgrad')
    _close(dw, ref, 'dW winograd {}x{}x{}'.format(N, H, W), 1e-5)
    run.again()
    _one_byte_short(B, lambda: launch(need - 1), 'winograd wgrad')


# ---- data gradients: the adjoint dispatch paths of tests/dgrad_cases.py ------------------------------------------------------------

def _dgrad_a_cases():
    """per 3x3 adjoint path its smallest case driven through the C ABI, with both epilogue adds"""
    from tests import dgrad_cases as D
    want = {'direct': ('abi', (1, 3, 3)), 'f2_single': ('abi', (2, 13, 21)), 'f2_batch': ('abi', (2, 13, 21)), 'f4_batch': ('auto', (2, 13, 20))}
    out = []
    for path, (drive, shape) in want.items():
        out.append(next(c for c in D.A_CASES if c.path == path and c.drive == drive and (c.N, c.H, c.W) == shape and c.adds == 2))
    return out


def _dgrad_b_cases():
    """per strided adjoint path and configuration its smallest case (one row of 21 grid columns, one add)"""
    from tests import dgrad_cases as D
    return [c for c in D.B_CASES if c.adds == 1]


def _case_id(c):
    from tests import dgrad_cases as D
    return D.case_id(c)


@pytest.mark.parametrize('case', _dgrad_a_cases(), ids=_case_id)
def test_conv3x3_data_gradient_paths(cuda, case):
    from tests import dgrad_cases as D
    L, B = _L(), Bufs(cuda)
    lib, st = L.lib, L.current_stream()
    assert D.expected_plan(L, case)
    N, H, W = case.N, case.H, case.W
    g, adds = D.inputs(case)
    gd, r1, r2 = B.fin(g, 'g'), B.fin(adds[0], 'add1'), B.fin(adds[1], 'add2')
    ones, zeros = B.fin(np.ones(128, np.float32), 'scale'), B.fin(np.zeros(128, np.float32), 'shift')
    y = B.out((N, 128, H, W), 'dx')
    args = (L.ptr(ones), L.ptr(zeros), L.ptr(r1), L.ptr(r2), L.ptr(y), N, H, W, 0)
    w = D.filter_of(case)
    if case.drive == 'auto':
        wp = _pack(B, L, (lambda *a: lib.ic_pack_conv3x3_c128_both_f32(*a)), w, lib.ic_conv3x3_c128_both_packed_floats(), 1)
        B.done(lib.ic_conv3x3_c128_auto_f32(L.ptr(gd), L.ptr(wp), *args, D.auto_flags(L, case), st), case.path)
    elif case.path == 'direct':
        wp = _pack(B, L, (lambda *a: lib.ic_pack_conv3x3_c128_bwd_f32(*a)), w, lib.ic_conv3x3_c128_packed_floats())
        B.done(lib.ic_conv3x3_c128_bn_act_f32(L.ptr(gd), L.ptr(wp), *args, 0, st), case.path)
    elif case.path == 'f2_single':
        wp = _pack(B, L, lib.ic_pack_wino3x3_c128_f32, w, lib.ic_wino3x3_c128_packed_floats(), 1)
        B.done(lib.ic_wino3x3_c128_bn_act_f32(L.ptr(gd), L.ptr(wp), *args, 0, st), case.path)
    else:
        # the batched packer: the case's filter between two others, its fragments taken from the middle of the batch
        ws_ = [B.fin(D.random_filter(1), 'filter before'), B.fin(w, 'filter'), B.fin(D.random_filter(2), 'filter behind')]
        table = B.fin(torch.tensor([t.data_ptr() for t in ws_], dtype=torch.int64), 'pointer table', torch.int64, ZERO_FENCE)
        n = lib.ic_wino3x3_c128_packed_floats()
        batch = B.out((3, n), 'packed batch')
        B.done(lib.ic_pack_wino3x3_c128_batch_f32(L.ptr(table), L.ptr(batch), 3, 1, st), 'batched packer')
        wp = B.fin(batch[1], 'packed filter')
        B.done(lib.ic_wino3x3_c128_bn_act_f32(L.ptr(gd), L.ptr(wp), *args, 0, st), case.path)
    _close(y, D.reference(case), 'dX ' + D.case_id(case), D.rtol(case))


@pytest.mark.parametrize('case', _dgrad_b_cases(), ids=_case_id)
def test_strided_data_gradient_paths(cuda, case):
    """the calls TrainGraph._raw_backward_data makes for the layer (training.py: _conv_s / _deconv_s with scale 1, shift 0, the add
    made by torch afterwards), with fenced buffers"""
    from tests import dgrad_cases as D
    L, B = _L(), Bufs(cuda)
    lib, st = L.lib, L.current_stream()
    assert D.expected_plan(L, case)
    kh, kw, cin, cout, stride, tr = D.adjoint_call(case)
    g, adds = D.inputs(case)
    N, _, H, W = g.shape
    gd = B.fin(g, 'g')
    ones, zeros = B.fin(np.ones(cout, np.float32), 'scale'), B.fin(np.zeros(cout, np.float32), 'shift')
    dx = B.out(D.dx_shape(case), 'dx')
    assert tuple(dx.shape) == ((N, cout, 2 * H, 2 * W) if tr else (N, cout, -(-H // 2), -(-W // 2)))
    n = lib.ic_conv2d_mfma_packed_floats(kh, kw, cin, cout, stride, tr)
    if n:
        wp = _pack(B, L, lib.ic_pack_conv2d_mfma_f32, D.filter_of(case), n, kh, kw, cin, cout, stride, tr)
        B.done(lib.ic_conv2d_mfma_bn_act_f32(L.ptr(gd), L.ptr(wp), L.ptr(ones), L.ptr(zeros), L.ptr(dx), N, cin, H, W, cout, kh, kw, stride, tr, 0, st),
               case.path)
    elif tr:
        wd = B.fin(D.filter_of(case), 'filter')
        B.done(lib.ic_deconv2d_bn_act_f32(L.ptr(gd), L.ptr(wd), L.ptr(ones), L.ptr(zeros), L.ptr(dx), N, cin, H, W, cout, kh, kw, 0, None, None, 0, st),
               case.path)
    else:
        wd = B.fin(D.filter_of(case), 'filter')
        B.done(lib.ic_conv2d_bn_act_f32(L.ptr(gd), L.ptr(wd), L.ptr(ones), L.ptr(zeros), None, None, L.ptr(dx), N, cin, H, W, cout, kh, kw, stride, 0,
                                        None, None, st), case.path)
    _written(dx, case.path)
    got = dx
    for a in adds:
        got = got + torch.as_tensor(a).to(cuda)
    assert_close(got, D.reference(case), 'fenced dX ' + D.case_id(case), D.rtol(case))


# ---- BatchNorm ------------------------------------------------------------------------------------------------------------------------

class FencedBN(object):
    """the ic_bn_* entry points on NumPy arrays, the interface tests/bn_rule.py checks (as Device of tests/test_gpu_bn_kernels.py), with
    every tensor fenced, the workspace exactly ic_bn_workspace_bytes(C) and each call made over a 0xFF- and a 0x00-filled workspace:
    fences checked after each, the two results bit-identical"""

    def __init__(self, cuda):
        self.cuda, self.L, self.B, self._ws = cuda, _L(), Bufs(cuda), None
        self.st = self.L.current_stream()

    def put(self, a, dtype=torch.float32, name='input'):
        return self.B.fin(a, name, dtype)

    def nan(self, shape, dtype=torch.float32, name='output'):
        return self.B.out(tuple(shape), name, dtype)

    def ws(self, C):
        self._ws = self.B.ws(self.L.lib.ic_bn_workspace_bytes(C))
        return self._ws

    def _run(self, launch):
        runs = []
        for byte in (0xFF, 0x00):
            if self._ws is not None:
                poison(self._ws, byte)
            outs = launch()
            torch.cuda.synchronize()
            check_fences(*self.B.all)
            runs.append(outs)
        for u, v in zip(*runs):
            assert same_bits(u, v), 'a BatchNorm result depends on what the workspace held (or a second launch gives other bits)'
        self.B, self._ws = Bufs(self.cuda), None
        return [t.cpu() for t in runs[0]]

    def _ok(self, rc):
        assert rc == IC_OK, rc

    def moments(self, x):
        L, p = self.L, self.L.ptr
        N, C, H, W = x.shape
        xd, ws = self.put(x), self.ws(C)

        def launch():
            sums = self.nan((2, C), torch.float64)
            self._ok(L.lib.ic_bn_moments_f32(p(xd), p(sums), N, C, H * W, p(ws), self.st))
            return (sums,)
        return self._run(launch)[0]

    def stats(self, x):
        L, p = self.L, self.L.ptr
        N, C, H, W = x.shape
        xd, ws = self.put(x), self.ws(C)

        def launch():
            mean, var = self.nan((C,)), self.nan((C,))
            self._ok(L.lib.ic_bn_stats_f32(p(xd), p(mean), p(var), N, C, H * W, p(ws), self.st))
            return mean, var
        return self._run(launch)

    @staticmethod
    def _stats_dict(out, mm, mv):
        d = dict(zip(('mean', 'invstd', 'scale', 'shift'), out[:4]))
        rest = list(out[4:])
        if mm is not None:
            d['mm'] = rest.pop(0)
        if mv is not None:
            d['mv'] = rest.pop(0)
        return d

    def train_stats(self, x, gamma, beta, mm, mv):
        from tests import bn_rule as R
        L, p = self.L, self.L.ptr
        N, C, H, W = x.shape
        xd, gd, bd, ws = self.put(x), self.put(gamma), self.put(beta), self.ws(C)

        def launch():
            o = [self.nan((C,)) for _ in range(4)]
            m, v = self.put(mm), self.put(mv)
            self._ok(L.lib.ic_bn_train_stats_f32(p(xd), p(gd), p(bd), p(m), p(v), R.DECAY, R.EPS, p(o[0]), p(o[1]), p(o[2]), p(o[3]),
                                                 N, C, H * W, p(ws), self.st))
            return o + [t for t in (m, v) if t is not None]
        return self._stats_dict(self._run(launch), mm, mv)

    def fold_moments(self, sums, count, gamma, beta, mm, mv):
        from tests import bn_rule as R
        L, p = self.L, self.L.ptr
        C = len(gamma)
        sd, gd, bd = self.put(sums, torch.float64), self.put(gamma), self.put(beta)

        def launch():
            o = [self.nan((C,)) for _ in range(4)]
            m, v = self.put(mm), self.put(mv)
            self._ok(L.lib.ic_bn_train_fold_moments_f32(p(sd), count, p(gd), p(bd), p(m), p(v), R.DECAY, R.EPS, p(o[0]), p(o[1]), p(o[2]),
                                                        p(o[3]), C, self.st))
            return o + [t for t in (m, v) if t is not None]
        return self._stats_dict(self._run(launch), mm, mv)

    def train_forward(self, x, gamma, beta, mm, mv, res1, res2, relu):
        from tests import bn_rule as R
        L, p = self.L, self.L.ptr
        N, C, H, W = x.shape
        xd, gd, bd, r1, r2, ws = self.put(x), self.put(gamma), self.put(beta), self.put(res1), self.put(res2), self.ws(C)

        def launch():
            o = [self.nan((C,)) for _ in range(4)]
            m, v, y = self.put(mm), self.put(mv), self.nan(x.shape)
            self._ok(L.lib.ic_bn_train_forward_f32(p(xd), p(gd), p(bd), p(m), p(v), R.DECAY, R.EPS, p(o[0]), p(o[1]), p(o[2]), p(o[3]),
                                                   p(r1), p(r2), p(y), N, C, H * W, relu, p(ws), self.st))
            return o + [t for t in (m, v) if t is not None] + [y]
        out = self._run(launch)
        return self._stats_dict(out[:-1], mm, mv), out[-1]

    def apply(self, x, scale, shift, res1, res2, relu):
        L, p = self.L, self.L.ptr
        N, C, H, W = x.shape
        xd, sc, sh, r1, r2 = self.put(x), self.put(scale), self.put(shift), self.put(res1), self.put(res2)

        def launch():
            y = self.nan(x.shape)
            self._ok(L.lib.ic_bn_apply_f32(p(xd), p(sc), p(sh), p(r1), p(r2), p(y), N, C, H * W, relu, self.st))
            return (y,)
        return self._run(launch)[0]

    def backward_reduce(self, dy, x, scale, shift, mean, invstd, relu):
        L, p = self.L, self.L.ptr
        N, C, H, W = x.shape
        dyd, xd, ws = self.put(dy), self.put(x), self.ws(C)
        sc, sh, mu, inv = self.put(scale), self.put(shift), self.put(mean), self.put(invstd)

        def launch():
            sums, dgamma, dbeta = self.nan((2, C), torch.float64), self.nan((C,)), self.nan((C,))
            self._ok(L.lib.ic_bn_backward_reduce_f32(p(dyd), p(xd), p(sc), p(sh), p(mu), p(inv), p(sums), p(dgamma), p(dbeta), N, C, H * W,
                                                     relu, p(ws), self.st))
            return sums, dgamma, dbeta
        return self._run(launch)

    def backward(self, dy, x, scale, shift, mean, invstd, gamma, relu):
        L, p = self.L, self.L.ptr
        N, C, H, W = x.shape
        dyd, xd, gd, ws = self.put(dy), self.put(x), self.put(gamma), self.ws(C)
        sc, sh, mu, inv = self.put(scale), self.put(shift), self.put(mean), self.put(invstd)

        def launch():
            dx, dgamma, dbeta = self.nan(x.shape), self.nan((C,)), self.nan((C,))
            self._ok(L.lib.ic_bn_backward_f32(p(dyd), p(xd), p(sc), p(sh), p(mu), p(inv), p(gd), p(dx), p(dgamma), p(dbeta), N, C, H * W,
                                              relu, p(ws), self.st))
            return dx, dgamma, dbeta
        return self._run(launch)

    def backward_apply(self, dy, x, scale, shift, mean, invstd, gamma, sums, count, relu):
        L, p = self.L, self.L.ptr
        N, C, H, W = x.shape
        dyd, xd, gd, sd = self.put(dy), self.put(x), self.put(gamma), self.put(sums, torch.float64)
        sc, sh, mu, inv = self.put(scale), self.put(shift), self.put(mean), self.put(invstd)

        def launch():
            dx = self.nan(x.shape)
            self._ok(L.lib.ic_bn_backward_apply_f32(p(dyd), p(xd), p(sc), p(sh), p(mu), p(inv), p(gd), p(sd), count, p(dx), N, C, H * W,
                                                    relu, self.st))
            return (dx,)
        return self._run(launch)[0]


@pytest.mark.parametrize('name', ['a', 'c', 'd', 'i'])
@pytest.mark.parametrize('relu', [0, 1])
def test_batchnorm_entries_against_the_float64_rule(cuda, name, relu):
    """tests/bn_rule.check_case (the bounds of tests/test_gpu_bn_kernels.py) on (a) M = 1, (c) a ragged M = 2 x 63, (d) N = 5 with
    33 x 33 planes and (i) C = 130 > 64: the workspace does not grow with N or HW, only with C"""
    from tests import bn_rule as R
    R.check_case(FencedBN(cuda), name, relu)


@pytest.mark.parametrize('name', ['a', 'c', 'd', 'i'])
@pytest.mark.parametrize('relu', [0, 1])
def test_batchnorm_fused_forward(cuda, name, relu):
    """ic_bn_train_forward_f32 (which the rule's check_case does not call) on the same shapes, with two, one and no residual: the
    statistics and moving averages against the float64 rule at STAT_TOL, y against the rule's apply on the kernel's own scale and
    shift at OUT_TOL, and every output bit for bit what ic_bn_train_stats_f32 followed by ic_bn_apply_f32 give
    (test_fused_forward_is_stats_then_apply_bit_for_bit)"""
    from tests import bn_rule as R
    be, d = FencedBN(cuda), R.case_data(name)
    x, gamma, beta = d['x'], d['gamma'], d['beta']
    N, C, H, W = x.shape
    s, ss, _, _ = R.moments(x)
    ref = R.fold(s, ss, N * H * W, gamma, beta, d['mm'], d['mv'])
    st = be.train_stats(x, gamma, beta, d['mm'], d['mv'])
    for r1, r2, which in ((d['res1'], d['res2'], 'two residuals'), (d['res1'], None, 'one residual'), (None, None, 'no residual')):
        at = ', {} shape {} relu {}'.format(which, name, relu)
        fused, y = be.train_forward(x, gamma, beta, d['mm'], d['mv'], r1, r2, relu)
        assert not bool(torch.isnan(y).any())
        for k in R.STAT_KEYS:
            R.assert_scaled(fused[k], ref[k], R.STAT_TOL, 'fenced bn fused forward: ' + k + at)
            assert same_bits(fused[k], st[k]), 'fused forward: {} has other bits than ic_bn_train_stats_f32'.format(k) + at
        sc, sh = fused['scale'].numpy(), fused['shift'].numpy()
        R.assert_scaled(y, R.apply(x, sc, sh, r1, r2, relu), R.OUT_TOL, 'fenced bn fused forward: y' + at)
        assert same_bits(y, be.apply(x, sc, sh, r1, r2, relu)), 'fused forward: y has other bits than ic_bn_apply_f32' + at


def test_batchnorm_from_the_conv_epilogue_sums(cuda):
    """ic_bn_train_forward_cstats_f32 on the sums ic_wino4_3x3_c128_raw_stats_f32 left (2 x 32 x 32, both fenced) against the two-launch
    form on the same raw tensor, within 2e-6 (test_conv3x3_epilogue_batchnorm_sums)"""
    from tests import wino4_small_cases as C
    L, B = _L(), Bufs(cuda)
    st = L.current_stream()
    m = C.STATS_MAP
    _, N, H, W, _ = m
    d = C.c128_inputs(m)
    wp = _pack(B, L, L.lib.ic_pack_wino4_3x3_c128_f32, d['w'], L.lib.ic_wino4_3x3_c128_packed_floats(), 0)
    xd = B.fin(d['x'], 'x')
    parts = int(L.lib.ic_wino4_3x3_c128_stats_parts(N, H, W))
    raw_o, cst_o = B.out((N, 128, H, W), 'raw y'), B.out((128, parts, 2), 'stats')
    B.done(L.lib.ic_wino4_3x3_c128_raw_stats_f32(L.ptr(xd), L.ptr(wp), L.ptr(raw_o), L.ptr(cst_o), N, H, W, 0, st), 'raw stats')
    raw, cst = B.fin(raw_o, 'raw y (input)'), B.fin(cst_o, 'stats (input)')
    gamma, beta, res = B.fin(d['scale'], 'gamma'), B.fin(d['shift'], 'beta'), B.fin(d['r1'], 'res1')

    def bn(fused):
        mm, mv = B.fin(np.full(128, 0.25, np.float32), 'moving mean'), B.fin(np.full(128, 1.5, np.float32), 'moving variance')
        o = [B.out((128,), n) for n in ('mean', 'invstd', 'scale', 'shift')]
        y = B.out((N, 128, H, W), 'y')
        if fused:
            B.done(L.lib.ic_bn_train_forward_cstats_f32(L.ptr(raw), L.ptr(cst), parts, L.ptr(gamma), L.ptr(beta), L.ptr(mm), L.ptr(mv), 0.9, 1e-5,
                                                        L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]), L.ptr(o[3]), L.ptr(res), None, L.ptr(y), N, 128, H * W, 1, st),
                   'cstats forward')
        else:
            ws = B.ws(L.lib.ic_bn_workspace_bytes(128))
            poison(ws, 0xFF)
            B.done(L.lib.ic_bn_train_forward_f32(L.ptr(raw), L.ptr(gamma), L.ptr(beta), L.ptr(mm), L.ptr(mv), 0.9, 1e-5, L.ptr(o[0]), L.ptr(o[1]),
                                                 L.ptr(o[2]), L.ptr(o[3]), L.ptr(res), None, L.ptr(y), N, 128, H * W, 1, L.ptr(ws), st), 'forward')
        return [y, mm, mv] + o
    a_, b_ = bn(True), bn(False)
    for name, u, v in zip(('y', 'moving mean', 'moving variance', 'mean', 'invstd', 'scale', 'shift'), a_, b_):
        _close(u, v.double(), 'BatchNorm from the conv epilogue sums: ' + name, 2e-6)


# ---- losses and metrics -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', [(1, 3, 33, 47), (1, 2, 17, 19)], ids=lambda s: 'x'.join(map(str, s)))
def test_msssim_loss_and_gradient(cuda, shape):
    """ic_msssim_plan_fill + ic_msssim_loss_grad_f32 as test_hip_ms_ssim_distortion_value_and_gradient checks them (the oracle's float64
    MS-SSIM under autograd: 1e-5 on the value, 2e-4 of max|ref| on the gradient); the plan is uploaded into a fenced input"""
    from imgcomp_cvpr_amd import config_parser as cp, weights as W
    from oracle import train_oracle as T
    L, B = _L(), Bufs(cuda)
    lib, st = L.lib, L.current_stream()
    N, C, H, Wd = shape
    ae, _ = cp.parse(cp.builtin_config_path('ae_configs', 'cvpr', 'med'))
    K = float(ae.K_ms_ssim)
    rs = np.random.RandomState(H)
    a = (W.synthetic_image((N, 3, H, Wd), 'natural', 1)[:, :C]).astype(np.float64)
    b = np.clip(a + rs.normal(0, 9, a.shape), 0, 255)
    tb = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    ref = K * (1.0 - T.ms_ssim(torch.as_tensor(a).double(), tb))
    ref.backward()
    ref = ref.detach()
    nb = int(lib.ic_msssim_plan_bytes(H, Wd))
    assert nb > 0
    host = torch.zeros(nb, dtype=torch.uint8)
    assert lib.ic_msssim_plan_fill(H, Wd, host.data_ptr(), nb) == IC_OK
    plan = B.fin(host, 'plan', torch.uint8)
    xd, xo = B.fin(a, 'x'), B.fin(b, 'x_out')
    need = int(lib.ic_msssim_workspace_bytes(N, C, H, Wd))
    assert need > 0
    ws = B.ws(need)
    grad, scal = B.out((N, C, H, Wd), 'grad'), B.out((16,), 'scalars')

    def launch(grad_, nbytes):
        return lib.ic_msssim_loss_grad_f32(L.ptr(xd), L.ptr(xo), N, C, H, Wd, K, L.ptr(plan), L.ptr(grad_), L.ptr(scal), L.ptr(ws), nbytes, st)
    run = _Poisoned(B, ws, [grad, scal], lambda: launch(grad, need), 'msssim')
    used = list(range(0, 7)) + list(range(8, 13))
    _written(scal[used], 'scalars')
    assert abs(float(scal[0]) - (1.0 - float(ref) / K)) < 1e-5
    assert abs(float(scal[1]) - float(ref)) < 1e-5 * K
    _close(grad, tb.grad, 'MS-SSIM distortion gradient {}x{}'.format(H, Wd), 2e-4)
    run.again()
    _one_byte_short(B, lambda: launch(grad, need - 1), 'msssim')
    value = scal.clone()
    _refill(scal)
    B.done(launch(None, need), 'msssim, value only')
    assert same_bits(scal[:7], value[:7])


def _u8_pair(shape, seed):
    from imgcomp_cvpr_amd import weights as W
    N, C, H, Wd = shape
    a = W.synthetic_image((N, 3, H, Wd), 'natural', seed)[:, :C]
    a = np.ascontiguousarray(np.clip(a, 0, 255).astype(np.uint8))
    b = np.clip(a.astype(np.float64) + np.random.RandomState(seed).normal(0, 7, a.shape), 0, 255).astype(np.uint8)
    return a, b


@pytest.mark.parametrize('shape,per_image', [((1, 3, 40, 200), False), ((2, 3, 96, 200), False), ((1, 1, 17, 23), False), ((3, 3, 33, 40), True)],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else ('per_image' if v else 'batch'))
def test_val_metrics(cuda, shape, per_image):
    """ic_val_metrics_u8_f64 / ic_val_metrics_per_image_u8_f64 against the tap-by-tap float64 twin on the CPU within 1e-12
    (test_device_metrics_match_numpy).  uint8 inputs cannot hold a NaN: fences of 0x00 and of 0xFF, the same bits."""
    from imgcomp_cvpr_amd import metrics
    L, B = _L(), Bufs(cuda)
    lib, st = L.lib, L.current_stream()
    N, C, H, Wd = shape
    a, b = _u8_pair(shape, 3)
    ad, bd = B.fin(a, 'x', torch.uint8, ZERO_FENCE), B.fin(b, 'y', torch.uint8, ZERO_FENCE)
    need = int(lib.ic_val_metrics_workspace_bytes(1 if per_image else N, C, H, Wd))
    assert need > 0
    ws = B.ws(need)
    out = B.out((N, 6) if per_image else (6,), 'out6', torch.float64)
    entry = (lambda *a: lib.ic_val_metrics_per_image_u8_f64(*a)) if per_image else (lambda *a: lib.ic_val_metrics_u8_f64(*a))
    launch = lambda nbytes: entry(L.ptr(ad), L.ptr(bd), N, C, H, Wd, L.ptr(out), L.ptr(ws), nbytes, st)
    got = []
    for fill in (ZERO_FENCE, IN_FENCE):
        F.refence(ad, fill)
        F.refence(bd, fill)
        run = _Poisoned(B, ws, [out], lambda: launch(need), 'val metrics')
        if not got:
            _written(out, 'out6')
            rows = [(out[i], a[i:i + 1], b[i:i + 1]) for i in range(N)] if per_image else [(out, a, b)]
            for o, ai, bi in rows:
                twin = metrics.msssim_scale_values_device(torch.as_tensor(ai), torch.as_tensor(bi))
                assert float((o[:5].cpu() - twin).abs().max()) < 1e-12, (o.cpu(), twin)
                assert float(o[5]) == float(metrics.mse_uint8_device(torch.as_tensor(ai), torch.as_tensor(bi)))
        got.append(run.again()[0])
    assert same_bits(got[0], got[1]), 'the metrics depend on the bytes next to the images'
    _one_byte_short(B, lambda: launch(need - 1), 'val metrics')


# ---- the whole network ----------------------------------------------------------------------------------------------------------------

def _ae_tables(B, L, wts, ae_cfg):
    """what autoencoder._CVPR._prepare builds -- packed filters, folded BatchNorm, the encoder's centres -- with every tensor fenced
    (each packer writes into a fenced output first) -> (encoder tensors, decoder tensors)"""
    from imgcomp_cvpr_amd import autoencoder as A, weights as W
    lib = L.lib
    C, Bk = int(ae_cfg.num_chan_bn), int(ae_cfg.arch_param_B)
    enc, dec = [], []
    for scope, kind, shape in W.ae_conv_specs(C, Bk, bool(ae_cfg.heatmap)):
        w = wts[scope + '/weights']
        scale, shift = A.fold_batch_norm(*(wts[scope + '/BatchNorm/' + k] for k in ('gamma', 'beta', 'moving_mean', 'moving_variance')))
        kh, kw, a_, b_ = shape
        cin, cout = (a_, b_) if kind == 'conv' else (b_, a_)
        stride = 1 if (kh, kw) == (3, 3) and kind == 'conv' else 2
        tr = int(kind == 'deconv')
        n_mfma = lib.ic_conv2d_mfma_packed_floats(kh, kw, cin, cout, stride, tr)
        if kind == 'conv' and tuple(shape) == (3, 3, 128, 128):
            w_use = _pack(B, L, (lambda *a: lib.ic_pack_conv3x3_c128_both_f32(*a)), w, lib.ic_conv3x3_c128_both_packed_floats(), 0)
        elif scope.endswith(('/h2', '/h12')):
            w_use = _pack(B, L, lib.ic_pack_conv5s2_both_f32, w, lib.ic_conv5s2_both_packed_floats(tr), tr)
        elif n_mfma and not scope.endswith('/h1'):
            w_use = _pack(B, L, lib.ic_pack_conv2d_mfma_f32, w, n_mfma, kh, kw, cin, cout, stride, tr)
        else:
            w_use = B.fin(w, scope + ' filter')
        (enc if scope.startswith(A.SCOPE_AE_ENC) else dec).extend([w_use, B.fin(scale, scope + ' scale'), B.fin(shift, scope + ' shift')])
    enc.append(B.fin(wts[A.SCOPE_AE_ENC + '/centers'], 'centers'))
    return enc, dec


def _net_workspace(B, need, pos):
    """exactly `need` bytes; the sync area from `pos` on is caller-initialised (include/imgcomp_hip.h: ic_ae_sync_pos_bytes -- hand-off
    flags and the time-out word of the persistent stack kernel): zeroed as tests/test_gpu_stack.py prepares it, never poisoned"""
    ws = B.ws(need)
    assert 0 <= pos <= need
    ws[pos:].zero_()
    return ws


@pytest.mark.parametrize('plan', ['default', 'f4_everywhere'])
@pytest.mark.parametrize('H,W', [(64, 96), (40, 56)])
def test_whole_network_entries(cuda, configs, syn_weights, H, W, plan):
    """ic_ae_encode_f32, ic_ae_encode_cap_f32 and ic_ae_decode_f32 on one image with tables of fenced tensors and a workspace of exactly
    ic_ae_workspace_bytes, poisoned in front of ic_ae_sync_pos_bytes: against the oracle at NET_RTOL / HEATMAP_RTOL (tests/test_gpu_network.py)"""
    from imgcomp_cvpr_amd import weights as Wt
    from oracle import oracle as O
    from tests.util import NET_RTOL
    L, B = _L(), Bufs(cuda)
    lib, st = L.lib, L.current_stream()
    ae_cfg, _ = configs
    C, Bk, nl = int(ae_cfg.num_chan_bn), int(ae_cfg.arch_param_B), int(ae_cfg.num_centers)
    flags = L.CONV5_BOTH_PACKED | ((L.CONV3_WINO4 | L.CONV5_WINO4) if plan == 'f4_everywhere' else 0)
    enc_t, dec_t = _ae_tables(B, L, syn_weights, ae_cfg)
    enc_tab, dec_tab = L.ptr_table(enc_t), L.ptr_table(dec_t)
    N, hh, ww = 1, H // 8, W // 8
    x = Wt.synthetic_image((N, 3, H, W), 'natural', seed=9)
    ref = O.encode(torch.as_tensor(x).double(), syn_weights, ae_cfg.as_dict())
    xd = B.fin(x, 'x')
    need, pos = lib.ic_ae_workspace_bytes(N, H, W, C), lib.ic_ae_sync_pos_bytes(N, H, W, C)
    ws = _net_workspace(B, need, pos)
    outs = [B.out((N, C, hh, ww), n) for n in ('heatmap', 'z', 'qsoft', 'qhard', 'qbar')] + [B.out((N, C, hh, ww), 'symbols', torch.int64)]
    norm = int(ae_cfg.normalization == 'FIXED')

    def encode(nbytes):
        return lib.ic_ae_encode_f32(L.ptr(xd), enc_tab, Bk, C, nl, 1, norm, *[L.ptr(t) for t in outs], N, H, W, L.ptr(ws), nbytes, flags, st)
    run = _Poisoned(B, ws, outs, lambda: encode(need), 'encode', keep_from=pos)
    hm, z, qs, qh, qb, sym = outs
    _close(z, ref.z, 'network z {}x{} {}'.format(H, W, plan), NET_RTOL)
    _close(hm, ref.heatmap, 'network heatmap {}x{} {}'.format(H, W, plan), HEATMAP_RTOL)
    _written(qs, 'qsoft')
    _, rh, rsym = O.quantize(z.cpu(), syn_weights['autoencoder/encoder/centers'], 1.0)
    assert torch.equal(sym.cpu(), rsym) and torch.equal(qh.cpu(), rh), 'symbols / qhard not exact given the same z'
    assert torch.equal(qb, qs + (qh - qs))
    got = run.again()
    _one_byte_short(B, lambda: encode(need - 1), 'encode')
    # the capped entry with a cap that bounds nothing and the bottleneck copied out: the bits of ic_ae_encode_f32
    cap = B.fin(np.full((N, hh, ww), np.inf, np.float32), 'cap')
    bott = B.out((N, C + 1, hh, ww), 'bottleneck')
    _refill(*outs)

    def encode_cap(nbytes):
        return lib.ic_ae_encode_cap_f32(L.ptr(xd), enc_tab, Bk, C, nl, 1, norm, *[L.ptr(t) for t in outs], N, H, W, L.ptr(ws), nbytes, flags, st,
                                        L.ptr(cap), L.ptr(bott))
    B.done(encode_cap(need), 'encode cap')
    for t, g in zip(outs, got):
        assert same_bits(t, g), 'ic_ae_encode_cap_f32 with cap = +inf: other bits in ' + t._fence[3]
    _written(bott, 'bottleneck')
    assert_close(torch.as_tensor(O.heatmap3d(bott.double().cpu())), ref.heatmap, 'fenced network heatmap from the bottleneck copy', HEATMAP_RTOL)
    _one_byte_short(B, lambda: encode_cap(need - 1), 'encode cap')
    # ---- decode
    q = ref.qhard.float().numpy()
    qd = B.fin(q, 'q')
    x_out = B.out((N, 3, H, W), 'x_out')

    def decode(nbytes):
        return lib.ic_ae_decode_f32(L.ptr(qd), dec_tab, Bk, C, norm, L.ptr(x_out), N, H, W, L.ptr(ws), nbytes, flags, st)
    run = _Poisoned(B, ws, [x_out], lambda: decode(need), 'decode', keep_from=pos)
    _close(x_out, O.decode(ref.qhard, syn_weights, ae_cfg.as_dict()), 'network x_out {}x{} {}'.format(H, W, plan), NET_RTOL)
    run.again()
    _one_byte_short(B, lambda: decode(need - 1), 'decode')


@pytest.mark.parametrize('flags_name', ['default', 'CONV3_WINO4'])
@pytest.mark.parametrize('H,W', [(8, 12), (5, 7)])
def test_residual_stack_entry(cuda, H, W, flags_name):
    """ic_ae_res_stack_f32 (B = 2: 14 layers) on the 128-channel maps of the two images above (8 x 12; 5 x 7, where F(4x4) does not fit and
    the library falls to F(2x2)) against the float64 restatement of tests/test_gpu_stack.py at 2e-5"""
    import torch.nn.functional as TF
    L, B = _L(), Bufs(cuda)
    lib, st = L.lib, L.current_stream()
    flags = 0 if flags_name == 'default' else getattr(L, flags_name)
    Bk, N = 2, 1
    g = torch.Generator(device='cpu').manual_seed(11 + H)
    tens, raw = [], []
    for i in range(6 * Bk + 2):
        w = (torch.randn((3, 3, 128, 128), generator=g) * 0.03).numpy()
        sc, sh = (torch.rand(128, generator=g) * 0.6 + 0.5).numpy(), (torch.randn(128, generator=g) * 0.1).numpy()
        tens += [_pack(B, L, (lambda *a: lib.ic_pack_conv3x3_c128_both_f32(*a)), w, lib.ic_conv3x3_c128_both_packed_floats(), 0), B.fin(sc, 'scale'), B.fin(sh, 'shift')]
        raw.append((torch.as_tensor(w), torch.as_tensor(sc), torch.as_tensor(sh)))
    x = torch.relu(torch.randn((N, 128, H, W), generator=torch.Generator().manual_seed(1)))
    xd = B.fin(x, 'x')
    y = B.out((N, 128, H, W), 'y')
    need, pos = lib.ic_ae_res_stack_workspace_bytes(N, H, W), lib.ic_ae_res_stack_sync_pos_bytes(N, H, W)
    ws = _net_workspace(B, need, pos)
    tab = L.ptr_table(tens)

    def launch(nbytes):
        return lib.ic_ae_res_stack_f32(L.ptr(xd), tab, Bk, L.ptr(y), N, H, W, L.ptr(ws), nbytes, flags, st)
    run = _Poisoned(B, ws, [y], lambda: launch(need), 'residual stack', keep_from=pos)
    assert int(ws[pos:pos + 4].view(torch.int32).item()) == 0          # the time-out word

    def cba(t, i, relu):
        w, sc, sh = raw[i]
        o = TF.conv2d(t, w.double().permute(3, 2, 0, 1), padding=1) * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]
        return torch.relu(o) if relu else o
    net = res0 = x.double()
    li = 0
    for b in range(Bk):
        res_b = net
        for i in range(3):
            t = cba(net, li, True)
            net = cba(t, li + 1, False) + net + (res_b if i == 2 else 0)
            li += 2
    t = cba(net, li, False)
    _close(y, cba(t, li + 1, False) + net + res0, 'residual stack {}x{} {}'.format(H, W, flags_name), 2e-5)
    run.again()
    _one_byte_short(B, lambda: launch(need - 1), 'residual stack')
