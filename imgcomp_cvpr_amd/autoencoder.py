"""Convolutional autoencoder plugin -- MI355X mirror of the reference's code/autoencoder.py.

Same plugin surface (reference code/autoencoder.py:26-29, :33-86, :214-216):

    cls = get_network_cls(ae_config)            # keyed by config.arch ('CVPR')
    ae = cls(ae_config)
    enc = ae.encode(x, is_training=False)       # EncoderOutput(qbar, qhard, symbols, z, heatmap)
    x_out = ae.decode(enc.qhard, is_training=False)
    ae.get_centers_variable(); ae.get_subsampling_factor(); ae.encoder_variables(); ...

but on torch tensors that live on a HIP device, with every op executed by libimgcomp_hip.so
(hand-written gfx950 kernels behind the C ABI of include/imgcomp_hip.h).  TF's implicit variable
store is replaced by an explicit ``load_weights(dict)`` (names/layouts = the reference's checkpoint
variables).  There is no CPU path: tensors on the CPU raise.
"""
from collections import namedtuple, OrderedDict

import numpy as np
import torch

from . import _lib
from . import quantizer
from . import weights as _weights
from ._lib import lib, check, ptr

# reference: code/autoencoder.py:15,18
EncoderOutput = namedtuple('EncoderOutput', ['qbar', 'qhard', 'symbols', 'z', 'heatmap'])
_QuantizerOutput = namedtuple('_QuantizerOutput', ['qbar', 'qsoft', 'qhard', 'symbols'])

SCOPE_AE = 'autoencoder'
SCOPE_AE_ENC = SCOPE_AE + '/encoder'
SCOPE_AE_DEC = SCOPE_AE + '/decoder'

BN_EPSILON = 1e-5      # reference: code/autoencoder.py:118
BN_DECAY = 0.9         # reference: code/autoencoder.py:117
arch_param_n = 128     # reference: code/autoencoder.py:211


def get_network_cls(config):
    """reference: code/autoencoder.py:26-29."""
    return {
        'CVPR': _CVPR,
    }[config.arch]


def fold_batch_norm(gamma, beta, moving_mean, moving_variance, eps=BN_EPSILON):
    """Inference BatchNorm as y = x * scale + shift (float64 math, rounded once to fp32)."""
    g, b, m, v = (np.asarray(a, np.float64) for a in (gamma, beta, moving_mean, moving_variance))
    scale = g / np.sqrt(v + eps)
    shift = b - m * scale
    return scale.astype(np.float32), shift.astype(np.float32)


class _Network(object):
    def __init__(self, config, quantize=True):
        self.config = config
        self.quantize = quantize
        self.num_chan_bn_including_heatmap = config.num_chan_bn + 1
        self._train_graph = None   # training.TrainGraph.bind(): is_training=True calls run that graph's training-mode forward
        self._graph_version = -1
        self.plan_flags = 0        # IC_CONV3_* bits OR-ed into every call of THIS object (tests force a kernel form with it)
        self._centers = None       # set by load_weights(); access with get_centers_variable()
        self._params = None        # OrderedDict name -> device tensor (reference layouts)
        self._device = None

    # -- plugin surface -----------------------------------------------------------------------

    @staticmethod
    def get_subsampling_factor():
        raise NotImplementedError()

    def encode(self, x, is_training, plan_flags=0):
        """x: (N,3,H,W) float32 in 0..255 on the HIP device.  -> EncoderOutput.
        plan_flags (not in the reference): per-call IC_CONV3_* launch-plan bits for the 3x3 layers, see _lib.CONV3_*."""
        assert x.dtype == torch.float32, 'Expected float32 for x, got {}'.format(x.dtype)
        if is_training:
            return self._training_graph().plugin_encode(x)
        self._sync_with_training_graph()
        self._require_weights()
        return self._encode(x, is_training, int(plan_flags) | int(self.plan_flags))

    def decode(self, q, is_training, plan_flags=0):
        if is_training:
            return self._training_graph().plugin_decode(q)
        self._sync_with_training_graph()
        self._require_weights()
        return self._decode(q, is_training, int(plan_flags) | int(self.plan_flags))

    def _training_graph(self):
        if self._train_graph is None:
            raise ValueError('is_training=True needs the training graph that owns the variables and the backward: '
                             'training.TrainGraph(ae_config, pc_config, weights).bind(ae, pc) (see train.py)')
        return self._train_graph

    def _sync_with_training_graph(self):
        """test-in-train (train.py:115-127): is_training=False on a bound object evaluates the CURRENT training variables --
        moving averages folded into the convs, filters re-packed -- whenever an optimiser step has changed them"""
        g = self._train_graph
        if g is not None and self._graph_version != g.version:
            self.load_weights(OrderedDict((n, t.detach().cpu().numpy()) for n, t in g.params.items()), g.dev)
            self._graph_version = g.version

    def get_centers_variable(self):
        if self._train_graph is not None:
            return self._train_graph.params[SCOPE_AE_ENC + '/centers']          # the live training variable
        if self._centers is None:
            raise ValueError('Call load_weights(...) before trying to access centers')
        return self._centers

    def encoder_variables(self):
        """Trainable encoder variables, centres included (reference :70-73)."""
        return self._trainable(SCOPE_AE_ENC)

    def decoder_variables(self):
        return self._trainable(SCOPE_AE_DEC)

    def encoder_regularization_loss(self):
        """factor * l2_loss(conv weights) + centres term (reference :79-82, quantizer.py:18-24)."""
        return self._reg_loss(SCOPE_AE_ENC)

    def decoder_regularization_loss(self):
        return self._reg_loss(SCOPE_AE_DEC)

    # -- weights ------------------------------------------------------------------------------

    def load_weights(self, weights, device='cuda'):
        """weights: dict name -> array in the reference's TF layouts (checkpoint variable names)."""
        device = torch.device(device)
        if device.type != 'cuda':
            raise _lib.HipLibraryError('the autoencoder runs only on a HIP device, got {}'.format(device))
        self._device = device
        self._params = OrderedDict()
        for name, arr in weights.items():
            if name.startswith(SCOPE_AE + '/'):
                self._params[name] = torch.as_tensor(np.ascontiguousarray(arr), dtype=torch.float32).to(device)
        self._centers = self._params[SCOPE_AE_ENC + '/centers']
        self._prepare(weights)
        return self

    def init_weights(self, pc_config=None, seed=1234, device='cuda'):
        raise NotImplementedError('use weights.synthetic_weights(ae_config, pc_config) + load_weights')

    def _require_weights(self):
        if self._params is None:
            raise ValueError('no weights: call load_weights(dict) first (replaces TF variable init / Saver.restore)')

    def _trainable(self, scope):
        self._require_weights()
        return [t for n, t in self._params.items()
                if n.startswith(scope + '/') and 'moving_' not in n]

    def _reg_loss(self, scope):
        """value of the L2 terms of a scope.  On an object bound to a training graph the live variables are read; their
        gradients do not come from this value (they are folded into the filter-gradient kernels, training.py)."""
        if self._train_graph is None:
            self._require_weights()
        params = self._train_graph.params if self._train_graph is not None else self._params
        device = self._train_graph.dev if self._train_graph is not None else self._device
        centers = params[SCOPE_AE_ENC + '/centers']
        total = torch.zeros((), dtype=torch.float32, device=device)
        f = float(self.config.regularization_factor)
        for n, t in params.items():
            if n.startswith(scope + '/') and n.endswith('/weights'):
                total = total + f * 0.5 * (t * t).sum()
        if scope == SCOPE_AE_ENC and self.config.regularization_factor_centers != 0:
            total = total + quantizer.create_centers_regularization_term(self.config, centers)
        return total.detach()

    def _prepare(self, weights):
        raise NotImplementedError()

    def _encode(self, x, is_training, plan_flags=0):
        raise NotImplementedError()

    def _decode(self, q, is_training, plan_flags=0):
        raise NotImplementedError()


class _CVPR(_Network):
    """reference: code/autoencoder.py:214-268."""

    @staticmethod
    def get_subsampling_factor():
        return 8

    # -- device-side plan: packed filters, folded BN, pointer tables -------------------------------

    def _prepare(self, weights):
        cfg = self.config
        self._B = int(cfg.arch_param_B)
        self._C = int(cfg.num_chan_bn)
        self._L = int(cfg.num_centers)
        dev = self._device
        st = _lib.current_stream(dev)
        specs = _weights.ae_conv_specs(self._C, self._B, bool(cfg.heatmap))
        self._plan = {}           # scope -> (w_dev, scale_dev, shift_dev); keeps tensors alive
        self._edge_both = False
        enc_tab, dec_tab = [], []
        packed_n = lib.ic_conv3x3_c128_both_packed_floats()
        for scope, kind, shape in specs:
            w = self._params[scope + '/weights']
            scale, shift = fold_batch_norm(*(weights[scope + '/BatchNorm/' + k] for k in
                                             ('gamma', 'beta', 'moving_mean', 'moving_variance')))
            scale_d = torch.from_numpy(scale).to(dev)
            shift_d = torch.from_numpy(shift).to(dev)
            kh, kw, a_, b_ = shape
            cin, cout = (a_, b_) if kind == 'conv' else (b_, a_)
            stride = 1 if (kh, kw) == (3, 3) and kind == 'conv' else 2
            n_mfma = lib.ic_conv2d_mfma_packed_floats(kh, kw, cin, cout, stride, int(kind == 'deconv'))
            if kind == 'conv' and tuple(shape) == (3, 3, arch_param_n, arch_param_n):
                wp = torch.empty(packed_n, dtype=torch.float32, device=dev)
                # direct-form and Winograd fragments side by side; the library picks the form per launch
                check(lib.ic_pack_conv3x3_c128_both_f32(ptr(w), ptr(wp), 0, st), 'ic_pack_conv3x3_c128_both_f32')
                w_use = wp
            elif scope.endswith(('/h2', '/h12')) and (kh, kw, stride) == (5, 5, 2) and {cin, cout} == {64, 128}:
                # h2 / h12: MFMA fragments and the F(4x4)-over-phases fragments in one blob; the library picks per call
                # (IC_CONV5_BOTH_PACKED tells it the blob has both, see _encode / _decode)
                tr = int(kind == 'deconv')
                wp = torch.empty(lib.ic_conv5s2_both_packed_floats(tr), dtype=torch.float32, device=dev)
                check(lib.ic_pack_conv5s2_both_f32(ptr(w), ptr(wp), tr, st), 'ic_pack_conv5s2_both_f32')
                w_use = wp
                self._edge_both = True
            elif n_mfma and not scope.endswith('/h1'):
                # h2, to_bn, h12: matrix-core path, filter in MFMA fragment order
                wp = torch.empty(n_mfma, dtype=torch.float32, device=dev)
                check(lib.ic_pack_conv2d_mfma_f32(ptr(w), ptr(wp), kh, kw, cin, cout, stride, int(kind == 'deconv'), st),
                      'ic_pack_conv2d_mfma_f32')
                w_use = wp
            else:
                w_use = w
            self._plan[scope] = (w_use, scale_d, shift_d)
            (enc_tab if scope.startswith(SCOPE_AE_ENC) else dec_tab).extend([w_use, scale_d, shift_d])
        enc_tab.append(self._centers)
        torch.cuda.synchronize(dev)
        self._enc_tab = _lib.ptr_table(enc_tab)
        self._dec_tab = _lib.ptr_table(dec_tab)
        self._ws = None

    def _abi_flags(self, plan_flags):
        """the caller's per-call plan bits + what this object's filter blobs hold"""
        return int(plan_flags) | (_lib.CONV5_BOTH_PACKED if self._edge_both else 0)

    def sharing_weights(self):
        """a second object of this network over the SAME device weights, packed filters and pointer tables, with its own workspace
        and per-call state -- for a caller that keeps several images in flight, one object per stream (val.py), without uploading
        and packing the weights once per stream."""
        import copy
        other = copy.copy(self)
        other._ws = None
        other._last_qsoft = None
        return other

    def _workspace(self, N, H, W):
        need = lib.ic_ae_workspace_bytes(N, H, W, self._C)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self._device)
        return self._ws, need

    # -- forward -----------------------------------------------------------------------------------

    def _encode(self, x, is_training, plan_flags=0):
        assert not is_training          # (training mode is dispatched to the bound TrainGraph in encode())
        _lib.require_cuda(x, 'x')
        x = x.contiguous()
        N, three, H, W = x.shape
        assert three == 3, 'Expected N3HW, got {}'.format(tuple(x.shape))
        f = self.get_subsampling_factor()
        if H % f or W % f:
            raise ValueError('H and W must be multiples of {} (val.py pads images first), got {}x{}'.format(f, H, W))
        C, hh, ww = self._C, H // f, W // f
        mk = lambda: torch.empty((N, C, hh, ww), dtype=torch.float32, device=x.device)
        heat_on = bool(self.config.heatmap)
        if not self.quantize:
            # autoencoder.py:127-129: no quantiser -- the encoder hands on the (masked) bottleneck itself, _QuantizerOutput(z, None, None, None)
            z = mk()
            heatmap = mk() if heat_on else None
            ws, need = self._workspace(N, H, W)
            check(lib.ic_ae_encode_f32(ptr(x), self._enc_tab, self._B, C, self._L, int(heat_on),
                                       int(self.config.normalization == 'FIXED'), ptr(heatmap), ptr(z), None, None, None, None,
                                       N, H, W, ptr(ws), need, self._abi_flags(plan_flags), _lib.current_stream(x.device)), 'ic_ae_encode_f32')
            return EncoderOutput(z, None, None, z, heatmap)
        z, qsoft, qhard = mk(), mk(), mk()
        qbar = mk() if heat_on else None
        heatmap = mk() if heat_on else None
        symbols = torch.empty((N, C, hh, ww), dtype=torch.int64, device=x.device)
        ws, need = self._workspace(N, H, W)
        check(lib.ic_ae_encode_f32(ptr(x), self._enc_tab, self._B, C, self._L, int(heat_on),
                                   int(self.config.normalization == 'FIXED'),
                                   ptr(heatmap), ptr(z), ptr(qsoft), ptr(qhard), ptr(qbar), ptr(symbols),
                                   N, H, W, ptr(ws), need, self._abi_flags(plan_flags), _lib.current_stream(x.device)), 'ic_ae_encode_f32')
        if qbar is None:
            qbar = qhard      # forward value of qsoft + stop_gradient(qhard - qsoft)
        self._last_qsoft = qsoft
        return EncoderOutput(qbar, qhard, symbols, z, heatmap)

    # -- importance-map cap (not in the reference): an upper bound on heatmap2D per latent position, inference only --------

    def _check_cap(self, cap, shape, device, what='cap'):
        """cap: float32 device tensor of `shape`, 0 <= cap <= +inf -> contiguous; every refusal is a ValueError"""
        if not bool(self.config.heatmap):
            raise ValueError('{}: this config has no importance map (heatmap = False): there is nothing to cap'.format(what))
        if not self.quantize:
            raise ValueError('{}: this network was built with quantize=False'.format(what))
        if not isinstance(cap, torch.Tensor) or cap.dtype != torch.float32 or cap.device != device or tuple(cap.shape) != tuple(shape):
            raise ValueError('{}: expected a float32 tensor of shape {} on {}, got {}'.format(
                what, tuple(shape), device, '{} {} on {}'.format(cap.dtype, tuple(cap.shape), cap.device) if isinstance(cap, torch.Tensor) else type(cap).__name__))
        if not bool((cap >= 0).all()):            # (a NaN compares false)
            raise ValueError('{}: entries must be in [0, +inf], got a negative or NaN entry'.format(what))
        return cap.contiguous()

    def encode_capped(self, x, cap=None, keep_bottleneck=False, plan_flags=0):
        """encode(x, is_training=False) with h2 = min(heatmap2D, cap) in the importance map (ic_ae_encode_cap_f32).
        cap: None, or (N, H/8, W/8) float32 on x's device, 0 <= cap <= +inf; cap >= C everywhere is encode itself, bit for bit.
        -> (EncoderOutput, bottleneck (N, C+1, H/8, W/8) if keep_bottleneck else None): requantize(bottleneck, caps) quantises the
        same image under other caps without running the encoder again."""
        assert x.dtype == torch.float32, 'Expected float32 for x, got {}'.format(x.dtype)
        self._sync_with_training_graph()
        self._require_weights()
        _lib.require_cuda(x, 'x')
        x = x.contiguous()
        N, three, H, W = x.shape
        assert three == 3, 'Expected N3HW, got {}'.format(tuple(x.shape))
        f = self.get_subsampling_factor()
        if H % f or W % f:
            raise ValueError('H and W must be multiples of {} (val.py pads images first), got {}x{}'.format(f, H, W))
        C, hh, ww = self._C, H // f, W // f
        if not bool(self.config.heatmap) or not self.quantize:
            raise ValueError('encode_capped: this config has no importance map (heatmap = False) or no quantiser: use encode')
        if cap is not None:
            cap = self._check_cap(cap, (N, hh, ww), x.device)
        mk = lambda: torch.empty((N, C, hh, ww), dtype=torch.float32, device=x.device)
        z, qsoft, qhard, qbar, heatmap = mk(), mk(), mk(), mk(), mk()
        symbols = torch.empty((N, C, hh, ww), dtype=torch.int64, device=x.device)
        bott = torch.empty((N, C + 1, hh, ww), dtype=torch.float32, device=x.device) if keep_bottleneck else None
        ws, need = self._workspace(N, H, W)
        check(lib.ic_ae_encode_cap_f32(ptr(x), self._enc_tab, self._B, C, self._L, 1, int(self.config.normalization == 'FIXED'),
                                       ptr(heatmap), ptr(z), ptr(qsoft), ptr(qhard), ptr(qbar), ptr(symbols),
                                       N, H, W, ptr(ws), need, self._abi_flags(int(plan_flags) | int(self.plan_flags)),
                                       _lib.current_stream(x.device), ptr(cap), ptr(bott)), 'ic_ae_encode_cap_f32')
        self._last_qsoft = qsoft
        return EncoderOutput(qbar, qhard, symbols, z, heatmap), bott

    def requantize(self, bottleneck, caps, hard_only=False):
        """bottleneck (N, C+1, h, w) of encode_capped(keep_bottleneck=True); caps (N, T, h, w) or (N, h, w) (T = 1), 1 <= T <= 16
        -> EncoderOutput of batch N * T, image n * T + t under caps[n, t]: one launch of ic_heatmap_quantize_cap_f32 that reads the
        bottleneck once for all T.  hard_only: qhard and symbols alone (the rest None), which is all a rate search reads."""
        self._require_weights()
        _lib.require_cuda(bottleneck, 'bottleneck')
        C = self._C
        if bottleneck.dtype != torch.float32 or bottleneck.dim() != 4 or bottleneck.shape[1] != C + 1:
            raise ValueError('bottleneck: expected float32 (N, {}, h, w), got {} {}'.format(C + 1, bottleneck.dtype, tuple(bottleneck.shape)))
        bottleneck = bottleneck.contiguous()
        N, _, hh, ww = bottleneck.shape
        if isinstance(caps, torch.Tensor) and caps.dim() == 3:
            caps = caps[:, None]
        T = int(caps.shape[1]) if isinstance(caps, torch.Tensor) and caps.dim() == 4 else 0
        if isinstance(caps, torch.Tensor) and caps.dim() == 4 and not 1 <= T <= 16:
            raise ValueError('caps: 1 .. 16 levels per launch, got {}'.format(T))
        caps = self._check_cap(caps, (N, max(T, 1), hh, ww), bottleneck.device, 'caps')
        mk = lambda: torch.empty((N * T, C, hh, ww), dtype=torch.float32, device=bottleneck.device)
        qhard = mk()
        z, qsoft, qbar, heatmap = (None,) * 4 if hard_only else (mk(), mk(), mk(), mk())
        symbols = torch.empty((N * T, C, hh, ww), dtype=torch.int64, device=bottleneck.device)
        check(lib.ic_heatmap_quantize_cap_f32(ptr(bottleneck), ptr(caps), T, ptr(self._centers), self._L, 1.0,
                                              ptr(heatmap), ptr(z), ptr(qsoft), ptr(qhard), ptr(qbar), ptr(symbols),
                                              N, C, hh, ww, _lib.current_stream(bottleneck.device)), 'ic_heatmap_quantize_cap_f32')
        return EncoderOutput(qbar, qhard, symbols, z, heatmap)

    # -- the kernel family of one shape, forced on another (host queries only: no device call) ---------------

    PLAN_LIKE_MAX_PIXELS = 1 << 25      # from here on the edge kernels and the 3x3 forms meet their 31-bit offset limits and fall back

    def _decode_family(self, H, W, flags):
        """what decode(q of an (1, 3, H, W) picture) runs under the ABI flags `flags`: (3x3 form of ic_conv3x3_c128_pick_form, its
        F(2x2) decomposition 'whole' | 'ksplit' | 'mixed' or None, h12 on the F(4x4)-over-phases kernel?) -- network.hip's rules"""
        h4, w4 = H // 4, W // 4
        form = int(lib.ic_conv3x3_c128_pick_form(1, h4, w4, flags))
        split = None
        if form == 1:
            import ctypes
            pl = (ctypes.c_longlong * 5)()
            check(lib.ic_wino3x3_c128_plan(1, h4, w4, flags & ~(_lib.CONV3_WINO4_WG8 | _lib.CONV3_WINO4_WG4), pl), 'ic_wino3x3_c128_plan')
            whole, seg, _, t16, ksplit = (int(v) for v in pl)
            # whole-K, its per-wave form, the NB-segment and the 16 x 16 jobs do the same operations per output; K-split sums four
            # partial chains (tests/test_gpu_ops.py: the decompositions bit for bit)
            split = 'whole' if ksplit == 0 else 'ksplit' if whole + seg + t16 == 0 else 'mixed'
        h12_w4 = bool(flags & _lib.CONV5_BOTH_PACKED) and not (flags & _lib.CONV5_NO_WINO4) and \
            int(lib.ic_wino4_conv5s2_supported(1, h4, w4)) == 1 and \
            (bool(flags & _lib.CONV5_WINO4) or form == 2 or int(lib.ic_wino4_conv5s2_workgroups(1, h4, w4, 0)) >= 160)
        return form, split, h12_w4

    def decode_family(self, H, W):
        """_decode_family of an (1, 3, H, W) picture under this object's own plan_flags"""
        return self._decode_family(int(H), int(W), self._abi_flags(self.plan_flags))

    def plan_like(self, H, W):
        """the IC_CONV3_* / IC_CONV5_* bits that force, on a picture of ANOTHER shape, the kernel family decode gives an (1, 3, H, W)
        picture under this object's own plan_flags: the 3x3 form (direct, F(2x2), F(4x4)) with the F(2x2) decomposition that sums
        alike, and h12's form (F(4x4) over phases or the direct kernel).  Pass them as decode(..., plan_flags=bits) of the other
        picture; plan_holds says whether that picture can take them.  None where flags cannot say it: an F(2x2) plan that mixes
        whole-K and K-split launches, own flags whose form bits the wanted form cannot be OR-ed onto, IC_CONV3_LEAVE_IDLE_CUS
        (per-layer plans), a picture of PLAN_LIKE_MAX_PIXELS or more (the kernels' 31-bit fall-backs)."""
        H, W = int(H), int(W)
        f = self.get_subsampling_factor()
        if H < f or W < f or H % f or W % f:
            raise ValueError('H and W must be positive multiples of {}, got {}x{}'.format(f, H, W))
        flags = self._abi_flags(self.plan_flags)
        if H * W >= self.PLAN_LIKE_MAX_PIXELS or flags & _lib.CONV3_LEAVE_IDLE_CUS:
            return None
        form, split, h12_w4 = self._decode_family(H, W, flags)
        if form == 1 and split == 'mixed':
            return None
        want = {0: _lib.CONV3_DIRECT, 2: _lib.CONV3_WINO4}.get(form, _lib.CONV3_WINO_KSPLIT if split == 'ksplit' else _lib.CONV3_WINO_WHOLEK)
        if (flags & _lib.CONV3_FORM_MASK) | want != want:
            return None
        return want | (_lib.CONV5_WINO4 if h12_w4 else _lib.CONV5_NO_WINO4)

    def plan_holds(self, bits, H, W, Hw, Ww, top=0, left=0):
        """does decode of an (1, 3, Hw, Ww) window with plan_flags=bits (plan_like(H, W)) run the family of the (1, 3, H, W) picture,
        with its F(4x4) tiles where the picture has them?  top, left: the window's origin in the picture, in pixels; an F(4x4) tile
        is 4 x 4 positions at H/4, 16 x 16 pixels."""
        if bits is None or Hw * Ww >= self.PLAN_LIKE_MAX_PIXELS:
            return False
        flags = self._abi_flags(self.plan_flags)
        full, here = self._decode_family(int(H), int(W), flags), self._decode_family(int(Hw), int(Ww), flags | int(bits))
        if full != here:
            return False
        return not (full[0] == 2 or full[2]) or (int(top) % 16 == 0 and int(left) % 16 == 0)

    def _decode(self, q, is_training, plan_flags=0):
        assert not is_training
        _lib.require_cuda(q, 'q')
        q = q.contiguous()
        N, C, hh, ww = q.shape
        assert C == self._C, 'Expected {} bottleneck channels, got {}'.format(self._C, C)
        f = self.get_subsampling_factor()
        H, W = hh * f, ww * f
        x_out = torch.empty((N, 3, H, W), dtype=torch.float32, device=q.device)
        ws, need = self._workspace(N, H, W)
        check(lib.ic_ae_decode_f32(ptr(q), self._dec_tab, self._B, C, int(self.config.normalization == 'FIXED'),
                                   ptr(x_out), N, H, W, ptr(ws), need, self._abi_flags(plan_flags), _lib.current_stream(q.device)),
              'ic_ae_decode_f32')
        return x_out
