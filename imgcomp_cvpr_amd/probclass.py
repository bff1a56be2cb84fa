"""Context-model ("probability classifier") plugin -- mirror of the reference's code/probclass.py.

    cls = get_network_cls(pc_config)                 # keyed by pc_config.arch ('res_shallow')
    pc = cls(pc_config, num_centers=L)
    bits = pc.bitcost(q, target_symbols, is_training=False, pad_value=pc.auto_pad_value(ae))   # NCHW
    logits = pc.logits(q_padded, is_training=False)                                            # N,C,h,w,L

All positions are evaluated in parallel by libimgcomp_hip.so (csrc/probclass.hip); the volume is
padded on load, never materialised.  Weights come from ``load_weights(dict)`` in the reference's
variable names/layouts (unmasked conv3d filters [2,3,3,cin,cout] + biases).
"""
import ctypes
import itertools
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import _lib
from . import weights as _weights
from ._lib import lib, check, ptr


def get_network_cls(pc_config):
    """reference: code/probclass.py:11-15."""
    return {
        'res_shallow': _ResShallow,
    }[pc_config.arch]


def context_shape_from_context_size(context_size):
    """:return context shape as DHW (reference code/probclass.py:18-20)."""
    return context_size // 2 + 1, context_size, context_size


def context_size_from_context_shape(context_shape):
    return context_shape[-1]


class _Network3D(object):
    _PROBCLASS_SCOPE = 'probclass3d'

    def __init__(self, pc_config, num_centers):
        self.config = pc_config
        self.L = int(num_centers)
        self._params = None
        self._device = None
        self._ws = None
        self._last_logits = None
        self._train_graph = None      # training.TrainGraph.bind()
        self._graph_version = -1

    # -- static geometry (reference :40-57) --

    @classmethod
    def get_num_layers(cls):
        raise NotImplementedError()

    @classmethod
    def get_context_size(cls, config):
        """width / height of the receptive field."""
        return cls.get_num_layers() * (config.kernel_size - 1) + 1

    @classmethod
    def get_context_shape(cls, config):
        """Shape as DHW."""
        return context_shape_from_context_size(cls.get_context_size(config))

    @property
    def filter_shape(self):
        K = self.config.kernel_size
        return K // 2 + 1, K, K

    def auto_pad_value(self, ae):
        """0, or centers[0] when use_centers_for_padding (reference :59-61)."""
        return 0 if not self.config.use_centers_for_padding else ae.get_centers_variable()[0]

    # -- masks, as numpy (reference :150-176); the kernels skip the zeroed taps --

    def create_first_mask(self):
        K = self.config.kernel_size
        mask = np.ones(self.filter_shape, dtype=np.float32)
        mask[-1, K // 2, K // 2:] = 0
        mask[-1, K // 2 + 1:, :] = 0
        return mask[..., None, None]

    def create_other_mask(self):
        K = self.config.kernel_size
        mask = np.ones(self.filter_shape, dtype=np.float32)
        mask[-1, K // 2, K // 2 + 1:] = 0
        mask[-1, K // 2 + 1:, :] = 0
        return mask[..., None, None]

    # -- weights --

    def load_weights(self, weights, device='cuda'):
        device = torch.device(device)
        if device.type != 'cuda':
            raise _lib.HipLibraryError('the context model runs only on a HIP device, got {}'.format(device))
        self._device = device
        self._params = OrderedDict()
        for name, arr in weights.items():
            if name.startswith(self._PROBCLASS_SCOPE + '/'):
                self._params[name] = torch.as_tensor(np.ascontiguousarray(arr), dtype=torch.float32).to(device)
        self._prepare()
        return self

    def variables(self):
        self._require_weights()
        return list(self._params.values())

    def get_network_variables(self):
        return self.variables()

    def regularization_loss(self):
        """None unless config.regularization_factor is set (reference :115-119)."""
        if self.config.regularization_factor is None:
            return None
        if self._train_graph is not None:
            params = {n: t for n, t in self._train_graph.params.items() if n.startswith(self._PROBCLASS_SCOPE + '/')}
        else:
            self._require_weights()
            params = self._params
        f = float(self.config.regularization_factor)
        return (f * sum(0.5 * (t * t).sum() for n, t in params.items() if n.endswith('/weights'))).detach()

    def _require_weights(self):
        if self._params is None:
            raise ValueError('no weights: call load_weights(dict) first')

    def _prepare(self):
        raise NotImplementedError()

    # -- forward --

    def _pad_value_as_float(self, pad_value):
        """The C ABI takes the pad value by value.  A tensor (centers[0], reference probclass.py:59-61) is fetched from the
        device once per distinct VALUE SOURCE: a .item() per image would stall the host until everything queued on the
        stream -- the whole encoder -- has finished, before the decoder could be enqueued.
          * bound to a training graph (test-in-train, train.py:122-126): the optimiser updates the centres through a raw
            pointer, which neither moves the storage nor bumps torch's version counter, so the cache key is the graph's
            own `version` (bumped by every apply_gradients) and the value is the graph's pinned copy of centres[0];
          * unbound: keyed on the identity of the tensor that OWNS the storage (a weak reference: a fresh centres tensor at
            a recycled address is a different owner) plus its version counter."""
        if not torch.is_tensor(pad_value):
            return float(pad_value)
        g = self._train_graph
        if g is not None:
            key = ('graph', id(g), g.version)
            if getattr(self, '_pad_cache', (None, None))[0] != key:
                self._pad_cache = (key, float(g._pad_value()))
            return self._pad_cache[1]
        owner = pad_value._base if pad_value._base is not None else pad_value
        cached = getattr(self, '_pad_cache', None)
        if (cached is not None and cached[0][0] == 'tensor' and cached[0][1]() is owner
                and cached[0][2:] == (pad_value.data_ptr(), owner._version)):
            return cached[1]
        import weakref
        self._pad_cache = (('tensor', weakref.ref(owner), pad_value.data_ptr(), owner._version), float(pad_value.item()))
        return self._pad_cache[1]

    def bitcost(self, q, target_symbols, is_training, pad_value=0):
        """q: NCHW float32, target_symbols: NCHW int64 -> bit cost per symbol, NCHW
        (reference code/probclass.py:63-106)."""
        raise NotImplementedError()

    def logits(self, q, is_training):
        """q: ALREADY padded volume (N,D,H,W) [the reference passes N,D,H,W,1] -> (N,D-4,H-8,W-8,L)
        (reference code/probclass.py:130-135)."""
        raise NotImplementedError()


class _ResShallow(_Network3D):
    """conv0 -> residual(conv1, conv2) -> conv2(final), reference code/probclass.py:199-221."""
    _NUM_RESIDUAL = 1

    @classmethod
    def get_num_layers(cls):
        return 2 + _ResShallow._NUM_RESIDUAL * 2

    def _prepare(self):
        if self.config.kernel_size != 3:
            raise NotImplementedError('the HIP context model implements kernel_size = 3 (res_shallow configs)')
        if self.config.learn_pad_var:
            raise NotImplementedError('learn_pad_var=True is dead code in the reference configs')
        self._k = int(self.config.arch_param__k)
        tabs = []
        for scope, shape in _weights.pc_conv_specs(self.L, self._k, int(self.config.kernel_size)):
            w, b = self._params[scope + '/weights'], self._params[scope + '/biases']
            assert tuple(w.shape) == tuple(shape), (scope, tuple(w.shape), shape)
            tabs += [w, b]
        # the matrix-core layers' filter fragments, packed once: inference runs without a per-call packing launch
        n = lib.ic_pc_packed_floats(self._k, self.L)
        packed = None
        if n:
            packed = torch.empty(n, dtype=torch.float32, device=self._device)
            check(lib.ic_pc_pack_filters_f32(_lib.ptr_table(tabs + [None]), self._k, self.L, ptr(packed), _lib.current_stream(self._device)),
                  'ic_pc_pack_filters_f32')
            torch.cuda.synchronize(self._device)
        self._tab_tensors = tabs + [packed]
        self._tab = _lib.ptr_table(self._tab_tensors)

    def sharing_weights(self):
        """a second object of this network over the SAME device weights and packed filters with its own workspace and caches: one
        per stream for a caller that keeps several images in flight (val.py)."""
        import copy
        other = copy.copy(self)
        other._ws = None
        other._last_logits = None
        if hasattr(other, '_pad_cache'):
            del other._pad_cache
        return other

    def _workspace(self, N, C, h, w):
        need = lib.ic_pc_workspace_bytes(N, C, h, w, self._k)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self._device)
        return self._ws, need

    def _sync_with_training_graph(self):
        g = self._train_graph
        if g is not None and self._graph_version != g.version:
            self.load_weights(OrderedDict((n, t.detach().cpu().numpy()) for n, t in g.params.items()
                                          if n.startswith(self._PROBCLASS_SCOPE + '/')), g.dev)
            self._graph_version = g.version

    def bitcost(self, q, target_symbols, is_training, pad_value=0, return_logits=False):
        if is_training:
            if self._train_graph is None:
                raise ValueError('is_training=True needs the training graph that owns the variables and the backward: '
                                 'training.TrainGraph(ae_config, pc_config, weights).bind(ae, pc) (see train.py)')
            assert not return_logits
            return self._train_graph.plugin_bitcost(q, target_symbols, pad_value)
        self._sync_with_training_graph()
        self._require_weights()
        assert q.dim() == 4, 'Expected NCHW'
        _lib.require_cuda(q, 'q')
        assert target_symbols.dtype == torch.int64 and target_symbols.shape == q.shape
        q = q.contiguous()
        target_symbols = target_symbols.contiguous()
        N, C, h, w = q.shape
        bits = torch.empty_like(q)
        logits = torch.empty((N, C, h, w, self.L), dtype=torch.float32, device=q.device) if return_logits else None
        ws, need = self._workspace(N, C, h, w)
        check(lib.ic_pc_bitcost_f32(ptr(q), ptr(target_symbols), self._tab, self._k, self.L,
                                    self._pad_value_as_float(pad_value), ptr(logits), ptr(bits),
                                    N, C, h, w, ptr(ws), need, _lib.current_stream(q.device)), 'ic_pc_bitcost_f32')
        if return_logits:
            return bits, logits
        return bits

    def logits_unpadded(self, q, pad_value):
        """logits (N,C,h,w,L) for an un-padded q, padding on load with pad_value."""
        self._require_weights()
        _lib.require_cuda(q, 'q')
        q = q.contiguous()
        N, C, h, w = q.shape
        out = torch.empty((N, C, h, w, self.L), dtype=torch.float32, device=q.device)
        ws, need = self._workspace(N, C, h, w)
        check(lib.ic_pc_logits_f32(ptr(q), self._tab, self._k, self.L, self._pad_value_as_float(pad_value),
                                   ptr(out), N, C, h, w, ptr(ws), need, _lib.current_stream(q.device)),
              'ic_pc_logits_f32')
        return out

    def logits(self, q, is_training):
        if is_training:
            raise NotImplementedError('is_training=True: the context model trains inside imgcomp_cvpr_amd.training.TrainGraph '
                                      '(forward with tape + hand-written backward); this plugin method is inference only')
        self._require_weights()
        _lib.require_cuda(q, 'q')
        if q.dim() == 5:
            assert q.shape[-1] == 1, 'Expected NDHW1'
            q = q[..., 0]
        q = q.contiguous()
        N, D, H, W = q.shape
        out = torch.empty((N, D - 4, H - 8, W - 8, self.L), dtype=torch.float32, device=q.device)
        ws, need = self._workspace(N, D - 4, H - 8, W - 8)
        check(lib.ic_pc_logits_padded_f32(ptr(q), self._tab, self._k, self.L, ptr(out), N, D, H, W,
                                          ptr(ws), need, _lib.current_stream(q.device)), 'ic_pc_logits_padded_f32')
        return out


################################################################################
# Helpers for arithmetic coding (val.py --real_bpp), reference code/probclass.py:393-482
################################################################################


class ProbclassNetworkTesting(object):
    """bit cost of a whole symbol volume, fully convolutionally (reference code/probclass.py:393-421)."""

    def __init__(self, pc, ae, sess=None):
        self.pc = pc
        self.centers = ae.get_centers_variable()
        self.pad_value = pc.auto_pad_value(ae)

    def get_total_bit_cost(self, symbols):
        """:param symbols: CHW or NCHW numpy / tensor of all symbols of an image -> total bits (float)."""
        sym = symbols if torch.is_tensor(symbols) else torch.as_tensor(np.asarray(symbols))
        if sym.dim() == 3:
            sym = sym[None]
        assert sym.dim() == 4
        sym = sym.to(self.centers.device).long().contiguous()
        q = self.centers[sym]                                    # tf.gather(centers, symbols)
        bc = self.pc.bitcost(q, sym, is_training=False, pad_value=self.pad_value)
        return float(bc.double().sum())


class PredictionNetwork(object):
    """Frequency tables for the arithmetic coder (reference code/probclass.py:425-482).

    get_pr / get_freqs keep the reference's one-context-at-a-time interface (the decoder needs it: a symbol's
    table depends on the symbols decoded before it).  get_all(...) is the parallel path the README asks for
    (README.md:71): ONE pass of the context model yields the tables of every position, and because the kernels
    evaluate a fixed, position-independent fp32 expression per logit, both paths give bit-identical tables."""

    def __init__(self, pc, config, centers, sess=None, freqs_resolution=1e9):
        self.pc = pc
        self.pc_class = pc.__class__
        self.config = config
        self.centers = centers
        self.input_ctx_shape = self.pc_class.get_context_shape(config)
        self.freqs_resolution = float(freqs_resolution)

    def pad_symbols_volume(self, symbols):
        assert symbols.ndim == 3
        return pad_for_probclass3d(symbols, self.pc_class.get_context_size(self.config))

    def undo_pad_symbols_volume(self, symbols):
        assert symbols.ndim == 3
        return undo_pad_for_probclass3d(symbols, self.pc_class.get_context_size(self.config))

    def _tables(self, vol_padded):
        """vol_padded: (D,H,W) int symbols (already padded) -> (pr, freqs) for every context, raster C,H,W."""
        dev = self.centers.device
        sym = torch.as_tensor(np.ascontiguousarray(vol_padded)).to(dev).long()
        q = self.centers[sym][None].contiguous()                       # gather -> (1,D,H,W) float
        logits = self.pc.logits(q, is_training=False)                  # (1,D-4,H-8,W-8,L)
        n = logits.numel() // self.pc.L
        freqs = torch.empty((n, self.pc.L), dtype=torch.int64, device=dev)
        pr = torch.empty((n, self.pc.L), dtype=torch.float32, device=dev)
        check(lib.ic_pc_logits_to_freqs_f32(ptr(logits), n, self.pc.L, self.freqs_resolution, ptr(freqs), ptr(pr),
                                            _lib.current_stream(dev)), 'ic_pc_logits_to_freqs_f32')
        return pr.cpu().numpy(), freqs.cpu().numpy()

    def get_all(self, symbols_padded):
        """(pr, freqs), each (num_contexts, L), contexts in the order of iter_over_blocks."""
        return self._tables(symbols_padded)

    def encode_stream(self, symbols, capacity=None, order='raster', seg_ends=None, depth_block=None, lanes=None):
        """The mirror of decode_stream: the whole coding side on the device (ic_pc_encode_f32).  symbols: un-padded (C,h,w) numpy /
        tensor -> (stream_bytes, first_sym); a batch (N,C,h,w) -> a list of N such pairs, coded concurrently by ONE launch.
        The tables are bit for bit those of get_all(pad_symbols_volume(symbols)) -- the symbol volume padded with symbol 0, the
        centres gathered, pc.logits on the padded volume, as _tables does -- but they never exist in memory: the kernel takes
        (cum_lo, cum_hi, total) of each symbol from a table row held in registers, and only the stream comes back to the host.
        capacity: bytes reserved per stream (tests); default ic_pc_encode_capacity_bytes, which always suffices.
        order='wavefront': the same tables and symbols, coded in the order of codec.wavefront_order(C, h, w) -- logits and symbols
        are gathered through the permutation on the device, the kernel codes what it is given; the first symbol is the same.
        seg_ends=[n_0 < n_1 < ... = C h w] (raster only; ic_pc_encode_segments_f32): the volume's symbols cut at these cumulative counts
        into independent coder runs, one work-group each -- run s is arithmetic_coding.encode_sequence(flat[a:b], freqs[a:b]) with
        a = max(1, n_{s-1}), b = n_s, over the same tables.  -> ([segment bytes ...], first_sym) per volume; capacity is per segment.
        depth_block=B (order='wavefront' only, container format 10): the stream is codec.depth_plane(symbols, fill, B) as bytes, then
        the coder's bytes over the LIVE positions of the wavefront order alone (codec.depth_live_mask): the plane and the mask are a
        few tensor operations on the device, the dead positions go to the same launch as IC_PC_ENCODE_SKIP and are stepped over.  The
        tables are those of the whole volume, as ever.  fill is conceal_fallback(), the centre nearest zero.
        order='rans', lanes=W (container format 12; W in codec.RANS_LANES, default codec.DEFAULT_RANS_LANES): the stream of W
        interleaved rANS coders, codec.rans_encode over the same tables: logits and symbols are gathered through
        codec.rans_rounds(C, h, w, W) on the device, a hole as IC_PC_ENCODE_SKIP, and one wave per volume codes the rounds backwards
        (ic_pc_encode_segments_f32 with nsegs = -W).  Not with seg_ends or depth_block."""
        dev = self.centers.device
        sym = symbols if torch.is_tensor(symbols) else torch.as_tensor(np.ascontiguousarray(symbols))
        batched = sym.dim() == 4
        if not batched:
            sym = sym[None]
        assert sym.dim() == 4, 'Expected CHW or NCHW symbols'
        sym = sym.to(dev).long().contiguous()
        N, C, h, w = (int(v) for v in sym.shape)
        logits = self._symbol_logits(sym)
        count = C * h * w
        if order == 'rans':
            if seg_ends is not None or depth_block is not None:
                raise ValueError("order='rans' is one interleaved stream per volume: not with seg_ends or depth_block")
            res = self._encode_rans(logits, sym, lanes, capacity)
            return res if batched else res[0]
        if lanes is not None:
            raise ValueError("lanes is the number of coders of order='rans', order is {!r}".format(order))
        if order not in ('raster', 'wavefront'):
            raise ValueError("order is 'raster' or 'wavefront' -- or 'rans' --, got {!r}".format(order))
        coded, planes = sym, None
        if depth_block is not None:
            from .codec import check_depth_block
            B = check_depth_block(depth_block, C)
            if order != 'wavefront' or seg_ends is not None:
                raise ValueError("depth_block leaves positions out of the wavefront order: order is {!r}{}".format(
                    order, '' if seg_ends is None else ', with seg_ends'))
            planes, keep = self._depth_plane(sym, B)
            coded = torch.where(keep, sym, torch.full_like(sym, _lib.PC_ENCODE_SKIP))
        if order == 'wavefront':
            logits, coded = self._in_wavefront_order(logits, coded)
        if planes is not None:
            planes = planes.to(torch.uint8).cpu().numpy()       # (the host waits here, behind the gather)
        if seg_ends is not None:
            if order != 'raster':
                raise ValueError("seg_ends cuts a raster stream: order is {!r}".format(order))
            res = self._encode_segments(logits, sym, N, count, [int(e) for e in seg_ends], capacity)
            return res if batched else res[0]
        streams = self._encode_launch(logits, coded, N, count, count, capacity, None, 'rows')
        res = [((b'' if planes is None else planes[n].tobytes()) + streams[n], int(sym[n, 0, 0, 0])) for n in range(N)]
        return res if batched else res[0]

    def _symbol_logits(self, sym):
        """the logits (N,C,h,w,L) of a batch (N,C,h,w) of symbol volumes on the device: padded with symbol 0, the centres gathered,
        pc.logits on the padded volume, as _tables does"""
        pad = self.pc_class.get_context_size(self.config) // 2
        q = self.centers[torch.nn.functional.pad(sym, (pad, pad, pad, pad, pad, 0))].contiguous()    # (N,C+4,h+8,w+8), symbol 0 around
        return self.pc.logits(q, is_training=False)

    def _in_wavefront_order(self, logits, coded):
        """logits (N,C,h,w,L) and what is coded (N,C,h,w), gathered through the permutation of the volume's wavefront order on the device
        -> ((N,count,L), (N,count))"""
        from .codec import wavefront_order
        N, C, h, w = (int(v) for v in coded.shape)
        perm = torch.as_tensor(np.array(wavefront_order(C, h, w))).to(coded.device)       # (a copy: the cached order is read-only)
        return (logits.view(N, C * h * w, self.pc.L).index_select(1, perm).contiguous(),
                coded.reshape(N, C * h * w).index_select(1, perm).contiguous())

    def _encode_launch(self, logits, coded, N, count, longest, capacity, segments, take):
        """ONE launch of the coding side and what comes back: segments=None -> ic_pc_encode_f32, a coder per volume; (ends, nsegs) ->
        ic_pc_encode_segments_f32 with these.  Every coder has `capacity` bytes, by default what `longest` symbols can take; -> the bytes
        of every coder in the launch's order, or the ValueError of _encode_status.  take says how they come back, the one thing that
        differs between the callers: 'rows' copies every coder's bytes by themselves, 'head' and 'tail' copy the whole buffer once and
        cut the first / the LAST nbytes of every capacity."""
        dev = self.centers.device
        cap = int(lib.ic_pc_encode_capacity_bytes(longest)) if capacity is None else int(capacity)
        units = N * (segments[1] if segments is not None and segments[1] > 0 else 1)
        out = torch.empty((units, max(cap, 1)), dtype=torch.uint8, device=dev)
        info = torch.zeros((2, units), dtype=torch.int64, device=dev)   # row 0: nbytes; row 1: status (int32 in the low words)
        status = info[1].view(torch.int32)[:units]
        if segments is None:
            check(lib.ic_pc_encode_f32(ptr(logits), ptr(coded), N, count, self.pc.L, self.freqs_resolution, ptr(out), cap,
                                       ptr(info[0]), ptr(status), _lib.current_stream(dev)), 'ic_pc_encode_f32')
        else:
            host_ends = (ctypes.c_longlong * len(segments[0]))(*segments[0])
            check(lib.ic_pc_encode_segments_f32(ptr(logits), ptr(coded), N, count, self.pc.L, self.freqs_resolution, host_ends, segments[1],
                                                ptr(out), cap, ptr(info[0]), ptr(status), _lib.current_stream(dev)), 'ic_pc_encode_segments_f32')
        nbytes = info[0].tolist()
        for st in status.tolist():
            self._encode_status(st)
        if take == 'rows':
            return [bytes(out[u, :nbytes[u]].cpu().numpy()) for u in range(units)]
        host = out.cpu().numpy()
        return [bytes(host[u, cap - nbytes[u]:cap] if take == 'tail' else host[u, :nbytes[u]]) for u in range(units)]

    def _encode_rans(self, logits, sym, lanes, capacity):
        """encode_stream(order='rans') behind the logits: (N,C,h,w,L) logits and (N,C,h,w) symbols -> [(stream, first_sym)]"""
        from .codec import rans_rounds, check_rans_lanes, DEFAULT_RANS_LANES, RANS_M
        dev = self.centers.device
        W = check_rans_lanes(DEFAULT_RANS_LANES if lanes is None else lanes)
        N, C, h, w = (int(v) for v in sym.shape)
        rounds = torch.as_tensor(np.array(rans_rounds(C, h, w, W))).to(dev).view(-1)          # (a copy: the cached rounds are read-only)
        count = int(rounds.numel())
        firsts = [int(v) for v in sym[:, 0, 0, 0].tolist()]
        if count == 0:                                       # a 1 x 1 x 1 volume: nothing is coded, the coders rest at their initial state
            return [(np.full(W, RANS_M, dtype='<u4').tobytes(), f) for f in firsts]
        at = rounds.clamp(min=0)
        glog = logits.view(N, C * h * w, self.pc.L).index_select(1, at).contiguous()
        coded = torch.where(rounds >= 0, sym.view(N, C * h * w).index_select(1, at),
                            torch.full((), _lib.PC_ENCODE_SKIP, dtype=torch.int64, device=dev)).contiguous()
        return list(zip(self._encode_launch(glog, coded, N, count, count, capacity, ([count], _lib.PC_ENCODE_RANS(W)), 'tail'), firsts))

    def _depth_plane(self, sym, B):
        """codec.depth_plane and the live positions of a batch (N,C,h,w) of symbol volumes on their device -> ((N, ceil(h/B), ceil(w/B))
        int64 depths, (N,C,h,w) bool keep)"""
        N, C, h, w = (int(v) for v in sym.shape)
        fill = self.conceal_fallback()
        chan = torch.arange(C, device=sym.device).view(1, C, 1, 1)
        cell = ((sym != fill) * (chan + 1)).amax(1)                      # per cell: 1 + the deepest channel that holds something, 0: none
        nby, nbx = -(-h // B), -(-w // B)
        cell = torch.nn.functional.pad(cell, (0, nbx * B - w, 0, nby * B - h))
        depth = cell.view(N, nby, B, nbx, B).amax((2, 4))
        per_cell = depth.repeat_interleave(B, 1).repeat_interleave(B, 2)[:, :h, :w]
        return depth, chan < per_cell[:, None]

    @staticmethod
    def _encode_status(st):
        if st == 1:
            raise ValueError('Cannot code symbol because total is too large')
        if st != 0:
            raise ValueError('device range encoder: {} (status {})'.format(
                {2: 'stream capacity too small', 3: 'symbol outside [0, L)'}.get(st, 'error'), st))

    def _encode_segments(self, logits, sym, N, count, ends, capacity):
        """encode_stream(seg_ends=ends) behind the logits: one launch of N * len(ends) work-groups"""
        G = len(ends)
        if not 1 <= G <= 16 or ends[0] < 1 or ends[-1] != count or any(b <= a for a, b in zip(ends, ends[1:])):
            raise ValueError('segment ends {} are not 1 to 16 increasing symbol counts from at least 1 to {}'.format(ends, count))
        longest = max(b - max(1, a) for a, b in zip([0] + ends, ends))
        segs = self._encode_launch(logits, sym, N, count, longest + 1, capacity, (ends, G), 'head')
        return [(segs[n * G:(n + 1) * G], int(sym[n, 0, 0, 0])) for n in range(N)]

    def _encode_fronts(self, symbols, layer_ends, capacity=None):
        """a batch (N,C,h,w) of volumes of one shape, each coded in wavefront order and cut at fronts (container format 8): logits and
        symbols gathered through codec.wavefront_order(C, h, w) on the device, as encode_stream(order='wavefront') does it, then ONE
        ic_pc_encode_segments_f32 launch with the cuts codec.front_layer_cuts(C, h, w, layer_ends) -> [([segment bytes per layer],
        first_sym)].  Segment g is arithmetic_coding.encode_sequence over the permuted symbols and tables [max(1, n_{g-1}), n_g)."""
        from .codec import front_layer_cuts
        sym = symbols.to(self.centers.device).long().contiguous()
        N, C, h, w = (int(v) for v in sym.shape)
        cuts = front_layer_cuts(C, h, w, layer_ends)
        logits, coded = self._in_wavefront_order(self._symbol_logits(sym), sym)
        return self._encode_segments(logits, coded.view(N, C * h * w, 1, 1), N, C * h * w, cuts, capacity)

    def _preview(self, channels, C):
        """channels=None -> None (the full decode, the old entries); else (channels, fill symbol) for the *_channels entries, which
        exist for the k = 24 kernels only"""
        if channels is None:
            return None
        from .codec import check_channels
        channels = check_channels(channels, C)
        if self.pc._k != 24:
            raise ValueError('a preview (channels={}) needs a context model of width k = 24, this one has k = {}'.format(channels, self.pc._k))
        return channels, self.conceal_fallback()

    def decode_stream(self, stream_bytes, symbols_shape, first_sym, flags=0, channels=None, on_device=False):
        """Row N3: the whole sequential decode on the device (ic_pc_decode_f32) -- per symbol the same context-model
        kernels as get_freqs, the table, the arithmetic-decoder step and the gather of the next context are enqueued
        back to back without a host round trip.  stream_bytes: what the encoder wrote; symbols_shape: un-padded
        (C,h,w); first_sym: the uncoded first symbol.  -> (C,h,w) int64 numpy.
        channels=K: a preview (ic_pc_decode_channels_f32) -- the decoder stops after channels 0 .. K - 1, the others hold the fill
        symbol (conceal_fallback): codec.preview_symbols of the full decode.  None: all channels, the call as it always was.
        on_device=True: -> the (C,h,w) int64 DEVICE tensor instead (Codec.transcode codes it again: the symbols never visit the host)."""
        C, h, w = (int(v) for v in symbols_shape)
        preview = self._preview(channels, C)
        dev = self.centers.device
        data = torch.frombuffer(bytearray(stream_bytes) or bytearray(1), dtype=torch.uint8).to(dev)
        out = torch.empty((C, h, w), dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        need = lib.ic_pc_decode_workspace_bytes(C, h, w, self.pc._k)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        centers = self.centers.contiguous().float()
        args = (ptr(data), len(stream_bytes), int(first_sym), self.pc._tab, ptr(centers), self.pc._k, self.pc.L, self.freqs_resolution,
                ptr(out), ptr(status), C, h, w, ptr(ws), need, int(flags), _lib.current_stream(dev))
        if preview is None:
            check(lib.ic_pc_decode_f32(*args), 'ic_pc_decode_f32')
        else:
            check(lib.ic_pc_decode_channels_f32(*(args + preview)), 'ic_pc_decode_channels_f32')
        if int(status.item()) != 0:
            raise ValueError('Cannot decode symbol because total is too large')
        return out if on_device else out.cpu().numpy()

    def encode_tiles(self, symbols, th, tw, order='raster', layer_ends=None, front_ends=None, depth_block=None, lanes=None):
        """symbols: un-padded (C,h,w) -> [(stream_bytes, first_sym)] for the tiles of codec.tile_grid(h, w, th, tw), in grid order.
        Every tile is coded as a volume of its own: its stream is encode_stream(symbols[:, y0:y0+th', x0:x0+tw']) byte for byte.
        Tiles of one shape (at most four: interior, right column, bottom row, corner) are one encode_stream batch, one launch.
        order='wavefront': every tile's stream in the wavefront order of its own extent (encode_stream).
        layer_ends=[e_0 < ... = C] (raster only, container format 6): every tile's stream cut at these channel planes into segments
        (encode_stream(seg_ends=[e th' tw' ...])) -> [([segment bytes per layer], first_sym)].
        front_ends=[e_0 < ... = C] (container format 8; not with layer_ends or order='wavefront', the order is implied): every tile's
        stream in the wavefront order of its own extent, cut at that extent's fronts codec.front_layer_cuts(C, th', tw', front_ends)
        (_encode_fronts) -> [([segment bytes per layer], first_sym)].
        depth_block=B (order='wavefront' only, container format 10): every tile's stream is its own depth plane, blocks counted from the
        tile's corner, then the coder's bytes of its live positions (encode_stream).
        order='rans', lanes=W (container format 12; not with layer_ends, front_ends or depth_block): every tile's stream is that of W
        interleaved rANS coders over the rounds of its own extent (encode_stream)."""
        return self.encode_tiles_batch([symbols], th, tw, order=order, layer_ends=layer_ends, front_ends=front_ends, depth_block=depth_block,
                                       lanes=lanes)[0]

    @staticmethod
    def _check_front_ends(front_ends, order, layer_ends):
        if front_ends is not None and (layer_ends is not None or order != 'raster'):
            raise ValueError("front_ends cuts the wavefront order at fronts by itself: not with layer_ends (plane cuts of the raster "
                             "order) or order={!r}".format(order))

    @staticmethod
    def _check_depth_block(depth_block, order, layer_ends, front_ends):
        if depth_block is not None and (order != 'wavefront' or layer_ends is not None or front_ends is not None):
            raise ValueError("depth_block leaves positions out of the wavefront order: it needs order='wavefront' (got {!r}) and goes "
                             "with neither layer_ends nor front_ends".format(order))

    def decode_tiles(self, streams, first_syms, symbols_shape, th, tw, flags=0, channels=None, order='raster', lanes=None):
        """The mirror of encode_tiles: all tiles of a volume decoded by ONE launch, one work-group per tile
        (ic_pc_decode_tiles_f32; other k than 24 or non-zero flags: tile after tile, the slow path).  streams / first_syms in the
        order of codec.tile_grid(h, w, th, tw); symbols_shape: un-padded (C,h,w).  -> (C,h,w) int64 numpy.
        channels=K: a preview, through the batch entry as a batch of one (decode_tiles_batch).
        order='rans', lanes=W (container format 12): likewise through the batch entry, whose flag it is."""
        from .codec import tile_grid
        C, h, w = (int(v) for v in symbols_shape)
        if order not in ('raster', 'rans'):
            raise ValueError("decode_tiles reads raster streams or, with order='rans', rANS streams; order {!r} is decode_tiles_batch's".format(order))
        try:
            if channels is not None or order == 'rans':
                return self.decode_tiles_batch([(streams, first_syms, (C, h, w))], th, tw, want='symbols', flags=flags,
                                               channels=channels, order=order, lanes=lanes)[0].cpu().numpy()
            grid = tile_grid(h, w, th, tw)
            if len(streams) != len(grid) or len(first_syms) != len(grid):
                raise ValueError('{} streams and {} first symbols for a grid of {} tiles'.format(len(streams), len(first_syms), len(grid)))
            dev = self.centers.device
            (table, _, data, pos), where = _tile_tables([(0, t, cell, first_syms[t], streams[t], None) for t, cell in enumerate(grid)], dev)
            out = torch.empty((C, h, w), dtype=torch.int64, device=dev)
            status = torch.zeros(len(grid), dtype=torch.int32, device=dev)
            need = lib.ic_pc_decode_tiles_workspace_bytes(C, min(th, h), min(tw, w), len(grid), self.pc._k)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            centers = self.centers.contiguous().float()
            check(lib.ic_pc_decode_tiles_f32(ptr(data), pos, table, len(grid), self.pc._tab, ptr(centers), self.pc._k, self.pc.L,
                                             self.freqs_resolution, ptr(out), ptr(status), C, h, w, ptr(ws), need, int(flags),
                                             _lib.current_stream(dev)), 'ic_pc_decode_tiles_f32')
            _failed_tiles(status, where)                                        # (no report: the first tile that failed is a ValueError)
            return out.cpu().numpy()
        except ValueError as e:
            raise ValueError(str(e).replace('(volume 0, tile ', '(tile '))

    def encode_tiles_batch(self, volumes, th, tw, order='raster', layer_ends=None, front_ends=None, depth_block=None, lanes=None):
        """encode_tiles for a list of un-padded (C,h,w) symbol volumes of any mix of (h, w): -> per volume the list encode_tiles
        gives for it, byte for byte.  The tiles of ALL volumes are grouped by tile shape -- for a folder of equal-sized images the
        same four shapes as for one -- and each group is one encode_stream batch, one ic_pc_encode_f32 launch.
        layer_ends: as encode_tiles, the ends converted to symbol counts per tile shape (raster only).
        front_ends: as encode_tiles, every tile shape by its own cuts.
        depth_block: as encode_tiles.
        order='rans', lanes=W: as encode_tiles."""
        from .codec import tile_grid
        self._check_front_ends(front_ends, order, layer_ends)
        self._check_depth_block(depth_block, order, layer_ends, front_ends)
        dev = self.centers.device
        syms, grids = [], []
        for v in volumes:
            sym = v if torch.is_tensor(v) else torch.as_tensor(np.ascontiguousarray(v))
            assert sym.dim() == 3, 'Expected CHW symbols'
            syms.append(sym.to(dev).long())
            grids.append(tile_grid(int(sym.shape[1]), int(sym.shape[2]), th, tw))
        by_shape = OrderedDict()
        for n, grid in enumerate(grids):
            for t, (y0, x0, a, b) in enumerate(grid):
                by_shape.setdefault((int(syms[n].shape[0]), a, b), []).append((n, t))
        res = [[None] * len(grid) for grid in grids]
        for (_, a, b), members in by_shape.items():
            batch = torch.stack([syms[n][:, grids[n][t][0]:grids[n][t][0] + a, grids[n][t][1]:grids[n][t][1] + b] for n, t in members])
            seg_ends = None if layer_ends is None else [int(e) * a * b for e in layer_ends]
            coded = (self._encode_fronts(batch, front_ends) if front_ends is not None else
                     self.encode_stream(batch, order=order, seg_ends=seg_ends, depth_block=depth_block, lanes=lanes))
            for (n, t), r in zip(members, coded):
                res[n][t] = r
        return res

    def decode_tiles_batch(self, volumes, th, tw, want='q', max_workspace_bytes=1 << 31, flags=0, conceal=False, order='raster',
                           channels=None, layer_ends=None, tile_layers=None, front_ends=None, depth_block=None, lanes=None):
        """The mirror of encode_tiles_batch: the tiles of ALL volumes decoded by one launch per chunk (ic_pc_decode_tiles_batch_f32,
        one work-group per tile).  volumes: [(streams, first_syms, (C,h,w))], each as decode_tiles takes them, one C throughout.
        want: 'q' -> per volume the (C,h,w) float32 DEVICE tensor centers[symbols] (what ae.decode consumes: the symbols never
        visit the host), 'symbols' -> the (C,h,w) int64 device tensor, 'both' -> (q, symbols) pairs.
        The workspace is one slot per tile, so the tile list is cut into chunks whose workspace stays within max_workspace_bytes
        (chunk_tiles; a cut may fall inside a volume); the chunks run one after the other on the current stream.
        A subset: streams[t] may be None -- that tile is skipped, nothing of it is uploaded and no work-group runs for it.
        conceal=False: its cells are 0 (symbol 0, q 0.0).  conceal=True: skipped tiles (reason 'missing') and tiles whose decoder
        status is not 0 (reason 'decoder', instead of the ValueError) are the damaged set; one launch of ic_pc_conceal_tiles
        behind the decoder fills them from their intact neighbours (include/imgcomp_hip.h has the rule; the fallback symbol is
        the centre of smallest magnitude), and the call returns (result as above, [per volume [(tile, reason)] in tile order]).
        order='wavefront': the streams are in wavefront order (encode_tiles(order='wavefront')); sets PC_DECODE_WAVEFRONT, the
        decoder that takes a front at a time.  The order is per call: raster and wavefront volumes do not share one.
        channels=K: a preview (ic_pc_decode_tiles_batch_channels_f32) -- every tile's decoder stops after channels 0 .. K - 1 (in
        wavefront order: after their last front), the others hold the fill symbol / its centre.  Not with conceal=True.
        layer_ends=[e_0 < ... = C] (container format 6, ic_pc_decode_tiles_batch_layers_f32; raster, k = 24, flags 0, not with
        conceal=True): streams[t] is the list of the tile's G segments, as encode_tiles(layer_ends=...) gives them; entries of layers
        that begin at or above `channels` are not read and may be None.
        tile_layers=[per volume [g_t per tile]] (needs layer_ends; not with conceal=True or channels; recovery of a damaged or cut
        format-6 file): tile t is read up to its leading g_t layers, 0 <= g_t <= G, through ic_pc_decode_tiles_batch_layers_pertile_f32.
        g_t = 0 skips the tile like a None stream; its segments of layers >= g_t may be None.  A tile whose decoder status is not 0
        counts as holding nothing (reason 'decoder', instead of the ValueError).  Then, if any tile holds fewer than C channels, one
        ic_pc_conceal_tiles_channels launch fills every missing (tile, channel) from the neighbours that hold that channel (the
        fallback is the fill symbol, so a channel no neighbour holds is that of a preview).  The call returns (result as above, [per
        volume [(tile, layers_read, channels, reason)] in tile order for the tiles that hold fewer than C channels]); reason is
        'decoder' or None (the caller's own limit).
        front_ends=[e_0 < ... = C] (container format 8, ic_pc_decode_tiles_batch_fronts_f32 / _fronts_pertile_f32): everything said of
        layer_ends -- channels, tile_layers, what may be None, what is returned -- for streams[t] = the tile's G segments of its
        wavefront order cut at fronts, as encode_tiles(front_ends=...) gives them.  Not with layer_ends or order='wavefront' (the
        order is implied).
        depth_block=B (container format 10; order='wavefront', k = 24, flags 0; not with conceal=True, layer_ends, tile_layers or
        front_ends): streams[t] is the tile's depth plane, then the coder's bytes of its live positions, as
        encode_tiles(order='wavefront', depth_block=B) gives them; sets PC_DECODE_DEPTH(B) on ic_pc_decode_tiles_batch_channels_f32,
        whose `channels` is C unless channels=K asks for a preview.  A dead position holds the fill symbol / its centre.  A stream
        shorter than its plane is a ValueError that names the tile.
        order='rans', lanes=W (container format 12; k = 24, flags 0; not with conceal=True, layer_ends, tile_layers, front_ends or
        depth_block): streams[t] is the tile's stream of W interleaved rANS coders, as encode_tiles(order='rans', lanes=W) gives it;
        sets PC_DECODE_RANS(W) on ic_pc_decode_tiles_batch_channels_f32, whose `channels` is C unless channels=K asks for a preview.
        A full decode checks the stream's end: a ValueError that names the tile tells a stream that does not end where the coders'
        run ends (status 4) from a table whose total is too large (status 1)."""
        mode = self._decode_mode(want, int(volumes[0][2][0]) if volumes else None, conceal, order, channels, layer_ends, tile_layers,
                                 front_ends, depth_block, lanes, flags)
        if not volumes:
            return ([], []) if conceal or tile_layers is not None else []
        dev = self.centers.device
        shapes, grids, listed, missing, limits = _list_tiles(volumes, th, tw, mode, tile_layers)
        chunks, ws, ws_bytes = self._chunk_plan(mode, [cell for _, _, cell, _, _, _ in listed], len(shapes), max_workspace_bytes)
        tables, where = _tile_tables(listed, dev)
        vtable, offs, total = _lib.packed_volume_table(shapes)
        alloc = torch.zeros if missing else torch.empty
        q = alloc(total, dtype=torch.float32, device=dev) if want in ('q', 'both') else None
        sym = alloc(total, dtype=torch.int64, device=dev) if want in ('symbols', 'both') or mode.report is not None else None    # the rules read symbols
        status = torch.zeros(len(listed), dtype=torch.int32, device=dev)
        centers = self.centers.contiguous().float()
        per_tile = () if tile_layers is None else ((ctypes.c_int * max(len(limits), 1))(*limits),)
        for a, b in chunks:
            self._launch_tiles(mode, tables, vtable, len(shapes), sym, q, status, ws, ws_bytes, centers, a, b, per_tile)
        failed = _failed_tiles(status, where, mode.report, mode.coder)
        if mode.report is None:
            return _cut(q, sym, shapes, offs, want)
        if mode.report == 'held':
            held = self._conceal_held(sym, q, shapes, grids, vtable, tile_layers, set(failed), mode.ends, th, tw, centers)
            return _cut(q, sym, shapes, offs, want), held
        marked = [(n, t, 'missing') for n, t in missing] + [(n, t, 'decoder') for n, t in failed]
        damage = [sorted((t, why) for m, t, why in marked if m == n) for n in range(len(shapes))]
        if any(damage):
            self._conceal(sym, q, shapes, grids, vtable, damage, th, tw, centers)
        return _cut(q, sym, shapes, offs, want), damage

    def choose_tiles_batch(self, zs, th, tw, lam, want='symbols', max_workspace_bytes=1 << 31):
        """Rate-aware symbol choice at encode: the symbols of every th x tw tile of every volume, chosen front by front by the
        rule of codec.rdo_choose over the context model's own tables -- ONE launch per chunk of ic_pc_decode_tiles_batch_channels_f32
        with PC_DECODE_RDO, one work-group per tile, the sweep of the wavefront decoder with a chooser in place of a coder.
        zs: [(C, h, w) float32 DEVICE tensors], the masked bottleneck values (EncoderOutput.z), one C throughout.  lam: a float (in
        key units per bit, codec.rdo_lambda_q), or per volume a sequence with one lambda per tile in codec.tile_grid order.
        want: 'symbols' -> per volume the (C, h, w) int64 device tensor, 'q' -> centers[symbols] as float32, 'both' -> (q, symbols).
        The records (Lambda, then the tile's z) are gathered on the device; nothing visits the host but the status words.
        The workspace is one slot per tile: the tile list is cut into chunks within max_workspace_bytes as decode_tiles_batch does.
        A context model of another width than k = 24 is a ValueError; a table whose total is too large (status 1) too."""
        from .codec import tile_grid, rdo_is_sequence, rdo_lambda_q, rdo_tile_lambdas, rdo_record_bytes
        if want not in ('q', 'symbols', 'both'):
            raise ValueError("want is 'q', 'symbols' or 'both', got {!r}".format(want))
        if self.pc._k != 24:
            raise ValueError('rate-aware symbol choice needs a context model of width k = 24, this one has k = {}'.format(self.pc._k))
        zs = list(zs)
        if not zs:
            return []
        dev = self.centers.device
        per_volume = rdo_is_sequence(lam)
        if per_volume and len(lam) != len(zs):
            raise ValueError('lam: {} entries for {} volumes'.format(len(lam), len(zs)))
        shapes, rows, lams, pos = [], [], [], 0
        for n, z in enumerate(zs):
            if z.dim() != 3 or z.dtype != torch.float32:
                raise ValueError('volume {}: z is a (C, h, w) float32 tensor, got {} {}'.format(n, tuple(z.shape), z.dtype))
            _lib.require_cuda(z, 'z of volume {}'.format(n))
            C, h, w = (int(v) for v in z.shape)
            if C != int(zs[0].shape[0]):
                raise ValueError('volume {} has {} channels, volume 0 has {}'.format(n, C, int(zs[0].shape[0])))
            shapes.append((C, h, w))
            grid = tile_grid(h, w, th, tw)
            for (y0, x0, a, b), lm in zip(grid, rdo_tile_lambdas(lam[n] if per_volume else lam, len(grid))):
                nb = rdo_record_bytes(C, a, b)
                rows.append((y0, x0, a, b, pos, nb, 0, n))
                lams.append(rdo_lambda_q(lm))
                pos += (nb + 7) & ~7                                 # every record starts at a multiple of 8
        C = shapes[0][0]
        # the records, gathered on the device: Lambda of every tile by one upload and one indexed store, z by one strided copy per tile
        data = torch.zeros(pos, dtype=torch.uint8, device=dev)
        lam_dev = torch.as_tensor(np.asarray(lams, dtype='<f8')).to(dev)
        at = torch.as_tensor(np.asarray([r[4] // 8 for r in rows], dtype=np.int64)).to(dev)
        data.view(torch.float64)[at] = lam_dev                       # (every record starts at a multiple of 8: one indexed store)
        for y0, x0, a, b, off, nb, _, n in rows:
            data[off + 8:off + nb].view(torch.float32).view(C, a, b).copy_(zs[n][:, y0:y0 + a, x0:x0 + b])
        # the sweep of the wavefront decoder with a chooser in place of a coder: the full decode's tail, no fill symbol
        mode = _tiles_mode('_channels', C, _lib.PC_DECODE_RDO, (C, 0), coder='rdo')
        vtable, offs, total = _lib.packed_volume_table(shapes)
        chunks, ws, ws_bytes = self._chunk_plan(mode, [r[:4] for r in rows], len(shapes), max_workspace_bytes)
        q = torch.empty(total, dtype=torch.float32, device=dev) if want in ('q', 'both') else None
        sym = torch.empty(total, dtype=torch.int64, device=dev) if want in ('symbols', 'both') else None
        status = torch.zeros(len(rows), dtype=torch.int32, device=dev)
        centers = self.centers.contiguous().float()
        tables = (_lib.tile_table(rows), None, data, pos)
        for a, b in chunks:
            self._launch_tiles(mode, tables, vtable, len(shapes), sym, q, status, ws, ws_bytes, centers, a, b)
        _failed_tiles(status, [(n, None, y0, x0) for y0, x0, _, _, _, _, _, n in rows], coder='rdo')
        return _cut(q, sym, shapes, offs, want)

    def _decode_mode(self, want, C, conceal, order, channels, layer_ends, tile_layers, front_ends, depth_block, lanes, flags):
        """THE decision of decode_tiles_batch, on the host alone: which keywords go together, and for those that do the _TilesMode
        the call launches.  Every refusal of a combination is here, in this order.  C: the volumes' channels, which the ends, `channels`
        and the depth block are checked against; None (no volumes) -> None once the keywords have been checked.  The context model's
        width is read only where a check needs it."""
        from .codec import check_channels, check_layer_ends, check_depth_block, check_rans_lanes, DEFAULT_RANS_LANES
        rans = None
        if order == 'rans':
            if conceal or layer_ends is not None or tile_layers is not None or front_ends is not None or depth_block is not None or int(flags) != 0:
                raise ValueError("order='rans' does not go with conceal=True, layer_ends, tile_layers, front_ends, depth_block or flags "
                                 "({})".format(flags))
            if self.pc._k != 24:
                raise ValueError('lane-parallel rANS tiles need a context model of width k = 24, this one has k = {}'.format(self.pc._k))
            rans = check_rans_lanes(DEFAULT_RANS_LANES if lanes is None else lanes)
        elif lanes is not None:
            raise ValueError("lanes is the number of coders of order='rans', order is {!r}".format(order))
        if depth_block is not None:
            self._check_depth_block(depth_block, order, layer_ends, front_ends)
            if conceal or tile_layers is not None or int(flags) != 0:
                raise ValueError('depth_block does not go with conceal=True, tile_layers or flags ({})'.format(flags))
            if self.pc._k != 24:
                raise ValueError('depth-mapped tiles need a context model of width k = 24, this one has k = {}'.format(self.pc._k))
        kind = '_layers'
        if front_ends is not None:
            self._check_front_ends(front_ends, order, layer_ends)
            kind, layer_ends = '_fronts', front_ends
        if layer_ends is not None:
            if conceal:
                raise ValueError('layer_ends with conceal=True: salvage of layered tiles is not offered')
            if order != 'raster' or int(flags) != 0:
                raise ValueError('layer_ends cuts raster streams for the k = 24 decoder: order {!r}, flags {}'.format(order, flags))
            if self.pc._k != 24:
                raise ValueError(_NEEDS_K24.format(self.pc._k))
        if tile_layers is not None:
            if layer_ends is None:
                raise ValueError('tile_layers counts layers per tile: it needs layer_ends')
            if conceal or channels is not None:
                raise ValueError('tile_layers does not go with conceal=True or channels: it conceals per channel by itself, and '
                                 'every tile has its own limit')
        if channels is not None and conceal:
            raise ValueError('channels={} with conceal=True: a preview of a damaged file is not offered'.format(channels))
        if want not in ('q', 'symbols', 'both'):
            raise ValueError("want is 'q', 'symbols' or 'both', got {!r}".format(want))
        if order not in ('raster', 'wavefront', 'rans'):
            raise ValueError("order is 'raster' or 'wavefront' -- or 'rans' --, got {!r}".format(order))
        if C is None:
            return None
        flags = int(flags) | (_lib.PC_DECODE_WAVEFRONT if order == 'wavefront' else 0)
        ends, read = None, 0
        if layer_ends is not None:
            ends = check_layer_ends(layer_ends, C)
            upto = C if channels is None else check_channels(channels, C)
            read = len([g for g in range(len(ends)) if g == 0 or ends[g - 1] < upto])      # the layers that begin below `channels`: 0 .. read - 1
        preview = self._preview(channels, C)
        if depth_block is not None:
            flags |= _lib.PC_DECODE_DEPTH(check_depth_block(depth_block, C))
        if rans is not None:
            flags = _lib.PC_DECODE_RANS(rans)                     # alone in the flags: the order is implied
        if tile_layers is not None:
            return _tiles_mode(kind + '_pertile', C, flags, (self.conceal_fallback(),), ends, read, 'held')
        if ends is None and preview is None and depth_block is None and rans is None:
            return _tiles_mode('', C, flags, (), report='damage' if conceal else None)
        # the entries that take (channels, fill symbol): channels == C is the full decode
        coder = 'depth' if depth_block is not None else 'rans' if rans is not None else None
        return _tiles_mode(kind if ends is not None else '_channels', C, flags, preview or (C, self.conceal_fallback()), ends, read, coder=coder)

    def _chunk_plan(self, mode, tiles, nvolumes, max_workspace_bytes):
        """the tiles [(y0, x0, a, b)] of a call cut into chunks whose workspace stays within max_workspace_bytes (codec.chunk_tiles by
        the mode's own size) -> ([(start, stop)], ONE workspace for the largest chunk, its bytes)"""
        from .codec import chunk_tiles

        def need(th_max, tw_max, ntiles):
            return mode.size(mode.C, th_max, tw_max, ntiles, nvolumes, self.pc._k)
        chunks = chunk_tiles([(a, b) for _, _, a, b in tiles], need, int(max_workspace_bytes))
        ws_bytes = max([need(max(tiles[i][2] for i in range(a, b)), max(tiles[i][3] for i in range(a, b)), b - a) for a, b in chunks], default=0)
        return chunks, torch.empty(ws_bytes, dtype=torch.uint8, device=self.centers.device), ws_bytes

    def _launch_tiles(self, mode, tables, vtable, nvolumes, sym, q, status, ws, ws_bytes, centers, a, b, per_tile=()):
        """ONE launch of the mode's entry over the rows [a, b) of a call's tiles: the 19 arguments every entry takes, with the tile
        table, the status words, the per-tile tables of the entry's own tail (limits; the session's from) and the segment table from
        row a on, then the tail's scalars and, for the segmented entries, layer_ends, nlayers, segs.  tables: (tile table, segment
        table, the bytes on the device, their number), as _tile_tables gives them."""
        table, seg_table, data, pos = tables

        def from_row(arr, per_row=1):
            return ctypes.c_void_p(ctypes.addressof(arr) + a * per_row * ctypes.sizeof(arr._type_))
        args = (ptr(data), pos, from_row(table), b - a, vtable, nvolumes, self.pc._tab, ptr(centers), self.pc._k, self.pc.L,
                self.freqs_resolution, ptr(sym), ptr(q), ptr(status[a:b]), mode.C, ptr(ws), ws_bytes, mode.flags,
                _lib.current_stream(self.centers.device))
        args += tuple(from_row(arr) for arr in per_tile) + mode.tail
        if mode.ends is not None:
            args += ((ctypes.c_int * len(mode.ends))(*mode.ends), len(mode.ends), from_row(seg_table, len(mode.ends)))
        check(mode.call(*args), mode.name)

    def open_layers(self, volumes_geometry, th, tw, layer_ends=None, max_workspace_bytes=1 << 31, front_ends=None):
        """a LayerSession over the volumes [(C,h,w)] cut into th x tw tiles of layered streams (container format 6): the decoder's
        workspace, symbols and q stay on the device between its advance() calls, so that every layer of every tile is decoded once
        however often the caller looks at what has arrived (ic_pc_decode_tiles_batch_layers_resume_f32).
        front_ends in place of layer_ends (exactly one of the two): the same session over front-layered streams (container format 8,
        ic_pc_decode_tiles_batch_fronts_resume_f32): every front of every tile is swept once"""
        if (layer_ends is None) == (front_ends is None):
            raise ValueError('a session is opened with layer_ends (plane cuts, format 6) or with front_ends (front cuts, format 8): '
                             'exactly one of the two')
        return LayerSession(self, volumes_geometry, th, tw, layer_ends if front_ends is None else front_ends, max_workspace_bytes,
                            fronts=front_ends is not None)

    def conceal_fallback(self):
        """the symbol a tile gets that has no intact neighbour: the centre of smallest magnitude (ties: the smallest index), what
        the quantiser emits where the importance map has masked a channel"""
        from .codec import fill_symbol
        return fill_symbol(self.centers.detach().float().cpu().numpy())

    def _conceal(self, sym, q, shapes, grids, vtable, damage, th, tw, centers):
        """one ic_pc_conceal_tiles launch on the current stream for the damaged tiles of all volumes; sym / q as decode_tiles_batch
        lays them out (q may be None)"""
        marks, tiles = [], []
        for n, (grid, dmg) in enumerate(zip(grids, damage)):
            m = bytearray(len(grid))
            for t, _ in dmg:
                m[t] = 1
                tiles.append(grid[t] + (0, 0, 0, n))
            marks.append(bytes(m))
        marks = b''.join(marks)
        self._conceal_launch('ic_pc_conceal_tiles', sym, q, tiles, shapes, vtable, ctypes.create_string_buffer(marks, len(marks)), len(marks),
                             th, tw, centers)

    def _conceal_channels(self, sym, q, shapes, grids, vtable, have, th, tw, centers):
        """one ic_pc_conceal_tiles_channels launch on the current stream: have[n][t] = the leading channels tile t of volume n holds;
        every (tile, channel) at or above it is filled.  sym / q as decode_tiles_batch lays them out (q may be None)"""
        C = shapes[0][0]
        tiles = [grid[t] + (0, 0, 0, n) for n, (grid, row) in enumerate(zip(grids, have)) for t in range(len(grid)) if row[t] < C]
        flat = [int(v) for row in have for v in row]
        self._conceal_launch('ic_pc_conceal_tiles_channels', sym, q, tiles, shapes, vtable, (ctypes.c_uint16 * len(flat))(*flat), len(flat),
                             th, tw, centers)

    def _conceal_launch(self, name, sym, q, tiles, shapes, vtable, host_marks, nmarks, th, tw, centers):
        """the launch of either conceal entry: `tiles` are filled by the rule over host_marks, one mark per tile of every volume"""
        dev = self.centers.device
        table = _lib.tile_table(tiles)
        need = int(getattr(lib, name + '_workspace_bytes')(len(tiles), len(shapes), nmarks))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        check(getattr(lib, name)(ptr(sym), ptr(q), table, len(tiles), vtable, len(shapes), host_marks, ptr(centers), self.pc.L,
                                 self.conceal_fallback(), shapes[0][0], int(th), int(tw), ptr(ws), need, _lib.current_stream(dev)), name)
        torch.cuda.current_stream(dev).synchronize()        # the three host tables and the workspace are done with

    def _conceal_held(self, sym, q, shapes, grids, vtable, tile_layers, failed, ends, th, tw, centers):
        """what decode_tiles_batch(tile_layers=...) and LayerSession.advance report: -> [per volume [(tile, layers_read, channels,
        reason)] in tile order for the tiles that hold fewer than C channels]; a tile in `failed` = {(n, t)} holds nothing, reason
        'decoder'.  If there is any such tile, _conceal_channels has filled what they do not hold."""
        C = shapes[0][0]
        held, have = [], []
        for n, grid in enumerate(grids):
            row = [0 if (n, t) in failed or int(tile_layers[n][t]) == 0 else ends[int(tile_layers[n][t]) - 1] for t in range(len(grid))]
            have.append(row)
            held.append([(t, 0 if (n, t) in failed else int(tile_layers[n][t]), row[t], 'decoder' if (n, t) in failed else None)
                         for t in range(len(grid)) if row[t] < C])
        if any(held):
            self._conceal_channels(sym, q, shapes, grids, vtable, have, th, tw, centers)
        return held

    def get_pr(self, input_ctx):
        """:param input_ctx: symbols of ONE context, CHW = input_ctx_shape -> (L,) float32."""
        assert tuple(input_ctx.shape) == tuple(self.input_ctx_shape), '{} != {}'.format(
            input_ctx.shape, self.input_ctx_shape)
        return self._tables(input_ctx)[0][0]

    def get_freqs(self, input_ctx):
        """:param input_ctx: symbols of ONE context, CHW -> (L,) int64, all > 0."""
        assert tuple(input_ctx.shape) == tuple(self.input_ctx_shape), '{} != {}'.format(
            input_ctx.shape, self.input_ctx_shape)
        f = self._tables(input_ctx)[1][0]
        assert np.all(f > 0), 'We do not want zero frequencies!: {}'.format(f)
        return f


# How one call of the tile decoder goes to the library (PredictionNetwork._decode_mode; choose_tiles_batch and LayerSession build
# theirs).  flags: the final ones.  name, call, size: the entry, and its workspace bytes as a function of (C, th_max, tw_max, ntiles,
# nvolumes, k).  tail: the scalars of the entry's own tail, behind its per-tile tables and in front of layer_ends, nlayers, segs.
# C: the volumes' channels.  ends: the checked layer ends of a segmented entry, else None; read: the leading layers a tile is read up
# to unless tile_layers says otherwise.  report: what the call returns beside the result -- None (a status that is not 0 is a
# ValueError, in the words of `coder`: None, 'depth', 'rans' or 'rdo'), 'damage' or 'held' (these read the symbols: always allocated).
_TilesMode = namedtuple('_TilesMode', 'flags name call size tail C ends read report coder')
_NEEDS_K24 = 'layered tiles need a context model of width k = 24, this one has k = {}'


def _tiles_mode(kind, C, flags=0, tail=(), ends=None, read=0, report=None, coder=None):
    """the _TilesMode of the entry ic_pc_decode_tiles_batch<kind>_f32, kind '' / '_channels' / '_layers' / '_fronts', the latter two
    also with '_pertile' / '_resume': the one place where these names reach the library"""
    name = 'ic_pc_decode_tiles_batch{}_f32'.format(kind)
    size = getattr(lib, 'ic_pc_decode_tiles_batch{}_workspace_bytes'.format('' if kind == '_channels' else kind))
    nlayers = () if ends is None else (len(ends),)
    return _TilesMode(flags, name, getattr(lib, name), lambda *geometry: int(size(*(geometry + nlayers))), tail, C, ends, read, report, coder)


def _list_tiles(volumes, th, tw, mode, tile_layers=None, opened=None):
    """volumes [(streams, first_syms, (C,h,w))] -> (shapes, grids, listed, missing, limits): listed = the tiles that are read, as
    _tile_tables takes them; missing = [(n, t)] of those that are not (no stream, or 0 layers); limits = per listed tile the channels
    its layers hold, with tile_layers = [per volume [g_t per tile]].  Without it a tile of a segmented mode is read up to mode.read
    layers.  opened = (shapes, grids) of a LayerSession: its volumes may come without a shape and are counted in its words."""
    from .codec import tile_grid
    ends = mode.ends
    shapes, grids, listed, missing, limits = [], [], [], [], []
    if opened is None and tile_layers is not None and len(tile_layers) != len(volumes):
        raise ValueError('tile_layers has {} entries for {} volumes'.format(len(tile_layers), len(volumes)))
    for n, volume in enumerate(volumes):
        streams, first_syms = volume[0], volume[1]
        if opened is None:
            C, h, w = (int(v) for v in volume[2])
            if C != mode.C:
                raise ValueError('volume {} has {} channels, volume 0 has {}'.format(n, C, mode.C))
            grid = tile_grid(h, w, th, tw)
            if len(streams) != len(grid) or len(first_syms) != len(grid):
                raise ValueError('volume {}: {} streams and {} first symbols for a grid of {} tiles'.format(
                    n, len(streams), len(first_syms), len(grid)))
            if tile_layers is not None and len(tile_layers[n]) != len(grid):
                raise ValueError('volume {}: tile_layers has {} entries for a grid of {} tiles'.format(n, len(tile_layers[n]), len(grid)))
        else:
            (C, h, w), grid = opened[0][n], opened[1][n]
            if len(volume) > 2 and tuple(int(v) for v in volume[2]) != (C, h, w):
                raise ValueError('volume {} is {}, the session was opened for {}'.format(n, tuple(volume[2]), (C, h, w)))
            if len(streams) != len(grid) or len(first_syms) != len(grid) or len(tile_layers[n]) != len(grid):
                raise ValueError('volume {}: {} streams, {} first symbols and {} entries of tile_layers for a grid of {} tiles'.format(
                    n, len(streams), len(first_syms), len(tile_layers[n]), len(grid)))
        shapes.append((C, h, w))
        grids.append(grid)
        for t, cell in enumerate(grid):
            if tile_layers is not None:
                g_t = int(tile_layers[n][t])
                if not 0 <= g_t <= len(ends):
                    raise ValueError('volume {}, tile {}: {} layers to read of {}'.format(n, t, g_t, len(ends)))
                if g_t == 0:
                    missing.append((n, t))
                    continue
                if streams[t] is None or len(streams[t]) != len(ends) or any(streams[t][g] is None for g in range(g_t)):
                    raise ValueError('volume {}, tile {}: {} layers to read need the segments 0 .. {} of {}'.format(n, t, g_t, g_t - 1, len(ends)))
                listed.append((n, t, cell, first_syms[t], streams[t], range(g_t)))
                limits.append(ends[g_t - 1])
            elif streams[t] is None:
                missing.append((n, t))
            elif ends is not None:
                if len(streams[t]) != len(ends) or any(streams[t][g] is None for g in range(mode.read)):
                    raise ValueError('volume {}, tile {}: {} layers need the segments {} of {}'.format(
                        n, t, len(ends), list(range(mode.read)), len(ends)))
                listed.append((n, t, cell, first_syms[t], streams[t], range(mode.read)))
            else:
                listed.append((n, t, cell, first_syms[t], streams[t], None))
    return shapes, grids, listed, missing, limits


def _failed_tiles(status, where, report=None, coder=None):
    """the status words of a call's launches, row for row with where = [(n, t, y0, x0)]: THE host wait of the call, after which the
    tables and the streams are done with.  -> [(n, t)] of the rows whose status is not 0, for a call that reports them (_TilesMode.report);
    else the first of them is the ValueError, in the coder's words."""
    failed = []
    for (n, t, y0, x0), st in zip(where, status.tolist()):
        if st == 0:
            continue
        if report is not None:
            failed.append((n, t))
            continue
        if coder == 'rdo':
            raise ValueError('Cannot choose symbol because total is too large (volume {}, tile at ({}, {}))'.format(n, y0, x0))
        if coder == 'depth' and st == 2:
            raise ValueError('stream shorter than its depth plane (volume {}, tile {} at ({}, {}))'.format(n, t, y0, x0))
        if coder == 'rans' and st & 4 and not st & 1:                # (status 1 beside it: the total is the cause, said below)
            raise ValueError('the stream does not end where the coders\' run ends: a coder state is not 2^16 or bytes are missing '
                             'or left over (status {}; volume {}, tile {} at ({}, {}))'.format(st, n, t, y0, x0))
        raise ValueError('Cannot decode symbol because total is too large (volume {}, tile {} at ({}, {}))'.format(n, t, y0, x0))
    return failed


def _tile_tables(listed, dev):
    """The tables of one decode over tiles.  listed: per tile (n, t, (y0, x0, a, b), first_sym, stream, None), or
    (n, t, (y0, x0, a, b), first_sym, segments, layers) where `layers` is the range of the tile's segments to read.
    -> ((tile table, segment table, blob on the device `dev`, its length), where): the blob is everything that is read, joined (one
    byte if that is nothing) and uploaded; a stream's place in it stands in its tile's row; a tile of segments has zeros there and
    len(segments) rows of the segment table, (0, 0) for those outside `layers`; where = [(n, t, y0, x0)] per row of the tile table."""
    tiles, segs, blobs, pos, where = [], [], [], 0, []
    for n, t, (y0, x0, a, b), first_sym, payload, layers in listed:
        where.append((n, t, y0, x0))
        if layers is None:
            tiles.append((y0, x0, a, b, pos, len(payload), first_sym, n))
            blobs.append(bytes(payload))
            pos += len(payload)
            continue
        tiles.append((y0, x0, a, b, 0, 0, first_sym, n))
        for g, seg in enumerate(payload):
            if g in layers:
                segs.append((pos, len(seg)))
                blobs.append(bytes(seg))
                pos += len(seg)
            else:
                segs.append((0, 0))
    data = torch.frombuffer(bytearray(b''.join(blobs)) or bytearray(1), dtype=torch.uint8).to(dev)
    return (_lib.tile_table(tiles), _lib.seg_table(segs), data, pos), where


def _cut(q, sym, shapes, offs, want, copy=False):
    """the flat q / symbols of the volumes `shapes` at the element offsets `offs` -> per volume what `want` asks for, as (C,h,w)
    views, or as copies"""
    def cut(buf):
        views = [buf[o:o + c * h * w].view(c, h, w) for (c, h, w), o in zip(shapes, offs)]
        return [v.clone() for v in views] if copy else views
    return cut(q) if want == 'q' else cut(sym) if want == 'symbols' else list(zip(cut(q), cut(sym)))


# -- host-side helpers of the reference's NumPy branch (reference code/probclass.py:268-292,341-351,367-387) --

class LayerSession(object):
    """decode_tiles_batch(tile_layers=...) that goes on where its last call stopped (PredictionNetwork.open_layers).
    The session owns, on the device, ONE workspace for all tiles of its volumes (one slot per tile: a chunk's slots would not outlive
    the chunk, so nothing is chunked -- a ValueError names both sizes if the workspace exceeds max_workspace_bytes), the symbols and q
    of all volumes, and on the host the number of layers every tile's slot holds.
    advance(volumes_segments, tile_layers, want): volumes_segments = [(streams, first_syms)] as decode_tiles_batch takes them (a third
    entry, the shape, is compared with the session's), tile_layers = [per volume [g_t per tile]], the leading layers of every tile
    that are there now.  One ic_pc_decode_tiles_batch_layers_resume_f32 launch decodes, per tile, the layers between what its slot
    holds and g_t (codec.resume_plan), one ic_pc_conceal_tiles_channels launch behind it rewrites every (tile, channel) at or above
    the tile's limit, and the call returns what decode_tiles_batch(tile_layers=...) returns for the same bytes: (per volume q /
    symbols / (q, symbols), copies, [per volume [(tile, layers_read, channels, reason)]]).
    Tiles with 0 layers are left out of the launch.  The entry ties a slot to the tile's index in the launch and to the launch's shape
    (number of tiles, largest tile), so a tile continues only while both are what they were when its slot was written and starts
    afresh otherwise: in a format-6 file, which stores layer 0 of all tiles first, the launches change shape only while layer 0
    arrives, when there is nothing to continue.  A tile whose status is not 0 is reported with reason 'decoder' and starts afresh in
    the next call, as does a tile that is given fewer layers than its slot holds.
    fronts=True (open_layers(front_ends=...)): the streams are front-layered (container format 8) and the launch is
    ic_pc_decode_tiles_batch_fronts_resume_f32, with its larger workspace; advance() then returns what
    decode_tiles_batch(front_ends=..., tile_layers=...) returns.  Everything else is the same object."""

    def __init__(self, pred, volumes_geometry, th, tw, layer_ends, max_workspace_bytes=1 << 31, fronts=False):
        from .codec import tile_grid, check_layer_ends
        self.pred = pred
        self.shapes = [tuple(int(v) for v in shape) for shape in volumes_geometry]
        if not self.shapes:
            raise ValueError('a session needs at least one volume')
        C = self.shapes[0][0]
        for n, shape in enumerate(self.shapes):
            if shape[0] != C:
                raise ValueError('volume {} has {} channels, volume 0 has {}'.format(n, shape[0], C))
        if pred.pc._k != 24:
            raise ValueError(_NEEDS_K24.format(pred.pc._k))
        self.ends = check_layer_ends(layer_ends, C)
        self.fronts = bool(fronts)
        self.mode = _tiles_mode('_fronts_resume' if self.fronts else '_layers_resume', C, 0, (pred.conceal_fallback(),), self.ends,
                                report='held')
        self.entry = self.mode.name
        self.th, self.tw = int(th), int(tw)
        self.grids = [tile_grid(h, w, self.th, self.tw) for _, h, w in self.shapes]
        self.vtable, self.offs, self.total = _lib.packed_volume_table(self.shapes)
        dev = pred.centers.device
        need = self.mode.size(C, max(a for grid in self.grids for _, _, a, _ in grid), max(b for grid in self.grids for _, _, _, b in grid),
                              sum(len(grid) for grid in self.grids), len(self.shapes), pred.pc._k)
        if need > int(max_workspace_bytes):
            raise ValueError('the session keeps one workspace slot per tile and cannot be chunked: {} tiles need {} bytes, '
                             'max_workspace_bytes is {}'.format(sum(len(grid) for grid in self.grids), need, int(max_workspace_bytes)))
        self.ws = torch.zeros(need, dtype=torch.uint8, device=dev)             # zero: no slot holds anything yet
        self.sym = torch.zeros(self.total, dtype=torch.int64, device=dev)
        self.q = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.done = [[0] * len(grid) for grid in self.grids]                   # layers the tile's slot holds
        self.place = [[None] * len(grid) for grid in self.grids]               # (index in the launch, shape of the launch) of that slot
        self.launches = 0

    def advance(self, volumes_segments, tile_layers, want='q'):
        from .codec import resume_plan
        pred, mode = self.pred, self.mode
        if want not in ('q', 'symbols', 'both'):
            raise ValueError("want is 'q', 'symbols' or 'both', got {!r}".format(want))
        if len(volumes_segments) != len(self.shapes) or len(tile_layers) != len(self.shapes):
            raise ValueError('{} volumes and {} rows of tile_layers for a session of {} volumes'.format(
                len(volumes_segments), len(tile_layers), len(self.shapes)))
        _, _, listed, missing, _ = _list_tiles(volumes_segments, self.th, self.tw, mode, tile_layers, (self.shapes, self.grids))
        dev = pred.centers.device
        centers = pred.centers.contiguous().float()
        for n, t in missing:                                                   # a tile that holds nothing now has no slot to continue in
            self.done[n][t], self.place[n][t] = 0, None
        failed = set()
        if listed:
            shape = (len(listed), max(cell[2] for _, _, cell, _, _, _ in listed), max(cell[3] for _, _, cell, _, _, _ in listed))
            reads, froms, limits = [], [], []
            for i, (n, t, cell, first, streams, layers) in enumerate(listed):
                have = self.done[n][t] if self.place[n][t] == (i, shape) else 0
                g_from, channels = resume_plan(have, len(layers), self.ends)
                reads.append((n, t, cell, first, streams, range(g_from, len(layers))))
                froms.append(g_from)
                limits.append(channels)
            need = mode.size(mode.C, shape[1], shape[2], shape[0], len(self.shapes), pred.pc._k)
            assert need <= self.ws.numel()
            tables, where = _tile_tables(reads, dev)
            status = torch.zeros(len(reads), dtype=torch.int32, device=dev)
            pred._launch_tiles(mode, tables, self.vtable, len(self.shapes), self.sym, self.q, status, self.ws, need, centers, 0, len(reads),
                               ((ctypes.c_int * len(froms))(*froms), (ctypes.c_int * len(limits))(*limits)))
            self.launches += 1
            failed = set(_failed_tiles(status, where, mode.report))
            for i, (n, t, _, _, _, layers) in enumerate(listed):
                self.done[n][t], self.place[n][t] = (0, None) if (n, t) in failed else (len(layers), (i, shape))
        held = pred._conceal_held(self.sym, self.q, self.shapes, self.grids, self.vtable, tile_layers, failed, self.ends, self.th, self.tw, centers)
        return _cut(self.q, self.sym, self.shapes, self.offs, want, copy=True), held


def pad_for_probclass3d(x, context_size, pad_value=0, learn_pad_var=False):
    """numpy CHW / NCHW or torch NCHW: constant-pad depth (front only), H and W by context_size // 2."""
    assert not learn_pad_var, 'learn_pad_var is not supported'
    pad = context_size // 2
    assert pad >= 1
    if isinstance(x, np.ndarray):
        if x.ndim == 3:
            return pad_for_probclass3d(x[None], context_size, pad_value)[0]
        pads = [[0, 0], [pad, 0], [pad, pad], [pad, pad]]
        return np.pad(x, pads, mode='constant', constant_values=pad_value)
    N, C, H, W = x.shape
    out = x.new_full((N, C + pad, H + 2 * pad, W + 2 * pad), float(pad_value))
    out[:, pad:, pad:pad + H, pad:pad + W] = x
    return out


def undo_pad_for_probclass3d(x, context_size):
    if isinstance(x, np.ndarray) and x.ndim == 3:
        return undo_pad_for_probclass3d(x[None], context_size)[0]
    pad = context_size // 2
    assert pad >= 1
    return x[:, pad:, pad:-pad, pad:-pad]


def _iter_block_idices(syms_shape, block_sizes):
    C, H, W = syms_shape
    bC, bH, bW = block_sizes
    for c, h, w in itertools.product(range(C - bC + 1), range(H - bH + 1), range(W - bW + 1)):
        yield slice(c, c + bC), slice(h, h + bH), slice(w, w + bW)


def iter_over_blocks(syms, block_sizes):
    """blocks of a CHW volume in raster order C, then H, then W fastest."""
    for cs, hs, ws in _iter_block_idices(syms.shape, block_sizes):
        yield syms[cs, hs, ws]


def num_blocks(syms_shape, block_sizes):
    C, H, W = syms_shape
    bC, bH, bW = block_sizes
    return max(C - bC + 1, 0) * max(H - bH + 1, 0) * max(W - bW + 1, 0)
