"""Fenced, poisoned device buffers for the kernel tests (helper module; tests/test_cpu_fenced.py is its self-test).

The caching allocator rounds every block up, so a store a few rows past a tensor lands in slack nobody looks at, and fresh memory
next to a tensor is mostly zero -- the padding value -- so a load past an input gives the right answer by luck.  fenced() puts a
view between two FENCE-byte zones of a known byte the test owns:

  inputs (float):        0xFF -- every float32 / float64 read from the fence is a NaN and poisons whatever it feeds
  outputs, workspaces:   0xA5 -- the codec tests' guard value; check_fences() asserts that every fence byte survived the call
  integer inputs:        cannot hold a NaN: the call is run with fences of 0x00 and of 0xFF, the outputs must be bit-identical

A workspace is handed over dirty: poison(ws, 0xFF) and poison(ws, 0x00), one run over each, the outputs bit-identical (bits()).
A new kernel test takes every device buffer from fenced(), and a new entry point gets a line in COVERAGE below.
"""
import numpy as np
import torch

FENCE = 65536          # bytes on each side; a multiple of 256, so the view keeps the alignment of a fresh allocation
IN_FENCE = 0xFF        # float inputs: NaN bit patterns
OUT_FENCE = 0xA5       # outputs and workspaces: the codec tests' GUARD
ZERO_FENCE = 0x00      # the second fill of integer inputs

def fenced(array_or_shape, dtype=torch.float32, device='cpu', fill=IN_FENCE, name=None):
    """dense view of the given shape (or holding a copy of the given array / tensor, converted to dtype) FENCE bytes into an
    allocation of FENCE + view + FENCE bytes whose fences hold `fill`.  A view made from a shape is an output or a workspace:
    floating ones are pre-filled with NaN (every element must be written), others with the fence byte."""
    src = None
    if isinstance(array_or_shape, (tuple, list, torch.Size)) and all(isinstance(v, (int, np.integer)) for v in array_or_shape):
        shape = tuple(int(v) for v in array_or_shape)
    elif isinstance(array_or_shape, (int, np.integer)):
        shape = (int(array_or_shape),)
    else:
        src = array_or_shape if torch.is_tensor(array_or_shape) else torch.as_tensor(np.ascontiguousarray(array_or_shape))
        shape = tuple(src.shape)
    numel = int(np.prod(shape, dtype=np.int64)) if shape else 1
    nbytes = numel * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((2 * FENCE + nbytes,), fill, dtype=torch.uint8, device=device)
    view = raw[FENCE:FENCE + nbytes].view(dtype).view(shape)
    if src is not None:
        view.copy_(src.to(dtype))
    elif dtype.is_floating_point:
        view.fill_(float('nan'))
    assert view.is_contiguous() and view.data_ptr() == raw.data_ptr() + FENCE
    view._fence = (raw, nbytes, fill, name or 'buffer {}'.format(shape))
    return view


def allocation(view):
    """the whole allocation behind a fenced view (uint8): both fences and the view"""
    return view._fence[0]


def refence(view, fill):
    """give an existing view other fence bytes (the two-fills runs of integer inputs)"""
    raw, nbytes, _, name = view._fence
    raw[:FENCE].fill_(fill)
    raw[FENCE + nbytes:].fill_(fill)
    view._fence = (raw, nbytes, fill, name)
    return view


def fence_damage(view):
    """[] if both fences of the view are intact, else one line per damaged side"""
    raw, nbytes, fill, name = view._fence
    out = []
    for side, zone, base in (('front', raw[:FENCE], -FENCE), ('back', raw[FENCE + nbytes:], nbytes)):
        bad = (zone != fill).nonzero().flatten()
        if bad.numel():
            out.append('{}: {} fence: {} bytes changed, first at byte {:+d}, last at byte {:+d} relative to the view ({} bytes long)'.format(
                name, side, int(bad.numel()), base + int(bad[0]), base + int(bad[-1]), nbytes))
    return out


def check_fences(*views):
    """every fence byte of every view is unchanged (call after torch.cuda.synchronize()); None entries are skipped"""
    damage = []
    for v in views:
        if v is not None:
            damage += fence_damage(v)
    assert not damage, 'store outside a buffer:\n  ' + '\n  '.join(damage)


def poison(workspace, byte):
    """fill a workspace view (or the part of one handed in) with one byte"""
    workspace.reshape(-1).view(torch.uint8).fill_(byte)
    return workspace


def bits(t):
    """integer reinterpretation, so torch.equal compares NaNs too"""
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    return t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def snapshot(*views):
    """copies of the whole allocations (fences included) of the views, for unchanged()"""
    return [allocation(v).clone() for v in views if v is not None]


def unchanged(snap, *views):
    """a refused call left views and fences byte for byte as they were"""
    views = [v for v in views if v is not None]
    assert len(snap) == len(views)
    for s, v in zip(snap, views):
        assert torch.equal(s, allocation(v)), '{} changed although the call was refused'.format(v._fence[3])


# ---------------------------------------------------------------------------------------------------------------------------
# coverage manifest: every entry point of _lib.PROTOTYPES is either exercised by tests/test_gpu_fenced_buffers.py ('fenced') or
# left out for one of four reasons.  tests/test_cpu_fenced.py holds the dict to PROTOTYPES, so a new entry forces a decision.
FENCED = 'fenced'
NO_DEVICE_POINTER = 'takes or returns no device pointer'
DEBUG_SETTER = 'debug or profiling setter'
PEER = 'peer-exchange entry: works on a region shared between processes'


def _codec(test_file):
    return 'codec entry: outputs and workspaces guarded by tests/' + test_file


ALLOWED_REASON_PREFIXES = (NO_DEVICE_POINTER, DEBUG_SETTER, 'codec entry: outputs and workspaces guarded by tests/test_gpu_codec', PEER)

COVERAGE = {
    'ic_abi_version': NO_DEVICE_POINTER,
    'ic_strerror': NO_DEVICE_POINTER,
    'ic_crc32c': NO_DEVICE_POINTER,                      # host bytes
    'ic_conv2d_bn_act_f32': FENCED,
    'ic_deconv2d_bn_act_f32': FENCED,
    'ic_conv3x3_c128_packed_floats': NO_DEVICE_POINTER,
    'ic_pack_conv3x3_c128_f32': FENCED,
    'ic_conv3x3_c128_bn_act_f32': FENCED,
    'ic_wino3x3_c128_packed_floats': NO_DEVICE_POINTER,
    'ic_pack_wino3x3_c128_f32': FENCED,
    'ic_pack_wino3x3_c128_batch_f32': FENCED,
    'ic_wino3x3_c128_bn_act_f32': FENCED,
    'ic_wino3x3_c128_workgroups': NO_DEVICE_POINTER,
    'ic_wino3x3_c128_plan': NO_DEVICE_POINTER,
    'ic_conv3x3_c128_both_packed_floats': NO_DEVICE_POINTER,
    'ic_pack_conv3x3_c128_both_f32': FENCED,
    'ic_conv3x3_c128_pick_algo': NO_DEVICE_POINTER,
    'ic_conv3x3_c128_auto_f32': FENCED,
    'ic_conv2d_mfma_packed_floats': NO_DEVICE_POINTER,
    'ic_pack_conv2d_mfma_f32': FENCED,
    'ic_conv2d_mfma_bn_act_f32': FENCED,
    'ic_quantize_f32': FENCED,
    'ic_heatmap_quantize_f32': FENCED,
    'ic_heatmap_quantize_cap_f32': FENCED,
    'ic_pc_workspace_bytes': NO_DEVICE_POINTER,
    'ic_pc_packed_floats': NO_DEVICE_POINTER,
    'ic_pc_mid_tile': NO_DEVICE_POINTER,
    'ic_pc_pack_filters_f32': FENCED,
    'ic_pc_logits_f32': FENCED,
    'ic_pc_logits_padded_f32': FENCED,
    'ic_pc_bitcost_f32': FENCED,
    'ic_pc_logits_to_freqs_f32': FENCED,
    'ic_pc_encode_capacity_bytes': NO_DEVICE_POINTER,
    'ic_pc_encode_f32': _codec('test_gpu_codec.py'),
    'ic_pc_decode_workspace_bytes': NO_DEVICE_POINTER,
    'ic_pc_decode_f32': _codec('test_gpu_codec_decoder.py'),
    'ic_pc_decode_tiles_workspace_bytes': NO_DEVICE_POINTER,
    'ic_pc_decode_tiles_f32': _codec('test_gpu_codec_tiled.py'),
    'ic_pc_decode_tiles_batch_workspace_bytes': NO_DEVICE_POINTER,
    'ic_pc_decode_tiles_batch_f32': _codec('test_gpu_codec_batch.py'),
    'ic_pc_decode_channels_f32': _codec('test_gpu_codec_preview.py'),
    'ic_pc_decode_tiles_batch_channels_f32': _codec('test_gpu_codec_preview.py'),
    'ic_pc_decode_tiles_batch_layers_workspace_bytes': NO_DEVICE_POINTER,
    'ic_pc_decode_tiles_batch_layers_f32': _codec('test_gpu_codec_layered.py'),
    'ic_pc_decode_tiles_batch_layers_pertile_workspace_bytes': NO_DEVICE_POINTER,
    'ic_pc_decode_tiles_batch_layers_pertile_f32': _codec('test_gpu_codec_recover.py'),
    'ic_pc_decode_tiles_batch_fronts_workspace_bytes': NO_DEVICE_POINTER,
    'ic_pc_decode_tiles_batch_fronts_f32': _codec('test_gpu_codec_fronts.py'),
    'ic_pc_decode_tiles_batch_fronts_pertile_workspace_bytes': NO_DEVICE_POINTER,
    'ic_pc_decode_tiles_batch_fronts_pertile_f32': _codec('test_gpu_codec_fronts.py'),
    'ic_pc_decode_tiles_batch_layers_resume_workspace_bytes': NO_DEVICE_POINTER,
    'ic_pc_decode_tiles_batch_layers_resume_f32': _codec('test_gpu_codec_resume.py'),
    'ic_pc_decode_tiles_batch_fronts_resume_workspace_bytes': NO_DEVICE_POINTER,
    'ic_pc_decode_tiles_batch_fronts_resume_f32': _codec('test_gpu_codec_fronts_resume.py'),
    'ic_pc_encode_segments_f32': _codec('test_gpu_codec_layered.py'),
    'ic_pc_conceal_tiles_workspace_bytes': NO_DEVICE_POINTER,
    'ic_pc_conceal_tiles': _codec('test_gpu_codec_checked.py'),
    'ic_pc_conceal_tiles_channels_workspace_bytes': NO_DEVICE_POINTER,
    'ic_pc_conceal_tiles_channels': _codec('test_gpu_codec_recover.py'),
    'ic_sum_f32': FENCED,
    'ic_mean_f32': FENCED,
    'ic_mean_rows_f32': FENCED,
    'ic_ae_workspace_bytes': NO_DEVICE_POINTER,
    'ic_ae_sync_pos_bytes': NO_DEVICE_POINTER,
    'ic_ae_res_stack_sync_pos_bytes': NO_DEVICE_POINTER,
    'ic_ae_encode_f32': FENCED,
    'ic_ae_encode_cap_f32': FENCED,
    'ic_ae_decode_f32': FENCED,
    'ic_ae_res_stack_workspace_bytes': NO_DEVICE_POINTER,
    'ic_ae_res_stack_f32': FENCED,
    'ic_peer_region_bytes': NO_DEVICE_POINTER,
    'ic_peer_max_values': NO_DEVICE_POINTER,
    'ic_peer_max_world': NO_DEVICE_POINTER,
    'ic_peer_region_create': PEER,
    'ic_peer_region_open': PEER,
    'ic_peer_region_close': PEER,
    'ic_peer_region_destroy': PEER,
    'ic_peer_allreduce_f64': PEER,
    'ic_peer_allreduce_f64_bounded': PEER,
    'ic_build_has_tuning_forms': NO_DEVICE_POINTER,
    'ic_conv3x3_c128_pick_form': NO_DEVICE_POINTER,
    'ic_wino4_3x3_c128_packed_floats': NO_DEVICE_POINTER,
    'ic_pack_wino4_3x3_c128_f32': FENCED,
    'ic_pack_wino4_3x3_c128_batch_f32': FENCED,
    'ic_wino4_3x3_c128_supported': NO_DEVICE_POINTER,
    'ic_wino4_3x3_c128_workgroups': NO_DEVICE_POINTER,
    'ic_wino4_3x3_c128_waves': NO_DEVICE_POINTER,
    'ic_wino4_3x3_c128_bn_act_f32': FENCED,
    'ic_wino4_3x3_c128_stats_parts': NO_DEVICE_POINTER,
    'ic_wino4_3x3_c128_raw_stats_f32': FENCED,
    'ic_wino4_conv5s2_packed_floats': NO_DEVICE_POINTER,
    'ic_pack_wino4_conv5s2_f32': FENCED,
    'ic_wino4_conv5s2_supported': NO_DEVICE_POINTER,
    'ic_wino4_conv5s2_workgroups': NO_DEVICE_POINTER,
    'ic_wino4_conv5s2_c64_c128_bn_act_f32': FENCED,
    'ic_wino4_deconv5s2_c128_c64_bn_act_f32': FENCED,
    'ic_val_metrics_workspace_bytes': NO_DEVICE_POINTER,
    'ic_val_metrics_u8_f64': FENCED,
    'ic_val_metrics_per_image_u8_f64': FENCED,
    'ic_space_to_depth2_f32': FENCED,
    'ic_conv5s2_both_packed_floats': NO_DEVICE_POINTER,
    'ic_pack_conv5s2_both_f32': FENCED,
    'ic_msssim_plan_bytes': NO_DEVICE_POINTER,
    'ic_msssim_plan_fill': FENCED,
    'ic_msssim_workspace_bytes': NO_DEVICE_POINTER,
    'ic_msssim_loss_grad_f32': FENCED,
    'ic_bn_workspace_bytes': NO_DEVICE_POINTER,
    'ic_bn_stats_f32': FENCED,
    'ic_bn_train_stats_f32': FENCED,
    'ic_bn_train_forward_f32': FENCED,
    'ic_bn_train_forward_cstats_f32': FENCED,
    'ic_bn_moments_f32': FENCED,
    'ic_bn_train_fold_moments_f32': FENCED,
    'ic_bn_backward_reduce_f32': FENCED,
    'ic_bn_backward_apply_f32': FENCED,
    'ic_bn_apply_f32': FENCED,
    'ic_bn_backward_f32': FENCED,
    'ic_conv2d_wgrad_workspace_bytes': NO_DEVICE_POINTER,
    'ic_conv2d_wgrad_f32': FENCED,
    'ic_conv3x3_c128_wgrad_workspace_bytes': NO_DEVICE_POINTER,
    'ic_conv3x3_c128_wgrad_f32': FENCED,
    'ic_pack_conv3x3_c128_bwd_f32': FENCED,
    'ic_heatmap_quantize_bwd_workspace_bytes': NO_DEVICE_POINTER,
    'ic_heatmap_quantize_bwd_f32': FENCED,
    'ic_pc_dlogits_f32': FENCED,
    'ic_pc_bwd_data_workspace_bytes': NO_DEVICE_POINTER,
    'ic_pc_bwd_data_f32': FENCED,
    'ic_pc_wgrad_workspace_bytes': NO_DEVICE_POINTER,
    'ic_pc_wgrad_f32': FENCED,
    'ic_channel_sum_workspace_bytes': NO_DEVICE_POINTER,
    'ic_channel_sum_f32': FENCED,
    'ic_adam_tf_f32': FENCED,
    'ic_stream_create_cu_range': NO_DEVICE_POINTER,      # stream handle
    'ic_stream_destroy': NO_DEVICE_POINTER,
    'ic_event_create': NO_DEVICE_POINTER,                # event handles
    'ic_event_destroy': NO_DEVICE_POINTER,
    'ic_event_record': NO_DEVICE_POINTER,
    'ic_event_elapsed_ms': NO_DEVICE_POINTER,
}
