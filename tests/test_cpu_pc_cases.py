"""The cases of tests/pc_cases.py are what tests/test_gpu_pc_forward.py takes them for (no GPU: the float64 oracle and the host
side of the library).  The conditions below are conditions on the INPUTS: a group that misses one gets another calibration
volume or seed, never a weaker condition."""
import math

import numpy as np
import pytest
import torch

from tests import pc_cases as P


@pytest.mark.parametrize('k,L', P.GROUPS)
def test_every_channel_is_live_and_every_symbol_a_target(k, L):
    """pooled over all volumes of the group: every output channel of res1/conv1 and of the final layer is positive at 10 % or
    more of the positions and clamped at 10 % or more (measured: 0.11 .. 0.88); every conv0 channel is positive somewhere and
    clamped somewhere (its input is mostly padding on volumes this small, so its shares stay skewed: 0.004 .. 0.99); every
    symbol 0 .. L - 1 is the target somewhere."""
    live, seen = P.liveness(k, L)
    for layer in ('conv1', 'final'):
        pos, neg = live[layer]
        assert pos.shape == ((k if layer == 'conv1' else L),)
        assert pos.min() >= 0.10 and neg.min() >= 0.10, (k, L, layer, pos.min(), neg.min())
    pos, neg = live['conv0']
    assert pos.shape == (k,) and pos.min() > 0 and neg.min() > 0
    assert seen == set(range(L))


def test_recentring_moves_three_biases_and_nothing_else():
    from imgcomp_cvpr_amd import weights as W
    for k, L in ((24, 6), (20, 11)):
        plain, wts = W.synthetic_weights(*P.configs(k, L)), P.weights(k, L)
        moved = {P.SCOPES[l] + '/biases' for l in P.RELU_LAYERS}
        assert set(wts) == {P.CENTERS} | {n for n in plain if n.startswith(P.PC + '/')}
        for n, a in wts.items():
            assert a.dtype == np.float32 and a.shape == plain[n].shape
            assert np.array_equal(a, plain[n]) != (n in moved), n
        assert P.weights(k, L) is wts                                 # one set per session: the references are computed on it


def test_volumes_reach_every_middle_tile_by_the_library_query():
    """ic_pc_mid_tile is host arithmetic (launch_pc_mfma calls it): the k = 24 list reaches 8 x 16, 5 x 25 and 6 x 21 in both
    middle layers, the picks are the ones the table states, k = 64 has its one tile and the VALU widths none."""
    from imgcomp_cvpr_amd import _lib
    mid = _lib.lib.ic_pc_mid_tile
    for k in (24, 64, 8, 20):
        for (N, C, h, w), tiles in P.volumes(k).items():
            assert (mid(k, h + 4, w + 4), mid(k, h + 2, w + 2)) == tiles, (k, (N, C, h, w))
    for layer in (0, 1):
        assert {t[layer] for t in P.K24_VOLUMES.values()} == {0, 1, 2}
    assert mid(24, 68, 100) == 1 and mid(24, 8, 16) == 0 and mid(24, 6, 21) == 2      # a Kodak volume's layer 1: 5 x 25
    assert mid(24, 10, 25) == 1 and mid(24, 12, 21) == 2 and mid(24, 16, 400) == 0
    assert mid(24, 5, 5) == 0 and mid(24, 4, 40) == 1                                  # ties go to the first shape of the table
    assert mid(64, 68, 100) == 3 and mid(12, 8, 16) == -1 and mid(24, 0, 16) == -1 and mid(24, 8, -1) == -1
    for k, L in P.VALU_GROUPS:
        assert _lib.lib.ic_pc_packed_floats(k, L) == 0
    for k, L in P.MFMA_GROUPS:
        assert _lib.lib.ic_pc_packed_floats(k, L) > 0


@pytest.mark.parametrize('k,L', P.EDGE_GROUPS)
def test_epilogue_edge_cases_are_edges(k, L):
    """far apart: somewhere the float64 logits spread over more than 90 (expf(-90) = 8e-40 is below the smallest normal float) and
    some target costs over 100 bits; all clamped: every logit is 0 and every symbol costs log2(L) bits"""
    bits, logits = P.reference_with(P.far_apart_weights(k, L), k, L, P.EDGE_VOLUME)
    assert float((logits.max(-1).values - logits.min(-1).values).max()) > 90
    assert float(bits.max()) > 100 and bool(torch.isfinite(bits).all())
    bits, logits = P.reference_with(P.all_clamped_weights(k, L), k, L, P.EDGE_VOLUME)
    assert not bool(logits.any())
    assert float((bits - math.log2(L)).abs().max()) < 1e-12
