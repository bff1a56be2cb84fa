"""Transcoding, the host side (no GPU): the symbol rule of an integer cap, budget_search over another number of steps, the command
line's refusals."""
import argparse
import math
import struct

import numpy as np
import pytest

from imgcomp_cvpr_amd import codec


# ---- the rule -----------------------------------------------------------------------------------------------------------------

C, SH, SW, FILL = 6, 5, 7, 2


def _volume(seed):
    return np.random.RandomState(seed).randint(0, 6, size=(C, SH, SW)).astype(np.int64)


def _loop_rule(sym, plane, fill):
    out = np.empty_like(sym)
    for c in range(sym.shape[0]):
        for y in range(sym.shape[1]):
            for x in range(sym.shape[2]):
                out[c, y, x] = sym[c, y, x] if c < plane[y, x] else fill
    return out


def test_cap_symbols_against_the_loop():
    rs = np.random.RandomState(3)
    pool = np.array([0, 1, 2, 3, 4, 5, 6, 7, 6.5, 100, np.inf])                   # integers in [0, C]; anything at or above C
    for seed in range(6):
        sym = _volume(seed)
        plane = rs.choice(pool, size=(SH, SW))
        for p in (plane, plane.astype(np.float32), np.minimum(plane, 50).astype(np.int64)):
            got = codec.cap_symbols(sym, p, FILL)
            assert got.dtype == sym.dtype and got is not sym
            assert np.array_equal(got, _loop_rule(sym, p, FILL)), seed
        assert np.array_equal(sym, _volume(seed))                                 # the argument is left as it was
        assert np.array_equal(codec.cap_channels(plane, C), np.minimum(plane, C).astype(np.int64))


@pytest.mark.parametrize('K', [0, 1, C - 1, C, C + 1, np.inf])
def test_constant_plane_is_a_preview(K):
    sym = _volume(11)
    got = codec.cap_symbols(sym, np.full((SH, SW), K), FILL)
    assert np.array_equal(got, codec.preview_symbols(sym, min(K, C), FILL))
    if K >= C:
        assert np.array_equal(got, sym)
    # cap_plane builds the planes: H, W of the header, then the integer check
    plane = codec.cap_plane(SH * 8 - 3, SW * 8, 8, level=None if K == np.inf else K)
    assert np.array_equal(codec.cap_symbols(sym, plane, FILL), got)


@pytest.mark.parametrize('plane,words', [
    (np.full((SH, SW), 2.5), ('2.5', 'fractional cap rescales z', 'bottleneck', 'compress')),
    (np.where(np.eye(SH, SW) > 0, 0.125, 3.0), ('0.125', 'bottleneck')),
    (np.full((SH, SW), -1.0), ('not in [0, +inf]',)),
    (np.full((SH, SW), np.nan), ('not in [0, +inf]',)),
    (np.where(np.eye(SH, SW) > 0, np.nan, 3.0), ('not in [0, +inf]',)),
    (np.full((SH, SW + 1), 3.0), ('shape',)),
    (np.full((SW, SH), 3.0), ('shape',)),
    (np.full((SH * SW,), 3.0), ('shape',)),
    (3.0, ('shape',)),
])
def test_cap_symbols_refusals(plane, words):
    with pytest.raises(ValueError) as e:
        codec.cap_symbols(_volume(1), plane, FILL)
    for word in words:
        assert word in str(e.value), str(e.value)


def test_cap_symbols_wants_a_volume():
    with pytest.raises(ValueError):
        codec.cap_symbols(np.zeros((SH, SW), np.int64), np.full((SH, SW), 1), FILL)


# ---- budget_search(steps=S) ---------------------------------------------------------------------------------------------------

def _run(table, estimate, S):
    calls = []

    def fits(k):
        assert 0 <= k <= S
        calls.append(k)
        return bool(table[k])

    k, probes = codec.budget_search(fits, estimate, steps=S)
    bound = 1 + 2 + 1 + int(math.ceil(math.log2(S)))
    assert probes == len(calls) <= bound, (S, estimate, calls)
    assert len(set(calls)) == len(calls), (S, estimate, calls)                    # no index coded twice
    assert k in calls and table[k], (S, estimate, k, calls)                       # fits(k) was established by a call ..
    assert k == S or (k + 1 in calls and not table[k + 1]), (S, estimate, k, calls)   # .. and so was not fits(k + 1)
    assert calls[0] == S
    return k, calls


@pytest.mark.parametrize('S', [1, 2, 32, 64])
def test_budget_search_steps(S):
    rs = np.random.RandomState(100 + S)
    tables = [list(rs.rand(S + 1) < p) for p in (0.1, 0.3, 0.5, 0.7, 0.9) for _ in range(4)]
    tables += [[k % 2 == 0 for k in range(S + 1)], [k <= S // 3 for k in range(S + 1)], [True] * (S + 1)]
    for table in tables:
        table[0] = True                                                           # (level 0 fits: the search has an answer)
        for estimate in list(range(S + 1)) + [-3, 10 * S]:
            k, calls = _run(table, estimate, S)
            if table[S]:
                assert k == S and calls == [S]
    for estimate in range(S + 1):                                                 # nothing fits: level 0 was asked, and no index twice
        calls = []
        with pytest.raises(ValueError) as e:
            codec.budget_search(lambda k: calls.append(k) or False, estimate, steps=S)
        assert 'smallest file' in str(e.value) and 0 in calls and len(set(calls)) == len(calls)
        assert len(calls) <= 1 + 2 + 1 + int(math.ceil(math.log2(S)))
    for threshold in range(S + 1):                                                # monotone: the threshold is found
        table = [k <= threshold for k in range(S + 1)]
        for estimate in range(S + 1):
            assert _run(table, estimate, S)[0] == threshold


def test_budget_search_refuses_no_steps():
    for S in (0, -1):
        with pytest.raises(ValueError):
            codec.budget_search(lambda k: True, 0, steps=S)


# the probe order of the function as it was before it took `steps` (recorded from it): the default is that function
RECORDED = [
    (lambda k: k <= 77, 60, 77, [256, 60, 61, 158, 109, 85, 73, 79, 76, 77, 78]),
    (lambda k: k <= 77, 77, 77, [256, 77, 78]),
    (lambda k: k <= 200, 0, 200, [256, 0, 1, 128, 192, 224, 208, 200, 204, 202, 201]),
    (lambda k: k % 2 == 0 and k < 256, 131, 62, [256, 131, 0, 65, 32, 48, 56, 60, 62, 63]),
    (lambda k: k < 40 or 100 < k < 130, 120, 129, [256, 120, 121, 188, 154, 137, 129, 133, 131, 130]),
    (lambda k: k == 0, 255, 0, [256, 255, 0, 127, 63, 31, 15, 7, 3, 1]),
    (lambda k: True, 5, 256, [256]),
]


def test_budget_search_default_is_unchanged():
    for fits, estimate, want, sequence in RECORDED:
        for kw in ({}, {'steps': codec.CAP_STEPS}):
            calls = []
            assert codec.budget_search(lambda k: calls.append(k) or fits(k), estimate, **kw) == (want, len(sequence))
            assert calls == sequence
    with pytest.raises(ValueError) as e:
        codec.budget_search(lambda k: False, 9)
    assert str(e.value) == 'no level fits: the smallest file, at level 0, is over the budget in bytes'


# ---- the command line ---------------------------------------------------------------------------------------------------------

def _flags(command='transcode', **kw):
    base = dict(command=command, tile=None, checked=False, wavefront=False, salvage=False, channels=None, layers=None, progressive=False,
                front_layers=None, front_progressive=False, partial=False, recover=False, chunk=None, fronts=False,
                cap=None, roi=None, background=None, max_bytes=None, bpp=None)
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.mark.parametrize('kw,words', [
    (dict(channels=8), ('--channels belongs to decompress',)),
    (dict(command='transcode-dir', channels=8), ('--channels belongs to decompress',)),
    (dict(partial=True), ('--partial belongs to decompress',)),
    (dict(command='transcode-dir', partial=True), ('--partial belongs to decompress',)),
    (dict(chunk=100), ('--chunk belongs to stream',)),
    (dict(command='transcode-dir', chunk=100), ('--chunk belongs to stream',)),
    (dict(fronts=True), ('--fronts belongs to stream',)),
    (dict(command='transcode-dir', fronts=True), ('--fronts belongs to stream',)),
    (dict(cap=2.5), ('--cap 2.5 is not an integer', 'bottleneck')),
    (dict(command='transcode-dir', cap=0.125), ('--cap 0.125 is not an integer',)),
    (dict(cap=4.0, roi=['0,0,8,8'], background=1.5), ('--background 1.5 is not an integer',)),
    (dict(cap=-1.0), ('--cap', 'not in [0, +inf]')),
    (dict(cap=float('nan')), ('--cap', 'not in [0, +inf]')),
    (dict(command='transcode-dir', roi=['0,0,8,8'], background=1.0), ('--roi belongs to compress / transcode',)),
    (dict(roi=['0,0,8,8']), ('--roi needs --background or a budget',)),
    (dict(background=1.0), ('--background needs --roi',)),
    (dict(cap=4.0, max_bytes=1000), ('--cap does not go with --max-bytes',)),
    (dict(max_bytes=1000, bpp=0.5), ('--max-bytes does not go with --bpp',)),
    (dict(max_bytes=0), ('--max-bytes 0 is not at least 1',)),
    (dict(checked=True), ('--checked needs --tile',)),
    (dict(wavefront=True), ('--wavefront needs --tile',)),
    (dict(progressive=True), ('--progressive needs --tile',)),
    (dict(front_layers='4,8'), ('--front-layers needs --tile',)),
    (dict(tile=128, progressive=True, front_progressive=True), ('--front-progressive does not go with --progressive',)),
    (dict(tile=128, wavefront=True, layers='4,32'), ('--layers does not go with --wavefront',)),
    (dict(salvage=True, recover=True), ('--recover does not go with --salvage',)),
    (dict(salvage=True, max_bytes=1000), ('--salvage does not go with',)),
    (dict(recover=True, roi=['0,0,8,8'], background=1.0), ('--recover does not go with',)),
])
def test_cli_refusals(kw, words):
    with pytest.raises(ValueError) as e:
        codec.check_option_args(_flags(**kw))
    for word in words:
        assert word in str(e.value), str(e.value)


def test_cli_accepted():
    for command in ('transcode', 'transcode-dir'):
        for kw in (dict(), dict(cap=4.0), dict(cap=0.0), dict(cap=float('inf')), dict(max_bytes=1000), dict(bpp=0.25),
                   dict(tile=128), dict(tile=128, checked=True), dict(tile=128, wavefront=True), dict(tile=128, layers='4,8,16,32'),
                   dict(tile=128, progressive=True), dict(tile=128, front_layers='4,32'), dict(tile=128, front_progressive=True, cap=8.0),
                   dict(tile=128, checked=True, max_bytes=900), dict(salvage=True), dict(recover=True), dict(salvage=True, cap=4.0),
                   dict(tile=128, progressive=True, recover=True)):
            codec.check_option_args(_flags(command, **kw))
    for kw in (dict(roi=['0,0,8,8'], background=1.0), dict(cap=8.0, roi=['0,0,8,8', '9,9,1,1'], background=2.0),
               dict(roi=['0,0,8,8'], max_bytes=1000), dict(roi=['0,0,8,8'], bpp=0.5)):
        codec.check_option_args(_flags('transcode', **kw))
    # command lines from before the options
    codec.check_option_args(argparse.Namespace(command='transcode', tile=None))
    codec.check_option_args(argparse.Namespace(command='transcode-dir', tile=None))
    codec.check_option_args(argparse.Namespace(command='decompress', tile=None))
    codec.check_option_args(argparse.Namespace(command='compress', tile=128, checked=True))


def test_the_old_commands_keep_their_sentences():
    for kw, sentence in (
            (dict(command='decompress', cap=4.0), "--cap belongs to compress / compress-dir: the cap on the importance map is the encoder's, a file is read without it"),
            (dict(command='compress-dir', roi=['0,0,8,8'], background=1.0), '--roi belongs to compress: a rectangle is in the pixels of one image'),
            (dict(command='decompress', roi=['0,0,8,8']), "--roi belongs to compress: the cap on the importance map is the encoder's, a file is read without it"),
            (dict(command='decompress', checked=True), '--checked belongs to compress / compress-dir: a file says by itself what it is'),
            (dict(command='compress', salvage=True), '--salvage belongs to decompress / decompress-dir'),
            (dict(command='stream', tile=128), '--tile belongs to compress / compress-dir: a file says by itself how it is tiled')):
        with pytest.raises(ValueError) as e:
            codec.check_option_args(_flags(**kw))
        assert str(e.value) == sentence
    codec.check_option_args(_flags('compress', cap=2.5))                          # a fractional cap is compress's, as before


def test_dir_jobs_and_dir_args(tmp_path):
    src, dst = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    for name in ('b.icf', 'a.ICF', 'c.png', 'd.txt'):
        (src / name).write_bytes(b'x')
    jobs = [(str(src / 'a.ICF'), str(dst / 'a.icf')), (str(src / 'b.icf'), str(dst / 'b.icf'))]
    assert codec.list_dir_jobs(str(src), str(dst), 'transcode-dir') == jobs
    assert codec.check_dir_args(_flags('transcode-dir', batch=8, input=str(src), output=str(dst)), 8) == (jobs, None)
    assert codec.check_dir_args(_flags('transcode-dir', batch=8, input=str(src), output=str(dst), tile=128, checked=True), 8) == (jobs, (16, 16))
    with pytest.raises(ValueError) as e:
        codec.check_dir_args(_flags('transcode-dir', batch=8, input=str(src), output=str(dst), tile=100), 8)
    assert 'multiple of the subsampling factor' in str(e.value)
    with pytest.raises(ValueError) as e:
        codec.check_dir_args(_flags('decompress-dir', batch=8, input=str(src), output=str(dst), tile=128), 8)
    assert str(e.value) == '--tile belongs to compress / compress-dir: a file says by itself how it is tiled'
    empty = tmp_path / 'empty'
    empty.mkdir()
    with pytest.raises(ValueError) as e:
        codec.list_dir_jobs(str(empty), str(dst), 'transcode-dir')
    assert '*.icf' in str(e.value)


def test_the_command_line_refuses_before_a_model_is_built(tmp_path, capsys):
    src = tmp_path / 'a.icf'
    src.write_bytes(b'x')
    for args, word in ((['transcode', str(src), str(tmp_path / 'b.icf'), '--cap', '2.5'], '--cap 2.5 is not an integer'),
                       (['transcode', str(src), str(tmp_path / 'b.icf'), '--channels', '4'], '--channels belongs to decompress'),
                       (['transcode-dir', str(tmp_path), str(tmp_path / 'out'), '--roi', '0,0,8,8', '--background', '1'], '--roi belongs to compress / transcode'),
                       (['transcode-dir', str(tmp_path), str(tmp_path / 'out'), '--background', '1.5', '--roi', '0,0,8,8'], '--roi belongs')):
        assert codec.main(args + ['--device', 'cuda:7']) == 2                     # (no such device is ever opened)
        assert word in capsys.readouterr().err
    assert not (tmp_path / 'b.icf').exists() and not (tmp_path / 'out').exists()


def test_the_calls_refuse_before_a_device():
    """an object without model or device gets as far as the parser: transcode and its kin read the file first"""
    c = object.__new__(codec.Codec)
    c.tile, c.checked, c.order, c.layers, c.front_layers = None, False, 'raster', None, None
    for call in (lambda: c.transcode(b''), lambda: c.transcode_to_budget(b'', 100), lambda: c.transcode(b'ICVF' + bytes(80))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match=r'^file 0: truncated file'):
        c.transcode_many([b'', b''])
    with pytest.raises(ValueError, match='caps: 1 entries for 2 files'):
        c.transcode_many([b'', b''], caps=[None])
    with pytest.raises(ValueError, match='truncated file'):
        c.repair(b'')
    for version in (1, 2):                                                        # no checksums to repair by: salvage's sentence
        with pytest.raises(ValueError) as e:
            c.repair(b'ICVF' + struct.pack('<H', version) + bytes(80))
        with pytest.raises(ValueError) as want:
            codec.parse_salvage(b'ICVF' + struct.pack('<H', version) + bytes(80))
        assert str(e.value) == str(want.value) and 'has nothing to salvage with' in str(e.value)
    c.tile, c.checked = None, True                                                # the target's refusals come first
    with pytest.raises(ValueError, match='checked=True needs a tile extent'):
        c.transcode(b'')
