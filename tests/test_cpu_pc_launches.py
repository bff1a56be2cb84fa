"""What PredictionNetwork's tile coders hand to the library, call by call, against tests/golden/pc_launches.json: the coders run on
the CPU against the recording stand-in of tests/pc_launch_cases.py (which also writes status words, symbols and coder bytes back),
so every scalar, every host table at the pointer a chunk was given, what is NULL, what comes back and every refusal is pinned.
The file was recorded before the host side of the tile coders was rewritten around one mode record, one listing and one launch."""
import json
import os

import pytest

from tests import pc_launch_cases as P

with open(P.PATH) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture()
def recorder(monkeypatch):
    rec = P.Recorder()
    for obj, name, value in P.substitutions(rec):
        monkeypatch.setattr(obj, name, value)
    return rec


@pytest.fixture(scope='module')
def networks():
    return P.prediction_network(24), P.prediction_network(17)


def test_golden_file():
    assert os.path.getsize(P.PATH) <= P.MAX_BYTES
    assert list(GOLDEN['cases']) == list(P.cases()), 'the cases of the module and of the golden file differ: see tools/make_pc_launch_golden.py'
    calls = [c.split('|')[0] for case in GOLDEN['cases'].values() for c in case['calls']]
    assert len(calls) >= 39 and len(set(calls)) >= 13
    assert set(calls) >= set(P.BATCH) | {'ic_pc_decode_tiles_f32', 'ic_pc_decode_f32', 'ic_pc_decode_channels_f32', 'ic_pc_encode_f32',
                                         'ic_pc_encode_segments_f32', 'ic_pc_conceal_tiles', 'ic_pc_conceal_tiles_channels'}


@pytest.mark.parametrize('name', list(GOLDEN['cases']))
def test_case(recorder, networks, name):
    call, script = P.cases()[name]
    got = P.run(recorder, lambda: call(*networks), script)
    want = GOLDEN['cases'][name]
    assert got['calls'] == want['calls']
    assert json.loads(json.dumps(got)) == want


def test_chunks_cut_inside_a_volume():
    """the budgets do what pc_launch_cases.budget says of them: launches of 3 and 2 tiles, and of 4 and 1, the latter cut inside a volume"""
    for mode in P.DECODE_MODES:
        for which, sizes in (('unlimited', [5]), ('two', [3, 2]), ('four', [4, 1])):
            calls = GOLDEN['cases']['decode/{}/both/{}'.format(mode, which)]['calls']
            assert [int(c.split('|')[1].split(',')[3]) for c in calls if c.split('|')[0] in P.BATCH] == sizes, (mode, which)
        assert GOLDEN['cases']['decode/{}/both/below'.format(mode)]['raises'] == 'ValueError', mode
    for which, sizes in (('unlimited', [6]), ('two', [3, 3]), ('four', [4, 2])):
        calls = GOLDEN['cases']['choose/per tile/symbols/{}/ok'.format(which)]['calls']
        assert [int(c.split('|')[1].split(',')[3]) for c in calls] == sizes, which


def test_refusal_grid(recorder, networks):
    messages, codes = P.refusal_grid(*networks)
    want = GOLDEN['grid']
    assert len(codes) == 2 * 4 * 2 ** 8
    assert [messages[c] for c in codes] == [want['messages'][int(c)] for c in want['codes'].split()]
