#!/usr/bin/env python
"""Writes tests/golden/pc_launches.json: what the tile coders of probclass.PredictionNetwork hand to the library for every case of
tests/pc_launch_cases.py, recorded against the fake binding of that module.  No device is needed.

REGENERATING THE FIXTURE says that the calls have changed: it is recorded from the code as it stands BEFORE a change to
probclass.py that is meant to leave the calls alone, and the test then holds the change to it.

    python tools/make_pc_launch_golden.py [--out PATH] [--force]

Everything is recorded twice and must agree."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import pc_launch_cases as P                       # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=P.PATH)
    ap.add_argument('--force', action='store_true', help='overwrite an existing fixture')
    flags = ap.parse_args(argv)
    if os.path.exists(flags.out) and not flags.force:
        sys.exit('{} exists: --force if the calls are meant to change'.format(flags.out))
    recorder = P.Recorder()
    kept = [(obj, name, getattr(obj, name)) for obj, name, _ in P.substitutions(recorder)]
    for obj, name, value in P.substitutions(recorder):
        setattr(obj, name, value)
    try:
        first, second = P.record_all(recorder), P.record_all(recorder)
    finally:
        for obj, name, value in kept:
            setattr(obj, name, value)
    data = json.dumps(first, separators=(',', ':')) + '\n'
    assert data == json.dumps(second, separators=(',', ':')) + '\n', 'two runs differ'
    assert len(data) <= P.MAX_BYTES, 'the fixture has {} bytes, the limit is {}'.format(len(data), P.MAX_BYTES)
    calls = [c.split('|')[0] for case in first['cases'].values() for c in case['calls']]
    os.makedirs(os.path.dirname(os.path.abspath(flags.out)), exist_ok=True)
    with open(flags.out, 'w') as f:
        f.write(data)
    print('wrote {}: {} bytes, {} cases, {} library calls over {} entries, {} refusal combinations with {} messages'.format(
        flags.out, len(data), len(first['cases']), len(calls), len(set(calls)), len(first['grid']['codes'].split()),
        len(first['grid']['messages']) - 1))


if __name__ == '__main__':
    main()
