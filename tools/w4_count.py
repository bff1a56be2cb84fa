#!/usr/bin/env python
"""Static instruction count of the F(4x4) 3x3 kernel per wave, from gfx950 assembly (CPU only: hipcc cross-compiles).

  hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-slp-vectorize --cuda-device-only -S imgcomp_cvpr_amd/csrc/conv3x3_wino4.hip -o w4.s
  python tools/w4_count.py w4.s [--kernel REGEX] [--all]

(`make -C imgcomp_cvpr_amd/csrc` leaves the same assembly as csrc/conv3x3_wino4.audit.s.)

Every instantiation of wino4_3x3_kernel is cut into basic blocks and each block's instructions are counted by class: MFMA, other
vector (`v_*`), LDS (`ds_*`), memory (`buffer_*`, `global_*`, `scratch_*`, `flat_*`) and scalar (`s_*`).  A block is weighted by how
often a wave runs it: the blocks of the k loop (the backward branch whose body holds MFMAs) by the loop's trip count, everything else
by 1.  The trip count is not in the assembly; it follows from the MFMAs a wave must issue, 9 x CIN: trips = (9 CIN - MFMAs outside the
loop) / MFMAs of one pass.  Other loops (the next layer's filter prefetch, the 8-wave form's counter polls) count as one pass.  In the
8-wave form a wave skips its transform slices behind scalar branches in every other iteration; the count takes every block of the loop
body, i.e. the transforming iteration.

The vector instructions that are not MFMAs are broken down further: accumulator-file moves (`v_accvgpr_*`), plain moves, DPP moves,
selects, integer adds / shifts (address arithmetic), and the rest (the transforms' floating-point arithmetic, conversions, compares).
Default output: the Kodak instantiation <WT=1, RES=1, 128, 128, SHUF=0, SEG2=0, WG8=0, STATS=0>; --all: one line per instantiation."""
import argparse
import re
import sys

NAME = re.compile(r'wino4_3x3_kernelILb(\d)ELi(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E')
KODAK = r'wino4_3x3_kernelILb1ELi1ELi128ELi128ELb0ELb0ELb0ELb0E'
CLASSES = ['mfma', 'vector', 'lds', 'memory', 'scalar']
VKINDS = ['accvgpr', 'mov', 'dpp', 'select', 'int', 'arith']


def kernels(path):
    """name -> list of instructions and labels"""
    name, body = None, None
    for ln in open(path):
        m = re.match(r'^([A-Za-z_][\w$.]*):', ln)
        if m and not ln.startswith('.L'):
            name, body = m.group(1), []
            continue
        if ln.startswith('.Lfunc_end') and body is not None:
            yield name, body
            name, body = None, None
            continue
        if body is None:
            continue
        s = ln.split(';')[0].strip()
        if not s or (s.startswith('.') and not s.endswith(':')):
            continue
        body.append(s)


def classify(s):
    op = s.split()[0]
    if op.startswith(('v_mfma', 'v_smfmac')):
        return 'mfma', None
    if op.startswith('v_'):
        if op.startswith('v_accvgpr'):
            return 'vector', 'accvgpr'
        if 'row_sh' in s or 'quad_perm' in s or 'row_bcast' in s or op.endswith('_dpp'):
            return 'vector', 'dpp'
        if op.startswith('v_mov') or op.startswith('v_readfirstlane') or op.startswith('v_readlane') or op.startswith('v_writelane'):
            return 'vector', 'mov'
        if op.startswith('v_cndmask'):
            return 'vector', 'select'
        if re.match(r'v_(add|sub|subrev|mul|mad|lshl|lshr|ashr|and|or|xor|bfe|mbcnt|add3|lshl_add|lshl_or|and_or|min|max)_?\w*[ui](16|24|32|64)', op) \
                or op.startswith(('v_mbcnt', 'v_add3_u32', 'v_lshl_add', 'v_lshl_or', 'v_and_or', 'v_mad_u', 'v_mad_i', 'v_mul_lo', 'v_mul_hi', 'v_lshlrev', 'v_lshrrev',
                                  'v_ashrrev', 'v_and_b', 'v_or_b', 'v_xor_b', 'v_or3', 'v_bfe', 'v_bfi', 'v_not_b')):
            return 'vector', 'int'
        return 'vector', 'arith'
    if op.startswith('ds_'):
        return 'lds', None
    if op.startswith(('buffer_', 'global_', 'scratch_', 'flat_')):
        return 'memory', None
    return 'scalar', None


def blocks_of(body):
    """[(label or None, [instructions])]: a block ends at a label or behind a branch"""
    out, cur, lab = [], [], None
    for s in body:
        if s.endswith(':'):
            if cur or lab is not None:
                out.append((lab, cur))
            cur, lab = [], s[:-1]
            continue
        cur.append(s)
        if s.startswith(('s_cbranch', 's_branch', 's_endpgm')):
            out.append((lab, cur))
            cur, lab = [], None
    if cur or lab is not None:
        out.append((lab, cur))
    return out


def tally(instrs):
    c = {k: 0 for k in CLASSES}
    v = {k: 0 for k in VKINDS}
    for s in instrs:
        cls, kind = classify(s)
        c[cls] += 1
        if kind:
            v[kind] += 1
    return c, v


def add(a, b, w=1):
    for k in b:
        a[k] = a.get(k, 0) + w * b[k]


def count_kernel(name, body):
    m = NAME.search(name)
    cin = int(m.group(3))
    bl = blocks_of(body)
    labels = {lab: i for i, (lab, _) in enumerate(bl) if lab is not None}
    per = [tally(ins) for _, ins in bl]
    # the k loop: the widest backward branch whose body holds MFMAs
    loop = None
    for i, (_, ins) in enumerate(bl):
        if not ins:
            continue
        op, _, tgt = ins[-1].partition(' ')
        tgt = tgt.strip()
        if op.startswith(('s_cbranch', 's_branch')) and tgt in labels and labels[tgt] <= i:
            n = sum(per[j][0]['mfma'] for j in range(labels[tgt], i + 1))
            if n and (loop is None or n > loop[2]):
                loop = (labels[tgt], i, n)
    total_mfma = sum(p[0]['mfma'] for p in per)
    need = 9 * cin
    if loop:
        outside = total_mfma - loop[2]
        assert (need - outside) % loop[2] == 0, (name, need, outside, loop[2])
        trips = (need - outside) // loop[2]
    else:
        assert total_mfma == need, (name, total_mfma, need)
        trips, loop = 1, (len(bl), len(bl) - 1, 0)
    parts = {}
    for part, rng, w in (('before the loop', range(0, loop[0]), 1), ('loop, one pass', range(loop[0], loop[1] + 1), 1),
                         ('behind the loop', range(loop[1] + 1, len(bl)), 1)):
        c, v = {}, {}
        for j in rng:
            add(c, per[j][0], w)
            add(v, per[j][1], w)
        parts[part] = (c, v)
    tot_c, tot_v = {}, {}
    for part, (c, v) in parts.items():
        w = trips if part == 'loop, one pass' else 1
        add(tot_c, c, w)
        add(tot_v, v, w)
    assert tot_c['mfma'] == need
    return dict(name=name, targs=m.groups(), trips=trips, parts=parts, total=(tot_c, tot_v))


def scratch_of(path):
    out, name = {}, None
    for ln in open(path):
        m = re.match(r'\s+\.name:\s+(\S+)', ln)
        if m:
            name = m.group(1)
        m = re.match(r'\s+\.private_segment_fixed_size:\s+(\d+)', ln)
        if m and name:
            out.setdefault(name, {})['scratch'] = int(m.group(1))
        m = re.match(r'\s+\.vgpr_count:\s+(\d+)', ln)             # (architectural + accumulator registers)
        if m and name:
            out.setdefault(name, {})['vgpr'] = int(m.group(1))
        m = re.match(r'\s+\.set\s+(\S+)\.num_agpr,\s*(\d+)', ln)
        if m:
            out.setdefault(m.group(1), {})['agpr'] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('path')
    ap.add_argument('--kernel', default=KODAK, help='regex on the mangled name (default: the Kodak instantiation)')
    ap.add_argument('--all', action='store_true', help='one summary line per instantiation')
    a = ap.parse_args()
    meta = scratch_of(a.path)
    found = 0
    for name, body in kernels(a.path):
        if not NAME.search(name):
            continue
        if not a.all and not re.search(a.kernel, name):
            continue
        found += 1
        r = count_kernel(name, body)
        md = meta.get(name, {})
        tc, tv = r['total']
        if a.all:
            print('<{}>  loop x{}  mfma {}  vector {}  (accvgpr {} mov {} dpp {} select {} int {} arith {})  lds {}  memory {}  scalar {}  vgpr {} agpr {} scratch {}'.format(
                ','.join(r['targs']), r['trips'], tc['mfma'], tc['vector'], tv['accvgpr'], tv['mov'], tv['dpp'], tv['select'], tv['int'], tv['arith'],
                tc['lds'], tc['memory'], tc['scalar'], md.get('vgpr', '?'), md.get('agpr', '?'), md.get('scratch', '?')))
            continue
        print('{}\n  <WT,RES,CIN,COUT,SHUF,SEG2,WG8,STATS> = <{}>   vgpr {} agpr {} scratch {} bytes'.format(
            name, ','.join(r['targs']), md.get('vgpr', '?'), md.get('agpr', '?'), md.get('scratch', '?')))
        hdr = '  {:24s} {:>6s} {:>7s} {:>5s} {:>7s} {:>7s} | {:>7s} {:>5s} {:>5s} {:>6s} {:>5s} {:>6s}'.format(
            'part', 'mfma', 'vector', 'lds', 'memory', 'scalar', 'accvgpr', 'mov', 'dpp', 'select', 'int', 'arith')
        print(hdr)
        for part, (c, v) in r['parts'].items():
            label = part + (' (x{})'.format(r['trips']) if part.startswith('loop') else '')
            print('  {:24s} {:6d} {:7d} {:5d} {:7d} {:7d} | {:7d} {:5d} {:5d} {:6d} {:5d} {:6d}'.format(
                label, *[c.get(k, 0) for k in CLASSES], *[v.get(k, 0) for k in VKINDS]))
        print('  {:24s} {:6d} {:7d} {:5d} {:7d} {:7d} | {:7d} {:5d} {:5d} {:6d} {:5d} {:6d}'.format(
            'per wave (weighted)', *[tc[k] for k in CLASSES], *[tv[k] for k in VKINDS]))
        print('  non-MFMA vector instructions per wave: {}   per MFMA: {:.3f}'.format(tc['vector'], tc['vector'] / float(tc['mfma'])))
    if not found:
        sys.exit('no instantiation of wino4_3x3_kernel matches')


if __name__ == '__main__':
    main()
