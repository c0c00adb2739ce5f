#!/usr/bin/env python
"""What a BLSTM layer call decides about its recurrent path, as a table: for a fixed grid of descriptors, one JSON
line each with the answers of the size and query exports of libnabu_hip.so

    nabu_blstm_uses_persistent, nabu_blstm_emits_packed (all three companions requested through placeholder
    pointers, as the layer does), nabu_blstm_reserve_bytes, nabu_blstm_ws_bytes, nabu_blstm_pk_bytes.

Nothing is launched.  The NABU_PERSIST_* switches are read once per process, so the table of every switch setting in
ENVS comes from a child process of its own.  The dense products are f16x3 (the precision under which companions exist).

    python tools/persist_dispatch_table.py                 # JSON lines on stdout, every setting of ENVS
    python tools/persist_dispatch_table.py --golden FILE   # the same table in the compact form of tests/golden/
    python tools/persist_dispatch_table.py --compare FILE  # regenerate and compare with a golden; exit status 1 on a difference

A golden (tests/golden/persist_dispatch_*.json) keeps every field as a column over the axes it depends on (compact());
expand() gives the full rows back, so a comparison is field for field."""
import argparse
import ctypes
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# axes, outermost first; the ones a size rarely depends on vary fastest (long runs in a golden's columns)
GRID = (('H', (32, 64, 128, 256, 512)),
        ('D', (40, 64, 80, 256, 1024)),
        ('B', (1, 4, 9, 16, 32, 33, 48, 64, 65, 96, 128)),
        ('T', (1, 33, 125, 1000)),
        ('fwd_only', (0, 1)),
        ('rec', ('default', 'f32')),
        ('short', (0, 1)),                       # 1: max_len = T // 2 (< T) where T > 1, else max_len = T
        ('mode', (0, 2, 1)))                     # NABU_LSTM_AUTO, _PERSISTENT, _STEPWISE
ENVS = ('', 'NABU_PERSIST_MX=0', 'NABU_PERSIST_MXF=0', 'NABU_PERSIST_MXF=2', 'NABU_PERSIST_FUSE_INPUT=0',
        'NABU_PERSIST_EMIT=0', 'NABU_PERSIST_DEBUG=1')
SWITCHES = ('NABU_PERSIST_MX', 'NABU_PERSIST_MXF', 'NABU_PERSIST_FUSE_INPUT', 'NABU_PERSIST_EMIT', 'NABU_PERSIST_DEBUG',
            'NABU_PERSIST_EMIT_MASK', 'NABU_PK', 'NABU_GEMM_PRECISION')
FIELDS = ('uses_persistent', 'emits_packed', 'reserve_bytes', 'ws_bytes', 'pk_bytes')


def points():
    for vals in itertools.product(*(v for _, v in GRID)):
        yield dict(zip((n for n, _ in GRID), vals))


def rows():
    """the table of THIS process (its environment as it is)"""
    from nabu_amd import _hip
    L = _hip.lib()
    pkb = (ctypes.c_size_t * 5)()
    for p in points():
        T = p['T']
        max_len = T // 2 if (p['short'] and T > 1) else T
        d = _hip.BlstmDesc(ctypes.sizeof(_hip.BlstmDesc), p['B'], T, p['D'], p['H'], max_len, p['mode'],
                           _hip.GEMM_PRECISIONS['f16x3'], 0.0, _hip.BLSTM_FWD_ONLY if p['fwd_only'] else 0,
                           _hip.REC_PRECISIONS[p['rec']], 0, None, None, None, None, None)
        ref = ctypes.byref(d)
        row = dict(p)
        row['uses_persistent'] = int(L.nabu_blstm_uses_persistent(ref))
        row['reserve_bytes'] = int(L.nabu_blstm_reserve_bytes(ref))
        row['ws_bytes'] = int(L.nabu_blstm_ws_bytes(ref))
        row['pk_bytes'] = [int(v) for v in pkb] if L.nabu_blstm_pk_bytes(ref, pkb) == 0 else None
        d.out_pk_rows = d.out_pk_cols = d.hT_pk = 1          # placeholders: the query reads them for null only
        row['emits_packed'] = int(L.nabu_blstm_emits_packed(ref))
        yield row


def child_rows(env, extra=None):
    """the table under one setting of ENVS: a fresh process, the other switches unset (extra: more environment)"""
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(extra or {})
    if env:
        k, v = env.split('=')
        e[k] = v
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=e, stdout=subprocess.PIPE, check=True).stdout
    return [json.loads(line) for line in out.decode().splitlines()]


NO_DEVICE = {'HIP_VISIBLE_DEVICES': '-1', 'ROCR_VISIBLE_DEVICES': '-1'}     # the table of a host without a GPU, anywhere


def table(extra=None):
    return {env: child_rows(env, extra) for env in ENVS}


def rle(col):
    out = []
    for v in col:
        if out and out[-2] == v:
            out[-1] += 1
        else:
            out += [v, 1]
    return out


def unrle(col):
    return [v for v, n in zip(col[0::2], col[1::2]) for _ in range(n)]


# a golden stores the five sizes of pk_bytes as columns of their own (each depends on fewer axes than the list)
STORED = FIELDS[:-1] + tuple('pk_bytes_%d' % i for i in range(5))


def stored(row, f):
    if not f.startswith('pk_bytes_'):
        return row[f]
    return None if row['pk_bytes'] is None else row['pk_bytes'][int(f[-1])]


def keys(axes):
    """the points of the sub-grid spanned by `axes`, in GRID order"""
    return list(itertools.product(*(v for n, v in GRID if n in axes)))


def project(rws, f, axes):
    """{point of the sub-grid: value} if field f is a function of `axes` alone in these rows, else None"""
    m = {}
    for r in rws:
        v = stored(r, f)
        if m.setdefault(tuple(r[n] for n, _ in GRID if n in axes), v) != v:
            return None
    return m


def compact(tab, note):
    """per stored field: the axes it depends on under any setting; its values over that sub-grid (GRID order, last axis
    fastest) as run-length pairs [value, count, ...] for the default setting; for every other setting '=' (the same
    column), or {"set": [position, value, ...]} (the default's column with these positions replaced)"""
    g = {'note': note, 'grid': [[n, list(v)] for n, v in GRID], 'envs': list(ENVS), 'fields': list(FIELDS), 'columns': {}}
    for f in STORED:
        axes = [n for n, _ in GRID]
        for n, _ in GRID:
            rest = [x for x in axes if x != n]
            if all(project(tab[env], f, rest) is not None for env in ENVS):
                axes = rest
        ks = keys(axes)
        cols = {}
        for env in ENVS:
            m = project(tab[env], f, axes)
            cols[env] = [m[k] for k in ks]
        c = {'axes': axes, '': rle(cols[''])}
        for env in ENVS[1:]:
            d = [x for i, (a, b) in enumerate(zip(cols[''], cols[env])) if a != b for x in (i, cols[env][i])]
            c[env] = {'set': d} if d else '='
        g['columns'][f] = c
    return g


def expand(g):
    """a golden -> {setting: rows}"""
    assert [[n, list(v)] for n, v in GRID] == g['grid'] and list(ENVS) == g['envs'] and list(FIELDS) == g['fields'], \
        'the golden was written for another grid'
    tab = {env: [dict(p) for p in points()] for env in ENVS}
    for env in ENVS:
        for f in STORED:
            c = g['columns'][f]
            col = unrle(c[''])
            if env and c[env] != '=':
                for i, v in zip(c[env]['set'][0::2], c[env]['set'][1::2]):
                    col[i] = v
            m = dict(zip(keys(c['axes']), col))
            assert len(m) == len(col), (env, f, len(col))
            for r in tab[env]:
                r[f] = m[tuple(r[n] for n, _ in GRID if n in c['axes'])]
        for r in tab[env]:
            pk = [r.pop('pk_bytes_%d' % i) for i in range(5)]
            r['pk_bytes'] = None if None in pk else pk
    return tab


def write_golden(path, g):
    with open(path, 'w') as fid:
        fid.write('{\n')
        for k in ('note', 'grid', 'envs', 'fields'):
            fid.write('%s: %s,\n' % (json.dumps(k), json.dumps(g[k], separators=(',', ':'))))
        fid.write('"columns": {\n')
        fid.write(',\n'.join('%s: {\n%s\n}' % (json.dumps(f), ',\n'.join(
            '%s: %s' % (json.dumps(k), json.dumps(v, separators=(',', ':'))) for k, v in g['columns'][f].items()))
            for f in STORED))
        fid.write('\n}\n}\n')


def differences(got, want, limit=20):
    """field-for-field comparison of two tables; a list of messages (empty: equal)"""
    msgs = []
    for env in ENVS:
        if len(got[env]) != len(want[env]):
            msgs.append('%s: %d rows, golden has %d' % (env or 'default', len(got[env]), len(want[env])))
            continue
        for a, b in zip(got[env], want[env]):
            for k in b:
                if a.get(k) != b[k]:
                    if len(msgs) < limit:
                        msgs.append('[%s] %s: %s = %r, golden %r' % (
                            env or 'default', ' '.join('%s=%s' % (n, b[n]) for n, _ in GRID), k, a.get(k), b[k]))
                    elif len(msgs) == limit:
                        msgs.append('...')
    return msgs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--child', action='store_true', help='print the table of this process only')
    ap.add_argument('--golden', metavar='FILE', help='write the compact form')
    ap.add_argument('--note', default='', help='kept in the golden: which library and device produced it')
    ap.add_argument('--compare', metavar='FILE', help='compare with a golden')
    ap.add_argument('--no-device', action='store_true', help='hide the GPUs from the library (the table of a host without one)')
    a = ap.parse_args()
    if a.child:
        for r in rows():
            print(json.dumps(r, separators=(',', ':')))
        return 0
    tab = table(NO_DEVICE if a.no_device else None)
    if a.golden:
        write_golden(a.golden, compact(tab, a.note))
        return 0
    if a.compare:
        with open(a.compare) as fid:
            msgs = differences(tab, expand(json.load(fid)))
        print('\n'.join(msgs) if msgs else 'equal: %d rows x %d settings' % (len(tab['']), len(ENVS)))
        return 1 if msgs else 0
    for env in ENVS:
        for r in tab[env]:
            print(json.dumps(dict(r, env=env), separators=(',', ':')))
    return 0


if __name__ == '__main__':
    sys.exit(main())
