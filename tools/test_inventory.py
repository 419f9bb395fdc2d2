"""Prints one line per GPU kernel test input, with SHA-256 digests of its
bytes: every case of every env_table() of the three precisions (operands,
A's values, reference and, for real kinds, the bound) and every route case
(src, dst0, both index arrays, ref).

    python tools/test_inventory.py > inventory.txt
    python tools/test_inventory.py --summary     # one digest per case set

With --summary the lines of each (precision, case set) and of each
precision's routes are folded into one line: their number and a SHA-256
over them. It reads the case modules only (tests/spmm_cases*.py), never the
drivers, so the same script runs on any two commits; equal outputs mean that
no test input, expectation or bound moved between them.
"""
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import spmm_cases as sc  # noqa: E402
from tests import spmm_cases_bf16 as s16  # noqa: E402
from tests import spmm_cases_f64 as s64  # noqa: E402


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is None:
            h.update(b'none')
            continue
        a = np.ascontiguousarray(a)
        if a.dtype == np.longdouble:
            # x87 extended has padding bytes: hash the value, as two doubles
            hi = a.astype(np.float64)
            a = np.stack([hi, (a - hi).astype(np.float64)])
        h.update(f'{a.dtype.str}{a.shape}'.encode())
        h.update(a.tobytes())
    return h.hexdigest()[:16]


def f32_case(c):
    m = sc.matrix(c['matrix'])
    ops = sc.operands(c)
    vals = m['real_vals'] if c['kind'] == 'legacy' else m['vals']
    rows, ref = sc.reference(c, *ops)
    bound = sc.real_bound(c, *ops) if c['kind'] != 'exact' else None
    return ops, vals, (rows, ref), bound


def f64_case(c):
    ops = s64.operands(c)
    fn = s64.reference_longdouble if c['kind'] == 'real' else s64.reference
    bound = s64.real_bound(c, *ops) if c['kind'] != 'exact' else None
    return ops, s64.values(c['matrix'], c['kind']), fn(c, *ops), bound


def bf16_case(c):
    ops = s16.operands(c)
    rows, G = s16.reference(c, *ops)
    bound = s16.real_bound(c, *ops, G) if c['kind'] != 'exact' else None
    return ops, sc.matrix(c['matrix'])['vals'], (rows, G), bound


PRECISIONS = (('f32', sc, f32_case, sc.ROUTE_SHAPES),
              ('f64', s64, f64_case, sc.ROUTE_SHAPES),
              ('bf16', s16, bf16_case, s16.ROUTE_SHAPES))


def lines():
    for prec, mod, digest, shapes in PRECISIONS:
        memo = {}       # cases that differ only in queue/plan share inputs
        for env, (variables, cases) in mod.env_table().items():
            for c in cases:
                key = json.dumps({k: v for k, v in c.items()
                                  if k not in ('name', 'queue', 'plan',
                                               'qblocks', 'col_items',
                                               'remap', 'repeat')},
                                 sort_keys=True)
                if key not in memo:
                    ops, vals, (rows, ref), bound = digest(c)
                    memo[key] = (f'operands={sha(*ops)} A={sha(vals)} '
                                 f'ref={sha(rows, ref)} bound={sha(bound)}')
                yield (prec, env, json.dumps(variables, sort_keys=True),
                       c['name'], json.dumps(c, sort_keys=True), memo[key])
        for op in sc.ROUTE_OPS:
            for n, k in shapes:
                rc = mod.route_case(op, n, k)
                yield (prec, 'route', op, n, k,
                       sha(rc['src'], rc['dst0'], rc['src_idx'],
                           rc['dst_idx'], rc['ref']))


def main(argv):
    if '--summary' not in argv:
        for line in lines():
            print(*line)
        return
    groups = {}         # (precision, case set) -> [lines, running hash]
    for line in lines():
        group = groups.setdefault(line[:2], [0, hashlib.sha256()])
        group[0] += 1
        group[1].update((' '.join(map(str, line)) + '\n').encode())
    for (prec, env), (n, h) in groups.items():
        print(f'{prec:<5}{env:<9}{n:>4} lines  sha256 {h.hexdigest()[:32]}')


if __name__ == '__main__':
    main(sys.argv)
