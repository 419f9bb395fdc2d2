"""arrow_spmm_plan: the environment -> launch-plan policy, asserted without a
GPU. The kernel variables are read once per process, so every environment is
queried in a fresh child that loads libarrowspmm.so with ctypes only."""
import json
import os
import subprocess
import sys

import pytest

from tests import spmm_cases as sc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, 'arrow_matrix_amd', 'libarrowspmm.so')
FIELDS = ('vec', 'group', 'scheduler', 'nt_mode', 'chunk_items', 'grid_cap',
          'launches')

# argv: library, JSON list of [k, nnz, queue_mode], JSON dict of variables to
# set AFTER the first pass; prints the plans of pass one and of pass two
CHILD = r'''
import ctypes, json, os, sys
lib = ctypes.CDLL(sys.argv[1])
lib.arrow_spmm_plan.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
lib.arrow_spmm_plan.restype = ctypes.c_int
def ask(queries):
    res = []
    for k, nnz, mode in queries:
        out = (ctypes.c_int32 * 7)()
        assert lib.arrow_spmm_plan(k, nnz, mode, out, 7) == 7
        res.append(list(out))
    return res
queries = json.loads(sys.argv[2])
first = ask(queries)
os.environ.update(json.loads(sys.argv[3]))
print(json.dumps([first, ask(queries)]))
'''


@pytest.fixture(scope='module')
def lib_path():
    if not os.path.exists(LIB):
        subprocess.run(['make', '-C', os.path.join(REPO, 'arrow_matrix_amd',
                                                   'csrc')],
                       check=True, capture_output=True)
    return LIB


def _ask(lib_path, variables, queries, late=None):
    p = subprocess.run([sys.executable, '-c', CHILD, lib_path,
                        json.dumps(queries), json.dumps(late or {})],
                       env=sc.child_env(os.environ, variables),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    first, second = json.loads(p.stdout.strip().splitlines()[-1])
    return ([dict(zip(FIELDS, r)) for r in first],
            [dict(zip(FIELDS, r)) for r in second])


@pytest.mark.parametrize('name', list(sc.env_table()))
def test_env_plan_table(lib_path, name):
    """Every case of the variant table gets the plan the table states."""
    variables, cases = sc.env_table()[name]
    queries = [[c['k'], int(sc.matrix(c['matrix'])['cols'].size),
                -1 if c['queue'] is None else c['queue']] for c in cases]
    plans, _ = _ask(lib_path, variables, queries)
    for c, got in zip(cases, plans):
        assert got == c['plan'], c['name']


def test_table_names_the_variants_it_claims():
    """The table itself reaches what it is for: wave grabs at GROUP 8, 32 and
    64, block grabs at GROUP 1, 2 and 4, float2 x 8 at k=16, float2 x 64 at
    k=128, nt_mode 0, the smallest and the oversized grabs."""
    t = sc.env_table()
    def reached(name, **want):
        return any(all(c['plan'][f] == v for f, v in want.items())
                   for c in t[name][1])
    for g in (8, 32, 64):
        assert reached('qwave1', scheduler=sc.QWAVE, group=g)
    for g in (1, 2, 4):
        assert reached('qwave0', scheduler=sc.QBLOCK, group=g)
        assert reached('default', scheduler=sc.QWAVE, group=g)
    for s in (sc.GRID, sc.QBLOCK):
        assert reached('k16g8', scheduler=s, vec=2, group=8)
        assert reached('g64', scheduler=s, vec=2, group=64)
        assert reached('nt0', scheduler=s, nt_mode=0)
    assert reached('chunk1', grid_cap=8, chunk_items=4, group=64)
    assert reached('chunk1', scheduler=sc.QWAVE, chunk_items=16, group=4)
    # one grab larger than a whole segment (the standard case has 333 items)
    assert reached('chunk64', scheduler=sc.QWAVE, group=1, chunk_items=64 * 64)
    assert reached('chunk64', scheduler=sc.QBLOCK, group=8, chunk_items=32 * 64)
    assert reached('min_nnz0', scheduler=sc.GRID, group=2)
    assert reached('min_nnz0', scheduler=sc.QWAVE, group=4)
    assert reached('min_nnz0', scheduler=sc.QBLOCK, group=64)


def test_pick_cfg_every_k(lib_path):
    """k = 1..520: vec is the widest of 4, 2, 1 that divides k, the lanes
    cover min(k, 64 * vec) columns (a group never exceeds the 64-lane wave;
    at k % 4 == 0 that is min(k, 256)), the group is no larger than needed,
    and the number of column-offset launches is ceil(k / span)."""
    ks = list(range(1, 521))
    plans, _ = _ask(lib_path, {}, [[k, 1000, 0] for k in ks])
    for k, p in zip(ks, plans):
        span = p['group'] * p['vec']
        assert p['vec'] in (1, 2, 4) and k % p['vec'] == 0, (k, p)
        assert p['group'] in sc.GROUPS, (k, p)
        assert p['vec'] == (4 if k % 4 == 0 else 2 if k % 2 == 0 else 1)
        assert span >= min(k, 64 * p['vec']), (k, p)
        if k % 4 == 0:
            assert span >= min(k, 256), (k, p)
        assert p['group'] == 1 or span // 2 < k, (k, p)
        assert p['launches'] == -(-k // span), (k, p)
        assert p['scheduler'] == sc.GRID and p['chunk_items'] == 0
        assert p['grid_cap'] == sc.GRID_STRIDE_CAP and p['nt_mode'] == 1
        if k in sc.VEC_GROUP:
            assert (p['vec'], p['group']) == sc.VEC_GROUP[k]


def test_policy_default_threshold(lib_path):
    """Handle mode -1, nothing set: queues from 32M nnz, at GROUP >= 4."""
    q = [[128, (32 << 20) - 1, -1], [128, 32 << 20, -1], [16, 32 << 20, -1],
         [8, 32 << 20, -1]]
    plans, _ = _ask(lib_path, {}, q)
    assert [p['scheduler'] for p in plans] == [sc.GRID, sc.QBLOCK, sc.QWAVE,
                                               sc.GRID]


@pytest.mark.parametrize('first', ['default', 'qwave1'])
def test_variables_are_read_once(lib_path, first):
    """Setting a variable after the first call does not change the plan."""
    variables, _ = sc.env_table()[first]
    late = {'ARROW_QWAVE': '0', 'ARROW_K16_G8': '1', 'ARROW_SPMM_G64': '1',
            'ARROW_SPMM_NT': '0', 'ARROW_QUEUE': '1', 'ARROW_Q_MIN_NNZ': '0',
            'ARROW_Q_CHUNK': '9', 'ARROW_QW_CHUNK': '9',
            'ARROW_Q_BLOCKS': '16'}
    q = [[k, 5000, mode] for k in (4, 16, 128, 260) for mode in (-1, 0, 1)]
    before, after = _ask(lib_path, variables, q, late=late)
    assert before == after
    # and the late values would have changed it, had they been read first
    fresh, _ = _ask(lib_path, late, q)
    assert fresh != before


def test_bad_arguments(lib_path):
    import ctypes
    lib = ctypes.CDLL(lib_path)
    lib.arrow_spmm_plan.argtypes = [ctypes.c_int64, ctypes.c_int64,
                                    ctypes.c_int,
                                    ctypes.POINTER(ctypes.c_int32),
                                    ctypes.c_int]
    out = (ctypes.c_int32 * 7)()
    assert lib.arrow_spmm_plan(0, 10, 0, out, 7) < 0
    assert lib.arrow_spmm_plan(16, -1, 0, out, 7) < 0
    assert lib.arrow_spmm_plan(16, 10, 0, None, 7) < 0
    # a short buffer gets the leading fields only
    out2 = (ctypes.c_int32 * 7)(*([-7] * 7))
    assert lib.arrow_spmm_plan(16, 10, 0, out2, 2) == 7
    assert list(out2) == [4, 4, -7, -7, -7, -7, -7]
