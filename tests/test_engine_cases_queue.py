"""tests/engine_cases_queue.py without a GPU: the exactness budget of every
layout, the exact reference against the cpu-device engine bit for bit, K_OF
and the plans of QUEUE_ENVS against the library's own policy, and the job
names the driver and the GPU test share."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import engine_affine_driver as ead
from tests import engine_cases_queue as ecq
from tests import engine_scale_driver as esd
from tests import spmm_cases as sc
from tests.gpu_children import ENGINE_VARS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, 'arrow_matrix_amd', 'libarrowspmm.so')
PLAN_SYMBOL = {'float32': 'arrow_spmm_plan', 'float64': 'arrow_spmm_plan_f64',
               'bfloat16': 'arrow_spmm_plan_bf16'}
FIELDS = ('vec', 'group', 'scheduler', 'nt_mode', 'chunk_items', 'grid_cap',
          'launches')

# argv: library, JSON list of [symbol, k, nnz, queue_mode]; prints the plans
CHILD = r'''
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
res = []
for symbol, k, nnz, mode in json.loads(sys.argv[2]):
    fn = getattr(lib, symbol)
    fn.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                   ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    fn.restype = ctypes.c_int
    out = (ctypes.c_int32 * 7)()
    assert fn(k, nnz, mode, out, 7) == 7
    res.append(list(out))
print(json.dumps(res))
'''


# ---------------------------------------------------------------------------
# the exact class
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('layout', list(ecq.LAYOUTS))
def test_exactness_budget(layout):
    """The longest row of the recomposed pattern, counted in stored values
    over all parts, is within spmm_cases_affine's budget; the pattern and
    the permutations are the synth decomposition's; values, features and
    residual are of the exact class."""
    decomp = ecq.exact_decomposition(layout)
    synth = esd.make_decomp(**ecq.LAYOUTS[layout][1])
    assert len(decomp) == len(synth)
    for (B, p), (S, q) in zip(decomp, synth):
        assert (B.indptr == S.indptr).all() and (B.indices == S.indices).all()
        assert (p == q).all()
        assert np.isin(B.data, sc.EXACT_VALS).all() and B.dtype == np.float32
        # every value of the class is drawn
        assert set(np.unique(B.data)) == set(sc.EXACT_VALS)
    terms = ecq.row_terms(decomp)
    # the count is of stored values: where parts overlap it exceeds the
    # recomposed row's own length
    own = np.diff(ecq.exact_matrix(layout).indptr)
    assert (terms >= own).all() and terms.sum() == sum(B.nnz for B, _ in decomp)
    longest, units = ecq.exact_budget(layout)
    assert longest == terms.max() <= ecq.MAX_ROW_TERMS == 8192
    assert units < 2 ** 24
    for k in (row[0] for p in ecq.PRECISIONS for row in ecq.K_OF[p]):
        X, R, perm0 = ecq.exact_operands(layout, k)
        assert X.shape == R.shape == (ecq.n_rows(layout), k)
        for a in (X, R):
            assert (a == np.round(a)).all() and np.abs(a).max() == 8
        assert (perm0 == decomp[0][1]).all()


def test_hub_layout_has_split_rows():
    B0 = ecq.exact_decomposition('hub')[0][0]
    assert (np.diff(B0.indptr) > sc.SEG_NNZ).sum() >= 1
    assert ecq.exact_budget('hub')[0] > sc.SEG_NNZ


@pytest.mark.parametrize('tier', ['plain', 'affine'])
@pytest.mark.parametrize('precision', esd.PRECISIONS['cpu'])
@pytest.mark.parametrize('layout', list(ecq.LAYOUTS))
def test_exact_reference_equals_the_cpu_device(monkeypatch, layout, precision,
                                               tier):
    """One step of the cpu-device engine (scipy, per block, in the engine's
    precision) on exact_decomposition equals exact_reference bit for bit:
    this tests the reference. The cpu device reads ARROW_FOLD and the shape
    (banded or not); the other layout variables select GPU structures only,
    and their shapes run here all the same."""
    for var in ENGINE_VARS:
        monkeypatch.delenv(var, raising=False)
    for var, value in ecq.LAYOUTS[layout][0].items():
        monkeypatch.setenv(var, value)
    k = ecq.K_OF[precision][0][0]
    dt = np.float64 if precision == 'float64' else np.float32
    arrow = esd.load(ecq.exact_decomposition(layout), precision, 'cpu',
                     **ecq.build_args(layout, k))
    esd.assert_layout(layout, arrow, 'cpu')
    X, R, perm0 = ecq.exact_operands(layout, k)
    arrow.B.set_features(X[perm0].astype(dt))
    if tier != 'plain':
        arrow.set_affine_step(ecq.EXACT_ALPHA, ecq.EXACT_GAMMA,
                              R[perm0].astype(dt))
    arrow.step()
    C = arrow.B.result_tile().numpy()
    G = ecq.exact_reference(layout, k, tier)
    assert C.dtype == dt and C.shape == G.shape
    ref = G.astype(dt)
    assert (ref.astype(np.float64) == G).all()
    word = np.uint64 if dt == np.float64 else np.uint32
    assert (C.view(word) == ref.view(word)).all()
    assert np.abs(G).max() > 0
    # the affine tier is not the plain one scaled away
    assert tier == 'plain' or \
        not (G == ecq.exact_reference(layout, k, 'plain')).all()


def test_plain_step_bound_is_the_affine_drivers_at_alpha_1_gamma_0():
    """step_bound's golden and bound are linear in alpha at R = 0."""
    A = ecq.exact_matrix('fold1')
    rng = np.random.default_rng(3)
    X = 2 * rng.random((A.shape[0], 8)) - 1
    for precision in ecq.PRECISIONS:
        G, b = ecq.plain_step_bound(A, abs(A), X, 2, precision)
        Ga, ba = ead.step_bound(A, abs(A), X, np.zeros_like(X), 2, precision)
        np.testing.assert_allclose(ead.ALPHA * G, Ga, rtol=1e-14, atol=0)
        np.testing.assert_allclose(ead.ALPHA * b, ba, rtol=1e-14, atol=0)
        assert (b > 0).any()


# ---------------------------------------------------------------------------
# K_OF and QUEUE_ENVS against the library
# ---------------------------------------------------------------------------

@pytest.fixture(scope='module')
def lib_path():
    if not os.path.exists(LIB):
        try:
            subprocess.run(['make', '-C', os.path.join(
                REPO, 'arrow_matrix_amd', 'csrc')], check=True,
                capture_output=True)
        except (OSError, subprocess.CalledProcessError):
            pytest.skip("libarrowspmm.so cannot be built here")
    return LIB


QUERIES = [(p, row[0]) for p in ecq.PRECISIONS for row in ecq.K_OF[p]]


def _ask(lib_path, variables):
    env = {k: v for k, v in sc.child_env(os.environ, variables).items()
           if k not in ENGINE_VARS}
    q = [[PLAN_SYMBOL[p], k, 1, -1] for p, k in QUERIES]
    p = subprocess.run([sys.executable, '-c', CHILD, lib_path, json.dumps(q)],
                       env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return [dict(zip(FIELDS, r))
            for r in json.loads(p.stdout.strip().splitlines()[-1])]


@pytest.mark.parametrize('queue_env', list(ecq.QUEUE_ENVS))
def test_k_of_against_the_library(lib_path, queue_env):
    """A structure of one nonzero at handle mode -1 gets the scheduler, vec,
    group, chunk_items and grid_cap the tables claim, in a process that
    starts with the queue environment."""
    plans = _ask(lib_path, ecq.QUEUE_ENVS[queue_env])
    table = {(p, row[0]): row for p in ecq.PRECISIONS for row in ecq.K_OF[p]}
    for (p, k), got in zip(QUERIES, plans):
        assert got == ecq.expected_plan(queue_env, p, k), (p, k)
        _, vec, group, sched = table[p, k]
        assert (got['vec'], got['group'], got['scheduler']) == \
            (vec, group, sched), (p, k)
        mult = {'policy': {ecq.QWAVE: 2, ecq.QBLOCK: 4},
                'chunk1': {ecq.QWAVE: 1, ecq.QBLOCK: 1}}[queue_env][sched]
        lanes = 64 if sched == ecq.QWAVE else 256
        assert got['chunk_items'] == lanes // group * mult
        assert got['grid_cap'] == (2048 if queue_env == 'policy' else 8)
    # each precision has one width of each queue scheduler
    for p in ecq.PRECISIONS:
        assert [row[3] for row in ecq.K_OF[p]] == [ecq.QWAVE, ecq.QBLOCK]


def test_without_the_variables_every_plan_is_grid_stride(lib_path):
    """What every engine test ran until now."""
    for got in _ask(lib_path, {}):
        assert got['scheduler'] == ecq.GRID and got['chunk_items'] == 0
    # and the kernel table's chunk variables alone do not queue either
    for got in _ask(lib_path, sc.env_table()['chunk1'][0]):
        assert got['scheduler'] == ecq.GRID


# ---------------------------------------------------------------------------
# children and job names
# ---------------------------------------------------------------------------

def test_children_and_job_names():
    children = ecq.children()
    assert len(children) == len(set(children)) == 14
    assert [c for c in children if c[0] == 'policy'] == \
        [('policy', layout) for layout in ecq.LAYOUTS]
    assert len(ecq.LAYOUTS) == 10
    assert [layout for q, layout in children if q == 'chunk1'] == \
        ['default', 'hub', 'fuse_all0', 'fold1']
    first = ecq.jobs(*children[0])
    for queue_env, layout in children:
        jobs = ecq.jobs(queue_env, layout)
        assert jobs == first == ecq.jobs(queue_env, layout)
        names = [name for name, *_ in jobs]
        assert len(set(names)) == len(names) == 3 * 2 * 3
        for name, p, k, tier in jobs:
            assert name == ecq.job_name(p, k, tier)
            assert k in [row[0] for row in ecq.K_OF[p]]
        variables = ecq.child_variables(queue_env, layout)
        assert variables['ARROW_Q_MIN_NNZ'] == '0'
        assert set(variables) <= set(sc.KERNEL_VARS + ENGINE_VARS)
        assert {v: variables[v] for v in variables if v in ENGINE_VARS} == \
            ecq.LAYOUTS[layout][0]
        assert ('ARROW_Q_CHUNK' in variables) == (queue_env == 'chunk1')
    with pytest.raises(AssertionError):
        ecq.jobs('chunk1', 'banded')
    assert len({ecq.capture_job_name(*j) for j in ecq.CAPTURE_JOBS}) == 3


def test_layout_tables_agree_with_the_engine_drivers():
    """Shapes and variables are the drivers'; only k moves."""
    from tests import engine_norm_driver as end
    for name, (variables, shape, inside) in ead.MODES.items():
        assert ecq.LAYOUTS[name] == (variables, shape)
        assert (name in ecq.AFFINE_INSIDE) == inside
    for name, (variables, shape, fused) in end.MODES.items():
        assert ecq.LAYOUTS[name] == (variables, shape)
        assert (name in ecq.NORM_FUSED) == fused
    assert ecq.LAYOUTS['hub'] == esd.MODES['hub']
    assert ecq.build_args('hub', 128) == dict(ead.HUB, k=128)
    assert ecq.LAYOUTS['hub'][1]['hub_rows'] == 2
