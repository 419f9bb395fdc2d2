"""The float64 SpMM test inputs check themselves, and the float64 launch plan
is the hand-written table — on the CPU, against the built library (the plan
query needs no device)."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests import spmm_cases as sc
from tests import spmm_cases_f64 as s64

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def hip():
    from arrow_matrix_amd import hip
    if not hip.is_built():
        subprocess.run(['make', '-C',
                        os.path.join(REPO, 'arrow_matrix_amd', 'csrc')],
                       check=True, capture_output=True)
    return hip


def _exact_cases():
    return [s64.case('std', 130, 1, 0, None),
            s64.case('dual', 7, 1, 0, None, matrix='std_dual'),
            s64.case('rowids', 8, 0, 0, None, row_ids=True)]


def test_exact_operands_are_exact_in_double_only():
    """The float64 product equals an integer-scaled recomputation (units of
    2**-31, int64 arithmetic), stays inside the 49-bit headroom, and is NOT
    reproduced once X is rounded to fp32: the inputs discriminate."""
    for c in _exact_cases():
        X0, X1, C0 = s64.operands(c)
        m = sc.matrix(c['matrix'])
        _, ref = s64.reference(c, X0, X1, C0)
        # integers: a in units of 0.5, x in units of 2**-30
        A_int = sc._csr(m, s64.values(c['matrix'], 'exact') * 2, np.int64)
        X_int = np.rint(np.vstack([X0, X1]) * 2.0 ** 30).astype(np.int64)
        assert (X_int * 2.0 ** -30 == np.vstack([X0, X1])).all()
        want = np.asarray(A_int @ X_int)
        if c['beta']:
            rows = s64._rows(c, want.shape[0])
            want = want + 2 * np.rint(C0[rows] * 2.0 ** 30).astype(np.int64)
        assert np.abs(want).max() < 2 ** 49
        np.testing.assert_array_equal(ref, want.astype(np.float64) * 2.0 ** -31)
        # one element against exact rationals
        r = int(np.argmax(np.diff(m['indptr'])))
        b, e = m['indptr'][r], m['indptr'][r + 1]
        X = np.vstack([X0, X1])
        cols = np.where(m['cols'] < 0, m['n0'] - m['cols'].astype(np.int64) - 1,
                        m['cols'])
        acc = sum((Fraction(float(v)) * Fraction(float(X[cc, 0]))
                   for v, cc in zip(s64.values(c['matrix'], 'exact')[b:e],
                                    cols[b:e])), Fraction(0))
        if c['beta']:
            acc += Fraction(float(C0[s64._rows(c, m['rows'])[r], 0]))
        assert Fraction(float(ref[r, 0])) == acc
        # fp32 staging of X loses the 2**-30 parts
        X0f = X0.astype(np.float32).astype(np.float64)
        X1f = X1.astype(np.float32).astype(np.float64)
        assert (X0f != X0).any()
        _, staged = s64.reference(c, X0f, X1f, C0)
        assert (staged != ref).any()


def _double_row_sums(c, X0, X1, C0, reverse):
    m = sc.matrix(c['matrix'])
    vals = s64.values(c['matrix'], c['kind'])
    X = np.vstack([X0, X1])
    cols = np.where(m['cols'] < 0, m['n0'] - m['cols'].astype(np.int64) - 1,
                    m['cols'])
    rows = s64._rows(c, m['rows'])
    out = np.zeros((m['rows'], c['k']))
    for r in range(m['rows']):
        idx = range(m['indptr'][r], m['indptr'][r + 1])
        acc = C0[rows[r]].copy() if c['beta'] else np.zeros(c['k'])
        for t in (reversed(idx) if reverse else idx):
            acc = acc + vals[t] * X[cols[t]]
        out[r] = acc
    return out


@pytest.mark.parametrize('beta', [0, 1])
def test_real_cases_inside_the_bound(beta):
    """Forward and reversed double summation both stay inside the derived
    bound around the extended-precision reference."""
    c = s64.case('real', 12, beta, 0, None, matrix='real', kind='real')
    X0, X1, C0 = s64.operands(c)
    _, ref = s64.reference_longdouble(c, X0, X1, C0)
    bound = s64.real_bound(c, X0, X1, C0)
    for reverse in (False, True):
        got = _double_row_sums(c, X0, X1, C0, reverse)
        err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
        assert (err <= bound).all()
    # and the bound is a float64 bound: fp32 accumulation falls outside it
    got32 = s64.product(c, X0, X1, dtype=np.float32).astype(np.longdouble)
    if beta:
        got32 = got32 + C0.astype(np.float32).astype(np.longdouble)
    assert (np.abs(got32 - ref).astype(np.float64) > bound).any()


def test_table_matches_its_rule():
    for k, (vec, group, launches) in {**s64.PLAN_TABLE,
                                      **s64.PLAN_EXTRA}.items():
        assert vec == (2 if k % 2 == 0 else 1)
        lanes = -(-k // vec)
        assert group == min(64, 1 << (lanes - 1).bit_length())
        assert launches == -(-k // (vec * group))


@pytest.mark.parametrize('queue', [-1, 0, 1])
def test_f64_plan_equals_the_table(hip, queue):
    for k in s64.K_ALL:
        for nnz in (1000, 1 << 26):
            sched = {0: s64.GRID, 1: s64.default_queued(k),
                     -1: s64.policy(k, nnz)}[queue]
            got = hip.spmm_plan(k, nnz, queue, dtype=np.float64)
            assert got == s64.plan(k, sched), (k, nnz, queue)


@pytest.mark.parametrize('queue', [-1, 0, 1])
def test_f32_plan_unchanged(hip, queue):
    for k in sc.K_ALL:
        sched = sc.default_queued(k) if queue == 1 else sc.GRID
        assert hip.spmm_plan(k, 1000, queue, dtype=np.float32) == \
            sc.plan(k, sched)
        assert hip.spmm_plan(k, 1000, queue) == sc.plan(k, sched)


_PLAN_CHILD = """
import json, sys
import numpy as np
from arrow_matrix_amd import hip
ks = json.loads(sys.argv[1])
print(json.dumps([[hip.spmm_plan(k, 1 << 26, q, dtype=np.float64)
                   for q in (-1, 0, 1)] for k in ks]))
"""


@pytest.mark.parametrize('var', ['ARROW_SPMM_G64', 'ARROW_K16_G8'])
def test_fp32_layout_variables_do_not_touch_the_f64_plan(hip, var):
    """The variables are read once per process, so a child starts with one
    set; its float64 plans equal the table all the same."""
    ks = [16, 128]
    env = sc.child_env(os.environ, {var: '1'})
    p = subprocess.run([sys.executable, '-c', _PLAN_CHILD, json.dumps(ks)],
                       cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    for k, per_q in zip(ks, got):
        want = [s64.plan(k, s64.policy(k, 1 << 26)), s64.plan(k, s64.GRID),
                s64.plan(k, s64.default_queued(k))]
        assert per_q == want, (var, k)


@pytest.mark.parametrize('dtype', [np.float16, np.int32, np.complex128, 'bf16'])
def test_other_dtypes_raise_type_error(hip, dtype):
    """The binding's own dtype check, with its message: a binding without
    the dtype= keyword raises a TypeError of another kind."""
    msg = 'float32 or float64'
    with pytest.raises(TypeError, match=msg):
        hip._suffix(dtype)
    with pytest.raises(TypeError, match=msg):
        hip.spmm_plan(16, 1000, -1, dtype=dtype)
    # the routing calls check the dtype before anything is launched
    for route in (hip.gather_rows, hip.scatter_rows, hip.scatter_add_rows):
        with pytest.raises(TypeError, match=msg):
            route(0, 0, 0, 0, 4, dtype=dtype)
    for route in (hip.permute_rows, hip.permute_add_rows):
        with pytest.raises(TypeError, match=msg):
            route(0, 0, 0, 0, 0, 4, dtype=dtype)


def test_supported_dtypes_are_named(hip):
    assert hip._suffix(np.float32) == hip._suffix('float32') == 'f32'
    assert hip._suffix(np.float64) == hip._suffix(float) == 'f64'


def test_abi_version(hip):
    assert hip.abi_version() >= 1003


def test_env_table_is_well_formed():
    for name, (variables, cases) in s64.env_table().items():
        names = [c['name'] for c in cases]
        assert len(names) == len(set(names)), name
        ks = {c['k'] for c in cases if c['matrix'] == 'std'}
        assert set(s64.K_ALL) <= ks, name
        assert sum(c['kind'] == 'real' for c in cases) == 1, name
