"""Inputs, references and bounds of the operator-scaling tests (ABI 1007:
arrow_csr_sums, arrow_csr_scale), shared by test_spmm_cases_scale.py and
test_engine_scale_cpu.py on the CPU and by scale_driver.py /
engine_scale_driver.py on the GPU. Built on tests/spmm_cases.py. numpy/scipy
only: this module never touches the GPU.

Indexing, as the header states it: a row vector is indexed by OUTPUT row
(after row_ids), a column c >= 0 indexes the *0 vector, c < 0 the *1 vector
at -c-1.

Exact class. A holds spmm_cases' exact values {+-0.5, +-1, +-2}, the scale
factors come from {0.5, 1, 2} and X holds integers in [-8, 8]. A scaled value
v * r * c is then a multiple of 0.125 of magnitude <= 8 and is held exactly by
fp32 (and so by the single rounding of the contract); a product with X is a
multiple of 0.125 of magnitude <= 64 = 512 units; and a row of up to 4097
terms stays below 2**24 units: every partial sum of an fp32 SpMM on the
scaled matrix is exact in any order, split-row atomics included, and the
sums of the values themselves (multiples of 0.5, far below 2**53 units) are
exact in double in any order. The budget is asserted at import, below.

Real class. Real values (spmm_cases._real) and real factors; the reference is
the rounding formula of the contract, ((v.astype(f8) * r) * c).astype(T).
"""
import functools

import numpy as np
from scipy import sparse

from tests import spmm_cases as sc

FACTORS = np.array([0.5, 1.0, 2.0])
KS = (1, 4, 16, 128)
U = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53, 'bf16': 2.0 ** -24}  # of A's values
NP_DTYPE = {'f32': np.float32, 'f64': np.float64}

# -- the exactness budget, asserted the way spmm_cases states its own --------
_UNIT = 0.125
_MAX_SCALED = float(np.abs(sc.EXACT_VALS).max() * FACTORS.max() ** 2)
_MAX_PRODUCT = _MAX_SCALED * 8
_LONGEST = max(sc.std_row_lengths())
assert _LONGEST == 4097
assert _MAX_SCALED == 8.0 and _MAX_PRODUCT == 64.0
assert all(float(v * r * c / _UNIT).is_integer()
           for v in sc.EXACT_VALS for r in FACTORS for c in FACTORS)
assert _LONGEST * _MAX_PRODUCT / _UNIT < 2 ** 24


# ---------------------------------------------------------------------------
# structures
# ---------------------------------------------------------------------------

def _empty():
    """A structure of 5 rows with no nonzero at all."""
    return dict(rows=5, n0=7, n1=0, indptr=np.zeros(6, dtype=np.int64),
                cols=np.zeros(0, dtype=np.int32),
                vals=np.zeros(0, dtype=np.float32), real_vals=None)


@functools.lru_cache(maxsize=None)
def matrix(name):
    return _empty() if name == 'empty' else sc.matrix(name)


def case(name, matrix, kind='exact', row_ids=False):
    return dict(name=name, matrix=matrix, kind=kind, row_ids=row_ids)


CASES = [case('std', 'std'), case('std_dual', 'std_dual'),
         case('std_rowids', 'std', row_ids=True),
         case('dual_rowids', 'std_dual', row_ids=True),
         case('real', 'real', kind='real'),
         case('real_rowids', 'real', kind='real', row_ids=True),
         case('empty', 'empty')]


def out_rows(c):
    m = matrix(c['matrix'])
    return m['rows'] + 37 if c['row_ids'] else m['rows']


def row_ids(c):
    """Permuted, gapped output rows: a duplicate-free scatter of the structure
    rows into a larger output (spmm_cases.row_ids' draw)."""
    if not c['row_ids']:
        return None
    rng = np.random.default_rng(77)
    return rng.permutation(out_rows(c))[:matrix(c['matrix'])['rows']] \
        .astype(np.int64)


def nnz_rows(c):
    """Output row of every stored nonzero."""
    m = matrix(c['matrix'])
    r = np.repeat(np.arange(m['rows'], dtype=np.int64), np.diff(m['indptr']))
    rid = row_ids(c)
    return r if rid is None else rid[r]


def n1(c):
    return max(matrix(c['matrix'])['n1'], 1)


def values(c, prec):
    return matrix(c['matrix'])['vals'].astype(NP_DTYPE[prec])


def factors(c):
    """(r, c0, c1): float64 scale vectors of out_rows, n0 and n1 entries."""
    m = matrix(c['matrix'])
    rng = np.random.default_rng([1007, sum(map(ord, c['name']))])
    shapes = (out_rows(c), m['n0'], n1(c))
    if c['kind'] == 'real':
        return tuple(rng.uniform(0.25, 4.0, s) for s in shapes)
    return tuple(FACTORS[rng.integers(0, FACTORS.size, s)] for s in shapes)


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------

def host_sums(c, prec, absolute, vals=None):
    """(row_sum, col_sum0, col_sum1) in float64 by np.add.at (sequential)."""
    m = matrix(c['matrix'])
    v = (values(c, prec) if vals is None else vals).astype(np.float64)
    if absolute:
        v = np.abs(v)
    cols = m['cols'].astype(np.int64)
    pos = cols >= 0
    row = np.zeros(out_rows(c))
    c0, c1 = np.zeros(m['n0']), np.zeros(n1(c))
    np.add.at(row, nnz_rows(c), v)
    np.add.at(c0, cols[pos], v[pos])
    np.add.at(c1, -cols[~pos] - 1, v[~pos])
    return row, c0, c1


def sum_bound(c, prec, vals=None):
    """Per entry of (row_sum, col_sum0, col_sum1): a double sum of n terms in
    any order errs by at most n * 2**-53 * sum|v|."""
    m = matrix(c['matrix'])
    cols = m['cols'].astype(np.int64)
    pos = cols >= 0
    mags = host_sums(c, prec, True, vals)
    counts = (np.bincount(nnz_rows(c), minlength=out_rows(c)),
              np.bincount(cols[pos], minlength=m['n0']),
              np.bincount(-cols[~pos] - 1, minlength=n1(c)))
    return tuple(n * 2.0 ** -53 * s for n, s in zip(counts, mags))


def scaled_values(c, prec, r=None, c0=None, c1=None):
    """The rounding formula of the contract: ((v.astype(f8) * r) * c)
    .astype(T), None being the factor 1."""
    m = matrix(c['matrix'])
    v = values(c, prec)
    cols = m['cols'].astype(np.int64)
    pos = cols >= 0
    rf = np.ones(v.size) if r is None else r[nnz_rows(c)]
    cf = np.ones(v.size)
    if c0 is not None:
        cf[pos] = c0[cols[pos]]
    if c1 is not None:
        cf[~pos] = c1[-cols[~pos] - 1]
    return ((v.astype(np.float64) * rf) * cf).astype(v.dtype)


def operands(c, k):
    """(X0, X1): integers in [-8, 8] (exact) or spmm_cases.real_values, as
    float64 arrays; the driver casts them to the feature type."""
    m = matrix(c['matrix'])
    rng = np.random.default_rng([k, sum(map(ord, c['name']))])
    shapes = [(m['n0'], k), (n1(c), k)]
    if c['kind'] == 'real':
        return tuple(sc.real_values(rng, s).astype(np.float64) for s in shapes)
    return tuple(rng.integers(-8, 9, s).astype(np.float64) for s in shapes)


def product(c, vals, X0, X1):
    """(output rows, vals-weighted A @ [X0; X1] in float64), one row per
    structure row."""
    m = matrix(c['matrix'])
    cols = m['cols'].astype(np.int64)
    cols = np.where(cols < 0, m['n0'] - cols - 1, cols)
    A = sparse.csr_matrix((vals.astype(np.float64), cols, m['indptr']),
                          shape=(m['rows'], m['n0'] + n1(c)))
    rid = row_ids(c)
    rows = rid if rid is not None else np.arange(m['rows'])
    return rows, np.asarray(A @ np.vstack([X0, X1]))


# ---------------------------------------------------------------------------
# engine-level bounds
# ---------------------------------------------------------------------------

def normalised_bound(prec, n):
    """|sum - 1| of a normalised nonnegative row (column) of n stored values:
    one rounding to T per value, u_T in all since the exact quotients sum to
    1, plus n * 2**-53 for the double sums and the double quotient."""
    return U[prec] + n * 2.0 ** -53
