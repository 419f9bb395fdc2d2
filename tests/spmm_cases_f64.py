"""Inputs, references and the expected launch-plan table of the float64 SpMM
tests (test_spmm_cases_f64.py on the CPU; spmm_driver.py /
test_gpu_f64_kernels.py on the GPU).

The matrices (`std`, `std_dual`, `real`, `stride`, `zero_rows`, `remap*`),
`row_ids` and the case layout come from tests/spmm_cases.py unchanged. This
module imports numpy/scipy only: it never touches the GPU.

Exact inputs that only true float64 reproduces: A keeps EXACT_VALS
{+-0.5, +-1, +-2}; X and C0 entries are i + j*2**-30 with integers i, j in
[-8, 8]. Every product is a multiple of 2**-31 of magnitude < 17, so a row
of up to 8192 terms plus C0 stays below 2**18: every partial sum needs at
most 18 + 31 = 49 bits and is exact in double (53-bit significand) in any
order — with or without fma, through split-row atomics and beta=1. The
kernel output must equal the float64 reference bit for bit. None of it is
representable in fp32 (i + j*2**-30 needs up to 34 bits), so any float
staging of X, A or an accumulator breaks bit equality.
"""
import functools

import numpy as np

from tests import spmm_cases as sc

GRID, QBLOCK, QWAVE = sc.GRID, sc.QBLOCK, sc.QWAVE

# k -> (vec, group, launches) with no variables set, written out by hand:
# vec = 2 doubles per lane when k is even, else 1; group = the power of two
# >= ceil(k / vec), capped at 64; launches = ceil(k / (vec * group)).
PLAN_TABLE = {
    1: (1, 1, 1), 2: (2, 1, 1), 3: (1, 4, 1), 4: (2, 2, 1), 5: (1, 8, 1),
    6: (2, 4, 1), 7: (1, 8, 1), 8: (2, 4, 1), 12: (2, 8, 1), 16: (2, 8, 1),
    32: (2, 16, 1), 33: (1, 64, 1), 64: (2, 32, 1), 100: (2, 64, 1),
    128: (2, 64, 1), 129: (1, 64, 3), 130: (2, 64, 2), 256: (2, 64, 2),
    260: (2, 64, 3),
}
K_ALL = tuple(PLAN_TABLE)
# used by one case only (zero_rows): 8 launches of 64 lanes x 2
PLAN_EXTRA = {1024: (2, 64, 8)}

FRAC = 2.0 ** -30


def vec_group_launches(k):
    return PLAN_TABLE[k] if k in PLAN_TABLE else PLAN_EXTRA[k]


# spmm_cases' plan, default_queued and policy, on this table
plan = functools.partial(sc.plan, lookup=vec_group_launches)
default_queued = functools.partial(sc.default_queued,
                                   lookup=vec_group_launches)
policy = functools.partial(sc.policy, lookup=vec_group_launches)


# ---------------------------------------------------------------------------
# operands and references
# ---------------------------------------------------------------------------

def real_values(rng, shape):
    """Magnitudes uniform in [0.25, 1], random sign, drawn as double."""
    return rng.uniform(0.25, 1.0, shape) * rng.choice([-1.0, 1.0], shape)


@functools.lru_cache(maxsize=None)
def values(matrix, kind):
    """A's float64 values on the pattern of spmm_cases.matrix(matrix)."""
    m = sc.matrix(matrix)
    if kind == 'real':
        rng = np.random.default_rng([64, sum(map(ord, matrix))])
        v = real_values(rng, m['vals'].size)
    else:
        v = m['vals'].astype(np.float64)     # EXACT_VALS, exact in double
    v.setflags(write=False)
    return v


def exact_values(rng, shape):
    i = rng.integers(-8, 9, shape).astype(np.float64)
    j = rng.integers(-8, 9, shape).astype(np.float64)
    return i + j * FRAC


def operands(case):
    """(X0, X1, C0) float64; C0 has the output's shape (used at beta=1)."""
    m = sc.matrix(case['matrix'])
    k = case['k']
    rng = np.random.default_rng([64] + sc._seed(case))
    shapes = [(m['n0'], k), (max(m['n1'], 1), k), (sc.out_rows(case), k)]
    draw = real_values if case['kind'] == 'real' else exact_values
    return tuple(draw(rng, s) for s in shapes)


def product(case, X0, X1, dtype=np.float64, absolute=False):
    """A @ [X0; X1] over the structure rows, accumulated in `dtype`."""
    m = sc.matrix(case['matrix'])
    vals = values(case['matrix'], case['kind'])
    X = np.vstack([X0, X1]).astype(dtype)
    if absolute:
        vals, X = np.abs(vals), np.abs(X)
    return np.asarray(sc._csr(m, vals, dtype) @ X)


def _rows(case, n):
    rid = sc.row_ids(case)
    return rid if rid is not None else np.arange(n)


def reference(case, X0, X1, C0):
    """(touched_rows, ref) in float64; exact for the exact-valued cases."""
    ref = product(case, X0, X1)
    rows = _rows(case, ref.shape[0])
    if case['beta']:
        ref = ref + C0[rows]
    return rows, ref


def reference_longdouble(case, X0, X1, C0):
    """The real-valued reference, accumulated in x87 extended precision
    (u = 2**-64): its own error is below 2**-10 of real_bound, which the
    factor two in real_bound's n covers."""
    assert np.finfo(np.longdouble).nmant >= 63
    m = sc.matrix(case['matrix'])
    vals = values(case['matrix'], case['kind']).astype(np.longdouble)
    X = np.vstack([X0, X1]).astype(np.longdouble)
    c = m['cols'].astype(np.int64)
    c = np.where(c < 0, m['n0'] - c - 1, c)
    ref = np.zeros((m['rows'], X.shape[1]), dtype=np.longdouble)
    prod = vals[:, None] * X[c]
    nonempty = np.flatnonzero(np.diff(m['indptr']))
    ref[nonempty] = np.add.reduceat(prod, m['indptr'][nonempty], axis=0)
    rows = _rows(case, ref.shape[0])
    if case['beta']:
        ref = ref + C0[rows].astype(np.longdouble)
    return rows, ref


def real_bound(case, X0, X1, C0):
    """spmm_cases.real_bound's derivation with u = 2**-53: gamma_n =
    n*u/(1 - n*u), n = 2*len_i + 2 (one rounding per product and per add,
    doubled so that it holds with or without fma), applied to
    sum|a||x| + |C0|. Derived, not measured."""
    m = sc.matrix(case['matrix'])
    g = (2.0 * np.diff(m['indptr']) + 2.0) * 2.0 ** -53
    mag = product(case, X0, X1, absolute=True)
    if case['beta']:
        mag = mag + np.abs(C0[_rows(case, mag.shape[0])])
    return (g / (1.0 - g))[:, None] * mag


# ---------------------------------------------------------------------------
# the environment -> case table
# ---------------------------------------------------------------------------

# spmm_cases' builders, with this module's plan
case = sc.case
_sweep = functools.partial(sc._sweep, plan=plan)
_variants = functools.partial(sc._variants, plan=plan)
_real_case = sc._real_case


VARIANT_KS = (8, 64, 130)


def _env(tag, sched_of, **pl):
    """Every k of the table at beta 0 and 1, grid-stride and queued, plus
    the variants at k in VARIANT_KS."""
    cs = _sweep(f'{tag}_grid', K_ALL, 0, lambda k: GRID, **pl)
    cs += _sweep(f'{tag}_queued', K_ALL, 1, sched_of, **pl)
    for k in VARIANT_KS:
        cs += _variants(tag, k, sched_of, **pl)
    return cs


def _env_default():
    cs = _env('default', default_queued)
    cs += _sweep('mode-1', (16, 128), None, lambda k: GRID)  # nnz < Q_MIN_NNZ
    # 40 000 items at GROUP 64 (4 groups per block): past the 8192-block cap
    for beta in (0, 1):
        cs.append(case(f'grid_stride_beyond_cap_b{beta}', 128, beta, 0,
                       plan(128, GRID), matrix='stride', remap='both',
                       capped_groups_per_block=4))
    # k=64 is GROUP 32 (8 groups per block): gridDim.x = 33, 37, 39
    for r in sorted(sc.REMAP_ITEMS):
        cs.append(case(f'xcd_remap_grid_mod8_{r}', 64, (r // 2) % 2, 0,
                       plan(64, GRID), matrix=f'remap{r}', remap='both',
                       grid_mod8=r))
    cs.append(case('zero_rows_beyond_cap', 1024, 0, 0, plan(1024, GRID),
                   matrix='zero_rows', zero_rows_capped=True))
    cs.append(_real_case('default', 64, 1, plan(64, QBLOCK)))
    return cs


@functools.lru_cache(maxsize=None)
def env_table():
    """name -> (variables, cases). One fresh child process per entry."""
    return {
        'default': ({}, _env_default()),
        'qwave1': ({'ARROW_QWAVE': '1'},
                   _env('qwave1', lambda k: QWAVE)
                   + [_real_case('qwave1', 128, 1, plan(128, QWAVE))]),
        'qwave0': ({'ARROW_QWAVE': '0'},
                   _env('qwave0', lambda k: QBLOCK)
                   + [_real_case('qwave0', 8, 1, plan(8, QBLOCK))]),
        'nt0': ({'ARROW_SPMM_NT': '0'},
                _env('nt0', default_queued, nt=0)
                + [_real_case('nt0', 130, 0, plan(130, GRID, nt=0))]),
    }


# ---------------------------------------------------------------------------
# route / permute kernels
# ---------------------------------------------------------------------------

def route_case(op, n, k):
    """spmm_cases.route_case in float64: operands drawn as double, the numpy
    fancy-indexing reference bit for bit (one double add per element is the
    same on both sides)."""
    return sc.route_case(op, n, k, draw=real_values, seed_prefix=[64],
                         add=np.add)
