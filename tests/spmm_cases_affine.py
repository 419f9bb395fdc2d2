"""Inputs, references and case lists of the affine-step tests
(test_spmm_cases_affine.py on the CPU; affine_driver.py /
test_gpu_affine_kernels.py on the GPU):

    C[row] = alpha * (A @ X)[row] + gamma * R[row] + beta * C0[row]

The matrices (`std`, `std_dual`, `real`, `zero_rows`), `row_ids` and the
operands X0, X1, C0 come from tests/spmm_cases.py and the case modules of the
three precisions, unchanged. This module imports numpy/scipy (and, through
spmm_cases_bf16, torch's CPU casts) only: it never touches the GPU.

Exact class. A holds +-0.5 / +-1 / +-2, X and C0 integers in [-8, 8] (float64:
i + j * 2**-30, see spmm_cases_f64), R integers in [-8, 8], and (alpha, gamma)
come from EXACT_PAIRS: powers of two of magnitude 0.5 .. 2, or 0, or 1. A row
of up to 8192 products is a multiple of 0.5 below 2**17; alpha scales it to a
multiple of 0.25 below 2**18, gamma * R is a multiple of 0.5 of magnitude
<= 16, C0 an integer <= 8: every term and every partial sum, in any order, is
a multiple of 0.25 below 2**20 quarter-units, exact in fp32's 24 bits (in
float64 the same count gives 2**-32 units below 2**20: 52 bits). So the
result does not depend on fma or not, nor on alpha being applied per partial
(fp32 / f64 split rows) or once (bf16 finalise), and the output must equal
the float64 reference bit for bit; bf16 outputs must equal bf16_bits of it,
the float64 result cast ONCE.
"""
import functools

import numpy as np

from tests import spmm_cases as sc
from tests import spmm_cases_bf16 as s16
from tests import spmm_cases_f64 as s64

GRID, QBLOCK, QWAVE = sc.GRID, sc.QBLOCK, sc.QWAVE
PRECISIONS = ('f32', 'f64', 'bf16')

# (alpha, gamma, R given). (1, 0, NULL) must equal the plain entry point.
EXACT_PAIRS = ((0.5, 2.0, True), (-2.0, -0.5, True), (1.0, 0.0, False),
               (0.0, 1.0, True))
REAL_PAIR = (0.85, 0.15, True)

# fp32 / f64: VEC 1, 2 and 4, an idle lane (k = 3, 36), GUARD on the last
# column tile (130, 260) and two launches (130 in f64, 260)
K_F = (1, 3, 4, 16, 36, 128, 130, 260)
K_VARIANT = {'f32': (16, 130), 'f64': (16, 130), 'bf16': (16, 520)}
K_REAL = {'f32': (36, 128), 'f64': (36, 128), 'bf16': (24, 128)}
ENVS = {
    'default': {},
    'qwave1': {'ARROW_QWAVE': '1'},
    'qwave0': {'ARROW_QWAVE': '0'},
    'nt0': {'ARROW_SPMM_NT': '0'},
}


def ks(prec):
    return s16.K_GPU if prec == 'bf16' else K_F


def _mod(prec):
    return {'f32': sc, 'f64': s64, 'bf16': s16}[prec]


# ---------------------------------------------------------------------------
# operands and references
# ---------------------------------------------------------------------------

def operands(prec, case):
    """(X0, X1, C0, R): the precision's own operands and the residual, shaped
    like C0 (indexed by OUTPUT row). Exact class: integers in [-8, 8]. Real
    class: the precision's real values (bf16: rounded to bf16 once)."""
    X0, X1, C0 = _mod(prec).operands(case)
    rng = np.random.default_rng([1005] + sc._seed(case))
    if case['kind'] == 'real':
        R = s64.real_values(rng, C0.shape)
        if prec != 'f64':
            R = R.astype(np.float32)
        if prec == 'bf16':
            R = s16.to_bf16_valued(R)
    else:
        R = rng.integers(-8, 9, C0.shape).astype(C0.dtype)
    return X0, X1, C0, R


def _rows(case, n):
    rid = sc.row_ids(case)
    return rid if rid is not None else np.arange(n)


def plain_product(prec, case, X0, X1):
    """A @ [X0; X1] over the structure rows in the reference's type: float64,
    or x87 extended precision for the float64 real class (whose own error
    must stay far below the float64 bound)."""
    c0 = dict(case, beta=0)
    if prec == 'f64':
        fn = s64.reference_longdouble if case['kind'] == 'real' \
            else s64.reference
        return fn(c0, X0, X1, None)[1]
    return sc.reference(c0, X0, X1, None, np.float64)[1]


def abs_product(prec, case, X0, X1):
    if prec == 'f64':
        return s64.product(case, X0, X1, absolute=True)
    return sc.product(case, X0, X1, np.float64, absolute=True)


def reference(prec, case, X0, X1, C0, R, product=None):
    """(touched_rows, ref): alpha * (A@X) + gamma * R (+ C0) over the
    structure rows, in output order. `product`: plain_product's result, when
    the caller shares it among the cases of one (matrix, k)."""
    P = plain_product(prec, case, X0, X1) if product is None else product
    rows = _rows(case, P.shape[0])
    ref = P.dtype.type(case['alpha']) * P
    if case['has_R']:
        ref = ref + P.dtype.type(case['gamma']) * R[rows].astype(P.dtype)
    if case['beta']:
        ref = ref + C0[rows].astype(P.dtype)
    return rows, ref


def real_bound(prec, case, X0, X1, C0, R, ref, abs_prod=None):
    """spmm_cases.real_bound extended by derivation: gamma_n = n*u/(1 - n*u)
    with n = 2*len_i + 8 roundings (the 2*len_i + 2 of the plain step, one
    more for alpha * sum, two for gamma * r and its add, and the same again
    so that it holds with fma or without), u = 2**-24 (2**-53 for float64),
    applied to |alpha| sum|a||x| + |gamma||R| + |C0|. bf16 adds the one
    rounding of the result, 2**-8 of (|ref| + the fp32 bound), as
    tests/engine_bf16_driver.py derives it. Derived, not measured."""
    m = sc.matrix(case['matrix'])
    u = 2.0 ** -53 if prec == 'f64' else 2.0 ** -24
    g = (2.0 * np.diff(m['indptr']) + 8.0) * u
    mag = abs_product(prec, case, X0, X1) if abs_prod is None else abs_prod
    rows = _rows(case, mag.shape[0])
    mag = abs(case['alpha']) * mag
    if case['has_R']:
        mag = mag + abs(case['gamma']) * np.abs(R[rows]).astype(np.float64)
    if case['beta']:
        mag = mag + np.abs(C0[rows]).astype(np.float64)
    bound = (g / (1.0 - g))[:, None] * mag
    if prec == 'bf16':
        bound = bound + 2.0 ** -8 * (np.abs(ref).astype(np.float64) + bound)
    return bound


def dense_reference(prec, case, X0, X1, C0, R):
    """The same result from a dense float64 matrix and plain numpy, for the
    CPU test of `reference`."""
    m = sc.matrix(case['matrix'])
    vals = s64.values(case['matrix'], case['kind']) if prec == 'f64' \
        else m['vals'].astype(np.float64)
    D = np.zeros((m['rows'], m['n0'] + max(m['n1'], 1)))
    c = m['cols'].astype(np.int64)
    c = np.where(c < 0, m['n0'] - c - 1, c)
    r = np.repeat(np.arange(m['rows']), np.diff(m['indptr']))
    np.add.at(D, (r, c), vals)
    out = case['alpha'] * (D @ np.vstack([X0, X1]).astype(np.float64))
    rows = _rows(case, m['rows'])
    if case['has_R']:
        out = out + case['gamma'] * R[rows].astype(np.float64)
    if case['beta']:
        out = out + C0[rows].astype(np.float64)
    return rows, out


# ---------------------------------------------------------------------------
# case lists
# ---------------------------------------------------------------------------

def case(name, matrix, kind, k, beta, queue, pair, **opts):
    alpha, gamma, has_R = pair
    c = dict(name=name, matrix=matrix, kind=kind, k=k, beta=beta, queue=queue,
             alpha=alpha, gamma=gamma, has_R=has_R)
    c.update(opts)
    return c


def _pair_tag(pair):
    return 'a%g_g%g' % pair[:2]


@functools.lru_cache(maxsize=None)
def gpu_cases(prec, env):
    """The cases of one (precision, environment) child. Every case runs
    grid-stride (queue 0) and queued (queue 1: the scheduler the environment
    selects), at beta 0 and 1."""
    cs = []
    for matrix in ('std', 'std_dual'):
        for k in ks(prec):
            for beta in (0, 1):
                for pair in EXACT_PAIRS:
                    for q in (0, 1):
                        cs.append(case(
                            f'{matrix}_k{k}_b{beta}_{_pair_tag(pair)}_q{q}',
                            matrix, 'exact', k, beta, q, pair))
    pair = EXACT_PAIRS[0]
    for k in K_VARIANT[prec]:
        for beta in (0, 1):
            for q in (0, 1):
                tag = f'k{k}_b{beta}_q{q}'
                cs.append(case(f'rowids_{tag}', 'std', 'exact', k, beta, q,
                               pair, row_ids=True))
                cs.append(case(f'col1_{tag}', 'std', 'exact', k, beta, q,
                               pair, col_items=1))
                cs.append(case(f'col2_{tag}', 'std_dual', 'exact', k, beta, q,
                               EXACT_PAIRS[1], col_items=2))
            cs.append(case(f'qb8_k{k}_b{beta}', 'std', 'exact', k, beta, 1,
                           pair, qblocks=8))
    for k in K_REAL[prec]:
        for beta in (0, 1):
            for q in (0, 1):
                cs.append(case(f'real_k{k}_b{beta}_q{q}', 'real', 'real', k,
                               beta, q, REAL_PAIR))
    if env == 'default':
        # 1025 split rows x k = 1024: the initialise pass (bf16: the finalise
        # pass) past its 4096 x 256 grid cap
        for beta in (0, 1):
            cs.append(case(f'zero_rows_k1024_b{beta}', 'zero_rows', 'exact',
                           1024, beta, 0, pair, init_capped=True))
    return tuple(cs)


def expected_scheduler(env, queue, group):
    if not queue:
        return GRID
    if env == 'qwave1':
        return QWAVE
    if env == 'qwave0':
        return QBLOCK
    return QWAVE if group < 8 else QBLOCK


# ---------------------------------------------------------------------------
# the tail kernel, C = alpha * C + gamma * R
# ---------------------------------------------------------------------------

# (n, k); the last has n * k_vec > 16384 x 256 threads, like ROUTE_SHAPES'
AXPBY_SHAPES = {
    'f32': [(n, k) for n in (0, 1, 500) for k in (1, 3, 4, 33, 128)]
    + [(33000, 129)],
    'f64': [(n, k) for n in (0, 1, 500) for k in (1, 3, 4, 33, 128)]
    + [(33000, 129)],
    'bf16': [(n, k) for n in (0, 1, 500) for k in (8, 24, 128)]
    + [(33000, 1024)],
}


def axpby_case(prec, n, k, pair):
    """(C0, R, ref): integers in [-8, 8] and an EXACT_PAIRS pair, so that
    alpha * C + gamma * R is exact in every precision (a multiple of 0.5 of
    magnitude <= 32: 7 bits, bf16 holds 8)."""
    alpha, gamma, has_R = pair
    rng = np.random.default_rng([1005, n, k])
    dt = np.float64 if prec == 'f64' else np.float32
    C0 = rng.integers(-8, 9, (n, k)).astype(dt)
    R = rng.integers(-8, 9, (n, k)).astype(dt)
    ref = alpha * C0.astype(np.float64)
    if has_R:
        ref = ref + gamma * R.astype(np.float64)
    return C0, R, ref
