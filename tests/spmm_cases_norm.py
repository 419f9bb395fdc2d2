"""Inputs, references, bounds and case lists of the step-norm tests
(test_spmm_cases_norm.py on the CPU; norm_driver.py /
test_gpu_norm_kernels.py on the GPU):

    acc[0] += sum (c - d)^2        acc[1] += sum c^2

over every element of every output row the structure writes, c the value as
stored in C (bf16: after its one rounding), d the stored value of D[row], D
shaped like C and indexed by output row, D = NULL meaning d = 0. c - d is
formed in the accumulator type, squares and sums are double.

Everything but D comes from tests/spmm_cases_affine.py, unchanged; the cases
run at beta 0 only (the entry points refuse any other). This module imports
numpy (and, through spmm_cases_bf16, torch's CPU casts) only.

Exact class (fp32 and bf16 features). The affine result is a multiple of
0.25 below 2**20 quarter-units (spmm_cases_affine), and rounding it to bf16
keeps it a multiple of 0.25; D holds integers in [-8, 8]. So c and c - d are
multiples of 2**-2 below 2**19: c - d is exact in fp32's 24 bits, each square
is a multiple of 2**-4 below 2**38, and as long as a total stays below 2**53
units of 2**-4 every partial sum, in any order, is exact in double: the two
accumulators must equal exact_sums bit for bit, whatever order the atomics
land in. test_spmm_cases_norm.py checks the 2**53 on the cases used.

Real class and all float64: norm_bound.
"""
import functools
import math

import numpy as np

from tests import spmm_cases as sc
from tests import spmm_cases_affine as sa
from tests import spmm_cases_bf16 as s16
from tests import spmm_cases_f64 as s64

GRID, QBLOCK, QWAVE = sa.GRID, sa.QBLOCK, sa.QWAVE
PRECISIONS = sa.PRECISIONS
ENVS = sa.ENVS
K_VARIANT, K_REAL = sa.K_VARIANT, sa.K_REAL
ks = sa.ks

# the two pairs of the sweep: an affine step with a residual, and the plain
# product through the measuring entry point
PAIRS = (sa.EXACT_PAIRS[0], sa.EXACT_PAIRS[2])
UNIT = 16  # exact class: values in units of 2**-4


def operand_D(prec, case):
    """D, shaped like C0 (indexed by OUTPUT row). Exact class: integers in
    [-8, 8]; real class: the precision's real values, as R is drawn."""
    _, _, C0, _ = sa.operands(prec, dict(case, beta=0))
    rng = np.random.default_rng([1006] + sc._seed(dict(case, beta=0)))
    if case['kind'] == 'real':
        D = s64.real_values(rng, C0.shape)
        if prec != 'f64':
            D = D.astype(np.float32)
        if prec == 'bf16':
            D = s16.to_bf16_valued(D)
        return D
    return rng.integers(-8, 9, C0.shape).astype(C0.dtype)


def stored(prec, ref):
    """The float64 reference as the precision stores it (exact class: fp32
    holds it as it is, bf16 rounds it once)."""
    if prec == 'bf16':
        return s16.to_bf16_valued(ref.astype(np.float32)).astype(np.float64)
    if prec == 'f32':
        return ref.astype(np.float32).astype(np.float64)
    return np.asarray(ref, dtype=np.float64)


def exact_units(c, d):
    """(sum (c - d)^2, sum c^2) as Python ints in units of 2**-8 (the square
    of 2**-4), for arrays whose values are multiples of 2**-4. d None: 0."""
    cu = np.rint(np.asarray(c, dtype=np.float64) * UNIT).astype(np.int64)
    assert (cu == np.asarray(c, dtype=np.float64) * UNIT).all()
    du = np.zeros_like(cu) if d is None else \
        np.rint(np.asarray(d, dtype=np.float64) * UNIT).astype(np.int64)
    assert int(np.abs(cu).max(initial=0)) < 2 ** 27  # squares fit int64 rows
    cu, du = cu.reshape(len(cu), -1), du.reshape(len(du), -1)
    tot = lambda a: sum(int(v) for v in (a * a).sum(axis=1))
    return tot(cu - du), tot(cu)


def exact_sums(c, d):
    """exact_units as the two doubles the accumulators must hold."""
    u0, u1 = exact_units(c, d)
    assert u0 < 2 ** 53 and u1 < 2 ** 53
    return u0 / float(UNIT * UNIT), u1 / float(UNIT * UNIT)


def host_sums(c, d):
    """The two sums over float64 arrays c, d (None: 0), summed in extended
    precision and rounded once: the reference of the bounded comparisons."""
    c = np.asarray(c, dtype=np.float64).astype(np.longdouble)
    # c - d of two float64 is not exact in general: extended precision too
    diff = c if d is None else c - np.asarray(d).astype(np.longdouble)
    sq = lambda a: float((a * a).sum())
    return sq(diff), sq(c)


def norm_bound(prec, n_terms, s0, s1):
    """Absolute bounds on the two accumulators against host_sums, derived:
    each term of acc[0] is fl_Acc(c - d)^2, the difference carrying one
    rounding of the accumulator type (relative u = 2**-24, or 2**-53 for
    float64), hence (1 + u)^2 on its square: the 2 u; the square is rounded
    once to double (e = 2**-53; exact for fp32 and bf16 values, counted
    anyway); summing N non-negative terms in any order multiplies each by at
    most (1 + e)^(N - 1). So |acc[0] - s0| <= ((1 + u)^2 (1 + e)^N - 1) s0,
    and without the difference |acc[1] - s1| <= ((1 + e)^N - 1) s1. The
    reference's own rounding (one, of an extended-precision sum) adds e.
    Derived, not measured."""
    u = 2.0 ** -53 if prec == 'f64' else 2.0 ** -24
    e = 2.0 ** -53
    n = max(int(n_terms), 1)
    rel1 = math.expm1(n * math.log1p(e)) + e
    rel0 = math.expm1(2 * math.log1p(u) + n * math.log1p(e)) + e
    return rel0 * s0, rel1 * s1


# ---------------------------------------------------------------------------
# case lists
# ---------------------------------------------------------------------------

def case(name, matrix, kind, k, queue, pair, **opts):
    return sa.case(name, matrix, kind, k, 0, queue, pair, **opts)


@functools.lru_cache(maxsize=None)
def gpu_cases(prec, env):
    """The cases of one (precision, environment) child, all at beta 0: every
    case runs grid-stride (queue 0) and queued (queue 1: the scheduler the
    environment selects)."""
    cs = []
    for matrix in ('std', 'std_dual'):
        for k in ks(prec):
            for pair in PAIRS:
                for q in (0, 1):
                    cs.append(case(f'{matrix}_k{k}_{sa._pair_tag(pair)}_q{q}',
                                   matrix, 'exact', k, q, pair))
    pair = PAIRS[0]
    for k in K_VARIANT[prec]:
        for q in (0, 1):
            tag = f'k{k}_q{q}'
            # the rows the structure does not write hold NaN: counting one
            # would poison the sums
            cs.append(case(f'rowids_{tag}', 'std', 'exact', k, q, pair,
                           row_ids=True))
            cs.append(case(f'col1_{tag}', 'std', 'exact', k, q, pair,
                           col_items=1))
            cs.append(case(f'col2_{tag}', 'std_dual', 'exact', k, q, pair,
                           col_items=2))
            cs.append(case(f'dnull_{tag}', 'std', 'exact', k, q, pair,
                           D='null'))
            cs.append(case(f'dalias_{tag}', 'std', 'exact', k, q, pair,
                           D='alias'))
        cs.append(case(f'qb8_k{k}', 'std', 'exact', k, 1, pair, qblocks=8))
        cs.append(case(f'twice_k{k}', 'std', 'exact', k, 1, pair, twice=True))
    for k in K_REAL[prec]:
        for q in (0, 1):
            cs.append(case(f'real_k{k}_q{q}', 'real', 'real', k, q,
                           sa.REAL_PAIR))
    if env == 'default':
        # 1025 split rows x k = 1024: the split-row pass (bf16: the finalise
        # pass) past its 4096 x 256 grid cap
        cs.append(case('zero_rows_k1024', 'zero_rows', 'exact', 1024, 0, pair,
                       init_capped=True))
    return tuple(cs)


expected_scheduler = sa.expected_scheduler
DIFFNORM_SHAPES = sa.AXPBY_SHAPES


def diffnorm_case(prec, n, k):
    """(C, D): integers in [-8, 8], exact in every precision."""
    rng = np.random.default_rng([1006, n, k])
    dt = np.float64 if prec == 'f64' else np.float32
    return (rng.integers(-8, 9, (n, k)).astype(dt),
            rng.integers(-8, 9, (n, k)).astype(dt))
