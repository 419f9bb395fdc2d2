"""Inputs, references and the expected launch-plan table of the bfloat16-
feature SpMM tests (test_spmm_cases_bf16.py on the CPU; spmm_driver.py /
test_gpu_bf16_kernels.py on the GPU).

The matrices (`std`, `std_dual`, `real`, `stride`, `zero_rows`), `row_ids`
and the case layout come from tests/spmm_cases.py unchanged. This module
imports numpy/scipy and torch's CPU casts only: it never touches the GPU.

Exact class: A keeps EXACT_VALS {+-0.5, +-1, +-2} (fp32, as resident); X and
C0 hold integers in [-8, 8], all exact in bf16. Every product is a multiple
of 0.5 of magnitude <= 16, so a row of up to 8192 terms (plus C0) stays below
2**18 half-units and every partial sum, in every order, is exact in fp32.
The output must therefore equal bf16_RNE(C0*beta + A@X), the float64 result
cast ONCE, bit for bit, ties included. The long rows of `std` (2049, 4097
nonzeros) reach sums of a few hundred half-units, far past the 8 significant
bits of bf16: an implementation that rounds per segment, per atomic or per
column tile lands on other bits.
"""
import functools

import numpy as np
import torch

from tests import spmm_cases as sc

GRID, QBLOCK, QWAVE = sc.GRID, sc.QBLOCK, sc.QWAVE

# k -> (vec, group, launches) with no variables set, written out by hand:
# vec = 8 bf16 per lane; group = the power of two >= k / 8, capped at 64;
# launches = ceil(k / (8 * group)).
PLAN_TABLE = {
    8: (8, 1, 1), 16: (8, 2, 1), 24: (8, 4, 1), 32: (8, 4, 1),
    40: (8, 8, 1), 64: (8, 8, 1), 128: (8, 16, 1), 256: (8, 32, 1),
    264: (8, 64, 1), 512: (8, 64, 1), 520: (8, 64, 2), 1024: (8, 64, 2),
}
K_BAD = (4, 12, 129)            # not a multiple of 8: refused
# the GPU cases: GROUP 1 and 2; an idle lane; k=128; two launches with GUARD
# on the last
K_GPU = (8, 16, 24, 128, 520)


def vec_group_launches(k):
    return PLAN_TABLE[k]


# spmm_cases' plan, default_queued and policy, on this table
plan = functools.partial(sc.plan, lookup=vec_group_launches)
default_queued = functools.partial(sc.default_queued,
                                   lookup=vec_group_launches)
policy = functools.partial(sc.policy, lookup=vec_group_launches)


# ---------------------------------------------------------------------------
# bf16 <-> numpy. A bf16 array travels as its raw bits (uint16).
# ---------------------------------------------------------------------------

def bf16_bits(a):
    """Raw bits of `a` cast to bf16 once, with torch's cast (round to
    nearest even). `a` is float32, or float64 holding values that are exact
    in float32 (so that torch's double -> float -> bf16 path rounds once)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        a32 = a.astype(np.float32)
        assert (a32.astype(np.float64) == a).all(), \
            "the round-once oracle needs values that float32 holds exactly"
        a = a32
    assert a.dtype == np.float32
    return torch.from_numpy(a).to(torch.bfloat16).view(torch.int16) \
        .numpy().view(np.uint16)


def bf16_bits_by_hand(a32):
    """The same rounding written out on the float32 bit pattern: keep the
    top 16 bits; round up when the dropped half is above 0x8000, or equal to
    it and the kept part is odd. Finite inputs only."""
    u = np.ascontiguousarray(a32, dtype=np.float32).view(np.uint32)
    low = u & 0xffff
    keep = u >> 16
    up = (low > 0x8000) | ((low == 0x8000) & ((keep & 1) == 1))
    return (keep + up).astype(np.uint16)


def bf16_to_f64(bits):
    """The value of raw bf16 bits, as float64 (exact)."""
    b = np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16
    return b.view(np.float32).astype(np.float64)


def to_bf16_valued(a32):
    """float32 -> the float32 array of its bf16 roundings."""
    return bf16_to_f64(bf16_bits(a32)).astype(np.float32)


# ---------------------------------------------------------------------------
# operands and references
# ---------------------------------------------------------------------------

def operands(case):
    """(X0, X1, C0) as float32 arrays of bf16-representable values. Exact
    class: spmm_cases' integers in [-8, 8]. Real class: its magnitudes in
    [0.25, 1], rounded to bf16 once here (the operands ARE bf16 values)."""
    ops = sc.operands(case)
    if case['kind'] == 'real':
        ops = tuple(to_bf16_valued(o) for o in ops)
    for o in ops:
        assert (to_bf16_valued(o) == o).all()
    return ops


def reference(case, X0, X1, C0):
    """(touched_rows, G): the float64 product of the operands (+ C0 at
    beta=1) over the structure rows; exact for the exact class."""
    return sc.reference(case, X0, X1, C0, np.float64)


def real_bound(case, X0, X1, C0, G):
    """|C - G| <= 2**-8 |G| + (n_row + segments + 2) 2**-24 (|A|@|X| + |C0|):
    one round-to-nearest to bf16 (unit roundoff 2**-8), and the fp32 fma
    chain of n_row terms plus one add per split-row segment and the beta
    add. Derived, not measured; no element is exempt."""
    m = sc.matrix(case['matrix'])
    lens = np.diff(m['indptr'])
    segs = np.maximum(1, -(-lens // sc.SEG_NNZ))
    mag = sc.product(case, X0, X1, np.float64, absolute=True)
    if case['beta']:
        rid = sc.row_ids(case)
        rows = rid if rid is not None else np.arange(mag.shape[0])
        mag = mag + np.abs(C0[rows]).astype(np.float64)
    return 2.0 ** -8 * np.abs(G) + \
        ((lens + segs + 2.0) * 2.0 ** -24)[:, None] * mag


# ---------------------------------------------------------------------------
# the environment -> case table
# ---------------------------------------------------------------------------

# spmm_cases' builders, with this module's plan; of the std-case variants,
# std_dual and the row_ids scatter only
case = sc.case
VARIANTS = ('dual', 'rowids')
_sweep = functools.partial(sc._sweep, plan=plan)
_variants = functools.partial(sc._variants, plan=plan, variants=VARIANTS)
_real_case = sc._real_case


def _env_default():
    grid = lambda k: GRID
    cs = _sweep('grid', K_GPU, 0, grid)
    cs += _sweep('queued', K_GPU, 1, default_queued)
    for k in (16, 128, 520):
        cs += _variants('default', k, default_queued)
    # the same split-row case twice: identical bits (sums exact in fp32)
    cs.append(case('repeat_k128_b1', 128, 1, 1, plan(128, QBLOCK),
                   repeat=True))
    # 40 000 items at GROUP 64 (4 groups per block): past the 8192-block cap
    for beta in (0, 1):
        cs.append(case(f'grid_stride_beyond_cap_b{beta}', 520, beta, 0,
                       plan(520, GRID), matrix='stride', remap='both',
                       capped_groups_per_block=4))
    # 1025 split rows, two column-tiled launches, one finalise over both
    cs.append(case('zero_rows_k1024', 1024, 0, 0, plan(1024, GRID),
                   matrix='zero_rows'))
    cs.append(_real_case('grid', 128, 0, plan(128, GRID), beta=0))
    cs.append(_real_case('queued', 24, 1, plan(24, QWAVE)))
    return cs


@functools.lru_cache(maxsize=None)
def env_table():
    """name -> (variables, cases). One fresh child process per entry: the
    ARROW_* kernel variables are read once per process."""
    wave, block = (lambda k: QWAVE), (lambda k: QBLOCK)
    return {
        'default': ({}, _env_default()),
        'qwave1': ({'ARROW_QWAVE': '1'},
                   _sweep('qwave1', K_GPU, 1, wave)
                   + _variants('qwave1', 128, wave)
                   + [_real_case('qwave1', 128, 1, plan(128, QWAVE))]),
        'qwave0': ({'ARROW_QWAVE': '0'},
                   _sweep('qwave0', K_GPU, 1, block)
                   + _variants('qwave0', 16, block)
                   + [_real_case('qwave0', 8, 1, plan(8, QBLOCK))]),
    }


# ---------------------------------------------------------------------------
# route / permute kernels
# ---------------------------------------------------------------------------

# (n, k); the last has n * k / 8 = 4 224 000 > 16384 x 256 threads
ROUTE_SHAPES = [(n, k) for n in (0, 1, 500) for k in (8, 128)] \
    + [(33000, 1024)]


def route_case(op, n, k):
    """spmm_cases.route_case on bf16 operands, as raw bits. The copies must
    match fancy indexing bit for bit; the adding forms must equal
    bf16_RNE(float(dst) + float(src)): the fp32 sum of two bf16 values,
    rounded once."""
    rc = sc.route_case(
        op, n, k, seed_prefix=[16],
        draw=lambda rng, shape: to_bf16_valued(sc.real_values(rng, shape)),
        add=lambda dst, src: to_bf16_valued(dst + src))       # fp32 add
    return dict(rc, src=bf16_bits(rc['src']), dst0=bf16_bits(rc['dst0']),
                ref=bf16_bits(rc['ref']))
