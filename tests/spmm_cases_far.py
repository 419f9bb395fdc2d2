"""The far geometry: the existing kernel cases, placed so that the element
offsets the kernels form cross 2**31 elements (and the byte offsets 4 GiB).
test_spmm_cases_far.py checks the geometry on the CPU; far_driver.py /
test_gpu_far_offsets.py run it on the GPU.

A far case is a compact case plus a placement. The compact case (matrices
`std` / `std_dual`, operands, `row_ids`, pairs, `operand_D`, `route_case`,
references) is the one of tests/spmm_cases*.py, unchanged, and its reference
is computed on the compact arrays by those modules and compared bit for bit
(exact class only). The placement puts one side of the call into a TALL
buffer, at a window of rows that straddles the boundary B = 2**31 elements:
with r_B = ceil(B / k), a window of W rows starts at row r_B - W // 2.

    far-read    A's columns are shifted (cols + base0 reads X0, -(idx + base1
                + 1) reads X1); both windows lie in ONE tall read buffer, X1's
                after X0's with GAP_ROWS rows between them. C, R, D compact.
    far-write   row_ids = out_base + spmm_cases.row_ids(case), so C is tall;
                R (and D = R, which the entry points allow) is indexed by
                output row like C and lives at the same rows of ONE second
                tall buffer. X0, X1 compact.

A tall buffer ends one guard pad (PAD words, as spmm_driver.guarded) after
its last window.

What the geometry can and cannot show. Every touched element offset at or
past B is below 2**32, so a product formed in `int` wraps to a negative
offset, outside every window; a byte offset (at least 2 bytes per element)
formed in 32 bits, signed or unsigned, lands outside the window too. An
element offset formed in `unsigned` does not wrap below 2**32 elements, and
neither does an index counted in 16-byte vectors (idx * k_vec with k_vec =
k / 4): windows across 2**32 elements would double every buffer, and are not
built.

This module imports numpy (and, through spmm_cases_bf16, torch's CPU casts)
only: it never touches the GPU.
"""
import functools

import numpy as np

from tests import spmm_cases as sc
from tests import spmm_cases_affine as sa
from tests import spmm_cases_norm as sn

B = 2 ** 31               # elements
PAD = 64                  # spmm_driver.PAD: guard words around every buffer
GAP_ROWS = 16             # NaN rows between the X0 and the X1 window
PRECISIONS = sa.PRECISIONS
ITEMSIZE = {'f32': 4, 'f64': 8, 'bf16': 2}
WORDSIZE = {'f32': 4, 'f64': 4, 'bf16': 2}     # of spmm_driver's guard words

# f32: VEC 1, VEC 4, GUARD on the last tile, two launches; f64: 130 is two
# launches; bf16: 520 is two launches
K = {'f32': (3, 16, 130, 260), 'f64': (3, 16, 130), 'bf16': (16, 520)}
TWO_LAUNCHES = {'f32': 260, 'f64': 130, 'bf16': 520}
ROLES = ('read', 'write')
MATRIX = {'read': 'std_dual', 'write': 'std'}
# (entry point, beta, (alpha, gamma, R given))
ENTRIES = (('spmm', 0, sa.EXACT_PAIRS[2]), ('spmm', 1, sa.EXACT_PAIRS[2]),
           ('affine', 0, sa.EXACT_PAIRS[0]), ('affine', 1, sa.EXACT_PAIRS[0]),
           ('norm', 0, sn.PAIRS[0]))

ROUTE_N = 500
ROUTE_K = {'f32': (33, 128), 'f64': (33, 128), 'bf16': (24, 128)}
ROUTE_SIDES = ('src', 'dst')

_N129 = -(-B // 129) + 3
CONTIG_SHAPES = {'f32': ((2 ** 24 + 3, 128), (_N129, 129)),
                 'f64': ((2 ** 24 + 3, 128), (_N129, 129)),
                 'bf16': ((2 ** 24 + 3, 128),)}
CONTIG_KERNELS = ('axpby', 'diffnorm')
# f64 keeps ONE tall buffer: axpby without R, diffnorm without D
CONTIG_PAIR = {'f32': sa.EXACT_PAIRS[0], 'bf16': sa.EXACT_PAIRS[0],
               'f64': sa.EXACT_PAIRS[2]}
FORMULA = ((2654435761, 7), (2246822519, 9))    # (multiplier, shift)


def r_B(k):
    return -(-B // k)


# ---------------------------------------------------------------------------
# the SpMM entry points
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def spmm_cases(prec):
    """Every k of K[prec] x role x entry point x queue 0 and 1. Per (k, role)
    the plain cases come first, so that the second tall buffer of far-write
    exists only from the first affine case on."""
    mod = sa._mod(prec)
    cs = []
    for k in K[prec]:
        for role in ROLES:
            for entry, beta, pair in ENTRIES:
                for q in (0, 1):
                    sched = mod.default_queued(k) if q else sc.GRID
                    cs.append(sa.case(
                        f'far{role}_{entry}_k{k}_b{beta}_q{q}', MATRIX[role],
                        'exact', k, beta, q, pair, row_ids=(role == 'write'),
                        plan=mod.plan(k, sched), role=role, entry=entry))
    return tuple(cs)


def compact(prec, case, shared=None):
    """The compact case: operands, touched rows and reference of the existing
    modules (nothing is recomputed here by other means). shared: (X0, X1, C0,
    R, plain product), when the caller already holds them. D: norm cases
    only; far-write passes D = R."""
    if shared is None:
        X0, X1, C0, R = sa.operands(prec, case)
        P = None
    else:
        X0, X1, C0, R, P = shared
    rows, ref = sa.reference(prec, case, X0, X1, C0, R, product=P)
    D = None
    if case['entry'] == 'norm':
        D = R if case['role'] == 'write' else sn.operand_D(prec, case)
    return dict(X0=X0, X1=X1, C0=C0, R=R, D=D, rows=rows, ref=ref)


def _int32(a, what):
    a = np.asarray(a, dtype=np.int64)
    assert a.size == 0 or (int(np.abs(a).max()) < 2 ** 31 - 1), what
    return a


def placement(prec, case):
    """Where the tall side of the case lies. tall: {buffer: rows}; windows:
    {operand: (buffer, first row, rows)}; touched: {operand: the rows of its
    buffer the kernels address}; cols / row_ids: what the structure is
    created with (None: the compact case's own)."""
    m = sc.matrix(case['matrix'])
    k = case['k']
    if case['role'] == 'read':
        n0, n1 = m['n0'], max(m['n1'], 1)
        base0 = r_B(k) - n0 // 2
        base1 = base0 + n0 + GAP_ROWS
        c = m['cols'].astype(np.int64)
        idx1 = -c[c < 0] - 1
        cols = np.where(c >= 0, c + base0, -((-c - 1) + base1 + 1))
        assert base1 + n1 < 2 ** 31
        return dict(
            k=k, cols=_int32(cols, 'columns fit int32').astype(np.int32),
            row_ids=None, tall={'X': base1 + n1},
            windows={'X0': ('X', base0, n0), 'X1': ('X', base1, n1)},
            touched={'X0': np.unique(c[c >= 0]) + base0,
                     'X1': np.unique(idx1) + base1})
    W = sc.out_rows(case)
    out_base = r_B(k) - W // 2
    rid = out_base + sc.row_ids(case)
    assert out_base + W < 2 ** 31
    tall, windows, touched = {'C': out_base + W}, {'C': ('C', out_base, W)}, \
        {'C': rid}
    if case['has_R']:
        tall['R'] = out_base + W
        windows['R'] = ('R', out_base, W)
        touched['R'] = rid
        if case['entry'] == 'norm':      # D = R: the same buffer and rows
            windows['D'] = windows['R']
            touched['D'] = rid
    return dict(k=k, cols=None, row_ids=_int32(rid, 'row ids fit int32'),
                tall=tall, windows=windows, touched=touched)


# ---------------------------------------------------------------------------
# the route kernels
# ---------------------------------------------------------------------------

def route_cases(prec):
    return [(f'farroute_{op}_k{k}_{side}tall', op, k, side)
            for op in sc.ROUTE_OPS for k in ROUTE_K[prec]
            for side in ROUTE_SIDES]


def route_window_rows(op, side):
    """Rows of route_case's src / dst (without drawing them)."""
    small = op in ('scatter', 'scatter_add') if side == 'src' \
        else op == 'gather'
    return ROUTE_N if small else ROUTE_N + 13


def route_placement(prec, op, k, side):
    """`route_case`, unchanged, with its src or its dst as a window of a tall
    buffer. An index array of the tall side points into the window (idx +
    base); where the kernel walks that side contiguously (it has no index
    array), the pointer itself is the window's start (ptr_row = base)."""
    rc = sa._mod(prec).route_case(op, ROUTE_N, k)
    W = (rc['src'] if side == 'src' else rc['dst0']).shape[0]
    base = r_B(k) - W // 2
    idx = rc[side + '_idx']
    assert base + W < 2 ** 31
    return dict(
        k=k, rc=rc, side=side, base=base, tall={side: base + W},
        windows={side: (side, base, W)},
        idx=None if idx is None else idx + base,
        ptr_row=base if idx is None else 0,
        touched={side: base + (np.arange(W) if idx is None else idx)})


# ---------------------------------------------------------------------------
# the contiguous kernels
# ---------------------------------------------------------------------------

def contig_cases(prec):
    return [(f'far{kernel}_n{n}_k{k}', kernel, n, k)
            for kernel in CONTIG_KERNELS for n, k in CONTIG_SHAPES[prec]]


def formula(i, which=0):
    """Integers in [-8, 8] from the flat element index i (int64: a numpy
    array on the host, a torch tensor on the device); which = 0 for C, 1 for
    the second operand (R or D)."""
    mult, shift = FORMULA[which]
    return ((i * mult) >> shift) % 17 - 8


def contig_operands(prec, kernel):
    """Tall buffers of a contiguous case: C, and R / D except in float64."""
    return 1 if prec == 'f64' else 2


# ---------------------------------------------------------------------------
# offsets and memory, from the shapes
# ---------------------------------------------------------------------------

def element_offsets(k, rows):
    """Every element offset of the given rows of width k."""
    return (np.asarray(rows, dtype=np.int64)[:, None] * k
            + np.arange(k, dtype=np.int64)).reshape(-1)


def tall_bytes(prec, k, rows):
    return rows * k * ITEMSIZE[prec] + 2 * PAD * WORDSIZE[prec]


def peak_bytes(prec, k, tall):
    """The tall buffers alive during one case, guard pads included."""
    return sum(tall_bytes(prec, k, rows) for rows in tall.values())


def contig_peak_bytes(prec, kernel, n, k):
    return contig_operands(prec, kernel) * tall_bytes(prec, k, n)


@functools.lru_cache(maxsize=None)
def job_peaks(prec):
    """{job name: the peak figure the GPU test holds the child to (less its
    1 GiB allowance)}, for every job of the precision's child."""
    peaks = {}
    for c in spmm_cases(prec):
        peaks[c['name']] = peak_bytes(prec, c['k'], placement(prec, c)['tall'])
    for name, op, k, side in route_cases(prec):
        W = route_window_rows(op, side)
        peaks[name] = tall_bytes(prec, k, r_B(k) - W // 2 + W)
    for name, kernel, n, k in contig_cases(prec):
        peaks[name] = contig_peak_bytes(prec, kernel, n, k)
    peaks['rowid_misuse'] = 0
    return peaks


def job_names(prec):
    """Every JSON line the precision's child prints."""
    return list(job_peaks(prec))
