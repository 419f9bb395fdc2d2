"""Inputs, references and the environment -> launch-plan table shared by the
SpMM variant tests (test_plan_policy.py, test_spmm_cases.py on the CPU;
spmm_driver.py / test_gpu_variants.py on the GPU), and the builders of the
case tables of every precision (spmm_cases_f64.py, spmm_cases_bf16.py).

Everything is built here, in one place, from fixed seeds and raw CSR arrays.
This module imports numpy/scipy only: it never touches the GPU.

Exact inputs: A's values come from {+-0.5, +-1, +-2}; X and C0 hold integers
in [-8, 8]. Every product is a multiple of 0.5 of magnitude <= 16, so a row
of up to 8192 terms (plus C0) stays below 2**18 in units of 0.5 and every
partial sum, in every order, is exact in fp32 (24-bit significand): fma
accumulation, split-row atomics and beta=1 included. The kernel output must
therefore equal the float64 reference bit for bit.
"""
import functools

import numpy as np
from scipy import sparse

SEG_NNZ = 2048            # csrc: max nonzeros per work item
GRID_STRIDE_CAP = 8192    # csrc: grid-stride workgroup cap
Q_BLOCKS_DEFAULT = 2048   # csrc: ARROW_Q_BLOCKS default
GRID, QBLOCK, QWAVE = 0, 1, 2   # plan 'scheduler' values

K_ALL = (1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 20, 24, 32, 36, 64, 100, 128, 129,
         130, 256, 260, 512)
# k -> (vec, group) with no variables set, written out by hand
VEC_GROUP = {1: (1, 1), 2: (2, 1), 3: (1, 4), 4: (4, 1), 5: (1, 8), 6: (2, 4),
             7: (1, 8), 8: (4, 2), 12: (4, 4), 16: (4, 4), 20: (4, 8),
             24: (4, 8), 32: (4, 8), 36: (4, 16), 64: (4, 16), 100: (4, 32),
             128: (4, 32), 129: (1, 64), 130: (2, 64), 256: (4, 64),
             260: (4, 64), 512: (4, 64), 1024: (4, 64)}
GROUPS = (1, 2, 4, 8, 16, 32, 64)

N0, N1 = 2304, 512        # rows of X0 and of the dual operand X1
EXACT_VALS = np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], dtype=np.float32)


# ---------------------------------------------------------------------------
# matrices (raw CSR arrays; negative column c reads X1[-c-1])
# ---------------------------------------------------------------------------

def _mat(rows, lens, rng, dual=False, n0=N0, n1=N1):
    lens = np.asarray(lens, dtype=np.int64)
    assert lens.size == rows
    indptr = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    nnz = int(indptr[-1])
    # columns are drawn with replacement: rows longer than n0 need repeats,
    # and the kernels do not care (raw CSR, never canonicalised)
    cols = rng.integers(0, n0, nnz).astype(np.int32)
    if dual:
        neg = rng.random(nnz) < 0.3
        cols[neg] = -(rng.integers(0, n1, int(neg.sum())).astype(np.int32) + 1)
    vals = EXACT_VALS[rng.integers(0, EXACT_VALS.size, nnz)]
    return dict(rows=rows, n0=n0, n1=n1 if dual else 0, indptr=indptr,
                cols=cols, vals=vals, real_vals=None)


def n_items(mat):
    lens = np.diff(mat['indptr'])
    return int(np.maximum(1, -(-lens // SEG_NNZ)).sum())


def std_row_lengths():
    special = {7, 8, 9, 12, 2047, 2048, 2049, 4097}
    for g in GROUPS:
        special |= {0, 1, g - 1, g, g + 1, 2 * g + 3}
    return sorted(special)


def _std(dual):
    rng = np.random.default_rng(20240 + int(dual))
    special = std_row_lengths()
    rows = 330
    filler = rng.integers(0, 25, rows - 20 - len(special)).tolist()
    lens = np.array(special + filler)
    rng.shuffle(lens)
    at = 97   # one run of 20 consecutive empty rows
    lens = np.concatenate([lens[:at], np.zeros(20, dtype=lens.dtype), lens[at:]])
    m = _mat(rows, lens, rng, dual=dual)
    # ragged against every GROUPS_PER_BLOCK (4..256): leaves qseg ragged too
    assert n_items(m) % 4 in (1, 3), n_items(m)
    return m


def _from_scipy(A, seed):
    """An existing test's matrix: its pattern and fp32 values are kept as
    real_vals; `vals` is the exact-valued substitute on the same pattern."""
    A = sparse.csr_matrix(A, dtype=np.float32)
    rng = np.random.default_rng(seed)
    return dict(rows=A.shape[0], n0=A.shape[1], n1=0,
                indptr=A.indptr.astype(np.int64),
                cols=A.indices.astype(np.int32),
                vals=EXACT_VALS[rng.integers(0, EXACT_VALS.size, A.nnz)],
                real_vals=A.data.astype(np.float32))


def _random_csr(rows, cols, density, seed):   # as tests/test_gpu_kernels.py
    rs = np.random.RandomState(seed)
    m = sparse.random(rows, cols, density=density, format='csr',
                      random_state=rs, dtype=np.float64)
    return sparse.csr_matrix(m, dtype=np.float32)


def _legacy_wave_hub():   # test_spmm_queue_wave_grabs_hub's matrix
    rows, cols = 400, 5000
    rs = np.random.RandomState(13)
    A = sparse.random(rows, cols, density=0.002, format='lil', random_state=rs,
                      dtype=np.float64)
    A[3, :] = rs.rand(cols)
    A[111, :] = 0
    return sparse.csr_matrix(A, dtype=np.float32)


def _real():
    """Real-valued guard: rows of <= 64 entries, magnitudes uniform in
    [0.25, 1] with random sign (no product can underflow)."""
    rng = np.random.default_rng(515)
    rows = 203
    lens = np.concatenate([np.arange(65), rng.integers(0, 65, rows - 65)])
    rng.shuffle(lens)
    m = _mat(rows, lens, rng, n0=300)
    m['vals'] = real_values(rng, m['vals'].size)
    return m


def real_values(rng, shape):
    mag = rng.uniform(0.25, 1.0, shape)
    return (mag * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def _stride():
    # 40 000 items at GROUP 64 (4 groups per block) need 10 000 blocks: past
    # the 8192-block cap, so the grid-stride loop body iterates
    rng = np.random.default_rng(40000)
    return _mat(40000, rng.integers(1, 4, 40000), rng)


def _remap(items):
    rng = np.random.default_rng(items)
    return _mat(items, rng.integers(0, 13, items), rng)


def _zero_rows():
    # 1025 split rows x k=1024 = 1 049 600 elements > 4096 x 256 threads
    rng = np.random.default_rng(1025)
    return _mat(1025, np.full(1025, 2049), rng)


# remap cases at k=128 (GROUP 32, 8 groups per block): gridDim.x = 33, 37, 39
REMAP_ITEMS = {1: 8 * 32 + 3, 5: 8 * 36 + 5, 7: 8 * 38 + 1}


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name == 'std':
        return _std(False)
    if name == 'std_dual':
        return _std(True)
    if name == 'real':
        return _real()
    if name == 'stride':
        return _stride()
    if name == 'zero_rows':
        return _zero_rows()
    if name.startswith('remap'):
        return _remap(REMAP_ITEMS[int(name[5:])])
    if name.startswith('legacy_wave_k'):     # test_spmm_queue_wave_grabs[k]
        k = int(name[len('legacy_wave_k'):])
        return _from_scipy(_random_csr(600, 800, 0.02, seed=300 + k), 300 + k)
    if name == 'legacy_wave_hub':
        return _from_scipy(_legacy_wave_hub(), 13)
    if name == 'legacy_k16g8':               # test_spmm_k16_g8_layout
        return _from_scipy(_random_csr(500, 700, 0.03, seed=77), 77)
    raise KeyError(name)


# ---------------------------------------------------------------------------
# operands and references
# ---------------------------------------------------------------------------

def _seed(case):
    return [case['k'], case['beta'], sum(map(ord, case['matrix']))]


def out_rows(case):
    m = matrix(case['matrix'])
    return m['rows'] + 37 if case.get('row_ids') else m['rows']


def row_ids(case):
    """Duplicate-free scatter of the structure rows into a larger C."""
    if not case.get('row_ids'):
        return None
    rng = np.random.default_rng(77)
    return rng.permutation(out_rows(case))[:matrix(case['matrix'])['rows']] \
        .astype(np.int64)


def operands(case):
    """(X0, X1, C0) fp32; C0 has the output's shape (used at beta=1)."""
    m = matrix(case['matrix'])
    k = case['k']
    rng = np.random.default_rng(_seed(case))
    shapes = [(m['n0'], k), (max(m['n1'], 1), k), (out_rows(case), k)]
    if case['kind'] == 'real':
        return tuple(real_values(rng, s) for s in shapes)
    if case['kind'] == 'legacy':     # the original test's draws, in its order
        rng = np.random.default_rng(case['legacy']['seed'])
        X = (2 * rng.random(shapes[0]) - 1).astype(np.float32)
        C0 = (2 * rng.random(shapes[2]) - 1).astype(np.float32)
        return X, X[:1], C0
    return tuple(rng.integers(-8, 9, s).astype(np.float32) for s in shapes)


def _csr(m, vals, dtype):
    c = m['cols'].astype(np.int64)
    c = np.where(c < 0, m['n0'] - c - 1, c)      # X1 stacked below X0
    return sparse.csr_matrix((vals.astype(dtype), c, m['indptr']),
                             shape=(m['rows'], m['n0'] + max(m['n1'], 1)))


def product(case, X0, X1, dtype, absolute=False):
    """A @ [X0; X1] over the structure rows, accumulated in `dtype`."""
    m = matrix(case['matrix'])
    X = np.vstack([X0, X1]).astype(dtype)
    vals = m['real_vals'] if case['kind'] == 'legacy' else m['vals']
    if absolute:
        vals, X = np.abs(vals), np.abs(X)
    return np.asarray(_csr(m, vals, dtype) @ X)


def reference(case, X0, X1, C0, dtype=np.float64):
    """(touched_rows, ref): ref covers the structure rows in output order."""
    ref = product(case, X0, X1, dtype)
    rid = row_ids(case)
    rows = rid if rid is not None else np.arange(ref.shape[0])
    if case['beta']:
        ref = ref + C0[rows].astype(dtype)
    return rows, ref


def real_bound(case, X0, X1, C0):
    """Per-element bound for fp32 accumulation of a row of len_i terms plus
    C0 in ANY order, with or without fma: the standard recursive-summation
    bound gamma_n = n*u/(1 - n*u) with n = 2*len_i + 2 (one rounding per
    product and per add, doubled so that it holds either way), u = 2**-24,
    applied to sum|a||x| + |C0|. Derived, not measured."""
    m = matrix(case['matrix'])
    g = (2.0 * np.diff(m['indptr']) + 2.0) * 2.0 ** -24
    mag = product(case, X0, X1, np.float64, absolute=True)
    if case['beta']:
        rid = row_ids(case)
        rows = rid if rid is not None else np.arange(mag.shape[0])
        mag = mag + np.abs(C0[rows]).astype(np.float64)
    return (g / (1.0 - g))[:, None] * mag


# ---------------------------------------------------------------------------
# the environment -> plan table
# ---------------------------------------------------------------------------

def vec_group_launches(k):
    """The float32 lookup k -> (vec, group, launches); float64 and bfloat16
    features have tables of their own and pass theirs as `lookup`."""
    vec, group = VEC_GROUP[k]
    return vec, group, -(-k // (vec * group))


def plan(k, sched, vec=None, group=None, nt=1, q_mult=4, qw_mult=2,
         q_blocks=Q_BLOCKS_DEFAULT, lookup=vec_group_launches):
    """Expected arrow_spmm_plan fields for one launch. vec / group: what a
    layout variable (ARROW_K16_G8, ARROW_SPMM_G64) puts in the table's
    place."""
    dv, dg, launches = lookup(k)
    if vec or group:
        vec, group = vec or dv, group or dg
        launches = -(-k // (vec * group))
    else:
        vec, group = dv, dg
    chunk = {GRID: 0, QBLOCK: (256 // group) * q_mult,
             QWAVE: (64 // group) * qw_mult}[sched]
    return dict(vec=vec, group=group, scheduler=sched, nt_mode=nt,
                chunk_items=chunk,
                grid_cap=GRID_STRIDE_CAP if sched == GRID else q_blocks,
                launches=launches)


def default_queued(k, lookup=vec_group_launches):
    """set_queue(1), no variables: wave grabs at GROUP < 8, else block grabs."""
    return QWAVE if lookup(k)[1] < 8 else QBLOCK


def policy(k, nnz, q_min_nnz=32 << 20, lookup=vec_group_launches):
    """Handle mode -1, ARROW_QUEUE unset: queues need GROUP >= 4 and
    nnz >= ARROW_Q_MIN_NNZ."""
    if lookup(k)[1] >= 4 and nnz >= q_min_nnz:
        return default_queued(k, lookup)
    return GRID


def case(name, k, beta, queue, expect, matrix='std', kind='exact', **opts):
    """queue: None leaves the handle at mode -1; 0 / 1 call set_queue."""
    c = dict(name=name, matrix=matrix, kind=kind, k=k, beta=beta, queue=queue,
             plan=expect)
    c.update(opts)
    return c


VARIANTS = ('dual', 'rowids', 'col1', 'col2', 'qb8')


def _variants(tag, k, sched_of, plan=plan, variants=VARIANTS, **pl):
    """The std-case variants at one k: dual operand, row_ids scatter,
    col_items 1 and 2, set_qblocks(8); grid-stride and queued. `plan` is the
    precision's; `variants` names the ones it has."""
    out = []
    for q in (0, 1):
        e = plan(k, sched_of(k) if q else GRID, **pl)
        sfx = f'k{k}_q{q}'
        for beta in (0, 1):
            out.append(('dual', case(f'{tag}_dual_{sfx}_b{beta}', k, beta, q,
                                     e, matrix='std_dual')))
            out.append(('rowids', case(f'{tag}_rowids_{sfx}_b{beta}', k, beta,
                                       q, e, row_ids=True)))
        out.append(('col1', case(f'{tag}_col1_{sfx}', k, 0, q, e,
                                 col_items=1)))
        out.append(('col2', case(f'{tag}_col2_{sfx}', k, 1, q, e, col_items=2,
                                 matrix='std_dual')))
    out.append(('qb8', case(f'{tag}_qb8_k{k}', k, 0, 1,
                            plan(k, sched_of(k), **pl), qblocks=8)))
    return [c for variant, c in out if variant in variants]


def _sweep(tag, ks, queue, sched_of, plan=plan, **pl):
    return [case(f'{tag}_k{k}_b{beta}', k, beta, queue,
                 plan(k, sched_of(k), **pl))
            for k in ks for beta in (0, 1)]


def _real_case(tag, k, queue, expect, beta=1):
    return case(f'{tag}_real_k{k}', k, beta, queue, expect, matrix='real',
                kind='real')


def _legacy(name, matrix, k, seeds, tol, expect):
    """An existing test's matrix, k, betas and operand seeds behind the
    driver: its own allclose check against scipy's fp32 product is kept
    (kind 'legacy', same rtol/atol), the derived float64 bound is checked as
    well, and the exact check is added on the same sparsity pattern."""
    out = []
    for beta, seed in enumerate(seeds):
        out.append(case(f'{name}_b{beta}', k, beta, 1, expect, matrix=matrix,
                        kind='legacy', legacy=dict(seed=seed, tol=tol)))
        out.append(case(f'{name}_exact_b{beta}', k, beta, 1, expect,
                        matrix=matrix))
    return out


def _env_default():
    grid = lambda k: GRID
    cs = _sweep('grid', K_ALL, 0, grid)
    cs += _sweep('queued', K_ALL, 1, default_queued)
    cs += _sweep('mode-1', (16, 128), None, grid)   # nnz below ARROW_Q_MIN_NNZ
    for k in (3, 16, 128, 260):
        cs += _variants('default', k, default_queued)
    cs.append(_real_case('grid', 36, 0, plan(36, GRID)))
    cs.append(_real_case('queued', 16, 1, plan(16, QWAVE)))
    cs.append(_real_case('queued', 128, 1, plan(128, QBLOCK)))
    # the loops that never looped
    for beta in (0, 1):
        cs.append(case(f'grid_stride_beyond_cap_b{beta}', 260, beta, 0,
                       plan(260, GRID), matrix='stride', remap='both',
                       capped_groups_per_block=4))
    for r in sorted(REMAP_ITEMS):
        cs.append(case(f'xcd_remap_grid_mod8_{r}', 128, (r // 2) % 2, 0,
                       plan(128, GRID), matrix=f'remap{r}', remap='both',
                       grid_mod8=r))
    cs.append(case('zero_rows_beyond_cap', 1024, 0, 0, plan(1024, GRID),
                   matrix='zero_rows', zero_rows_capped=True))
    return cs


def _env_qwave1():
    wave = lambda k: QWAVE
    ks = (32, 128, 260, 5, 36, 100, 129, 130)       # GROUP 8, 16, 32, 64
    cs = _sweep('qwave1', ks, 1, wave)
    for k in (32, 128, 260):
        cs += _variants('qwave1', k, wave)
    cs.append(_real_case('qwave1', 128, 1, plan(128, QWAVE)))
    for k in (32, 128):
        cs += _legacy(f'spmm_queue_wave_grabs_k{k}', f'legacy_wave_k{k}', k,
                      (40 + k, 41 + k), 1e-5, plan(k, QWAVE))
    cs += _legacy('spmm_queue_wave_grabs_hub', 'legacy_wave_hub', 16, (13,),
                  2e-5, plan(16, QWAVE))
    return cs


def _env_qwave0():
    block = lambda k: QBLOCK
    cs = _sweep('qwave0', (1, 3, 4, 8, 16, 2, 6, 12), 1, block)  # GROUP 1,2,4
    for k in (3, 8, 16):
        cs += _variants('qwave0', k, block)
    cs.append(_real_case('qwave0', 16, 1, plan(16, QBLOCK)))
    return cs


def _env_k16g8():
    pl = dict(vec=2, group=8)
    cs = []
    for beta in (0, 1):
        cs.append(case(f'k16g8_grid_b{beta}', 16, beta, 0, plan(16, GRID, **pl)))
        cs.append(case(f'k16g8_queued_b{beta}', 16, beta, 1,
                       plan(16, QBLOCK, **pl)))
    cs += _variants('k16g8', 16, lambda k: QBLOCK, **pl)
    for k in (12, 20):                               # unaffected
        cs += _sweep('k16g8_other_grid', (k,), 0, lambda k: GRID)
        cs += _sweep('k16g8_other_queued', (k,), 1, default_queued)
    cs.append(_real_case('k16g8', 16, 1, plan(16, QBLOCK, **pl)))
    cs += _legacy('spmm_k16_g8_layout', 'legacy_k16g8', 16, (77, 78),
                  1e-5, plan(16, QBLOCK, **pl))
    return cs


def _env_g64():
    pl = dict(vec=2, group=64)
    cs = []
    for beta in (0, 1):
        cs.append(case(f'g64_grid_b{beta}', 128, beta, 0, plan(128, GRID, **pl)))
        cs.append(case(f'g64_queued_b{beta}', 128, beta, 1,
                       plan(128, QBLOCK, **pl)))
    cs += _variants('g64', 128, lambda k: QBLOCK, **pl)
    cs += _sweep('g64_other_grid', (64,), 0, lambda k: GRID)   # unaffected
    cs += _sweep('g64_other_queued', (64,), 1, default_queued)
    cs.append(_real_case('g64', 128, 1, plan(128, QBLOCK, **pl)))
    return cs


def _env_nt0():
    ks = (16, 128, 130)
    cs = _sweep('nt0_grid', ks, 0, lambda k: GRID, nt=0)
    cs += _sweep('nt0_queued', ks, 1, default_queued, nt=0)
    for k in (16, 128):
        cs += _variants('nt0', k, default_queued, nt=0)
    cs.append(_real_case('nt0', 128, 0, plan(128, GRID, nt=0)))
    return cs


_Q_KS = (1, 3, 4, 8, 16, 32, 100, 128, 130, 260)


def _env_chunk(tag, **pl):
    cs = _sweep(tag, _Q_KS, 1, default_queued, **pl)
    for k in (16, 128):
        cs += _variants(tag, k, default_queued, **pl)
    cs.append(_real_case(tag, 16, 1, plan(16, QWAVE, **pl)))
    cs.append(_real_case(tag, 128, 1, plan(128, QBLOCK, **pl)))
    return cs


def _policy(k):
    """Handle mode -1, ARROW_QUEUE unset, nnz >= ARROW_Q_MIN_NNZ."""
    return policy(k, nnz=0, q_min_nnz=0)


def _env_min_nnz0():
    ks = (1, 2, 8, 3, 16, 32, 128, 130)     # GROUP 1, 1, 2 | 4, 4, 8, 32, 64
    cs = _sweep('policy', ks, None, _policy)
    cs.append(case('policy_dual_k128', 128, 0, None, plan(128, QBLOCK),
                   matrix='std_dual'))
    cs.append(_real_case('policy', 16, None, plan(16, QWAVE)))
    return cs


def _env_queue(tag, env_on):
    ks = (4, 16, 128)
    env_sched = default_queued if env_on else (lambda k: GRID)
    cs = _sweep(f'{tag}_mode-1', ks, None, env_sched)
    cs += _sweep(f'{tag}_set0', ks, 0, lambda k: GRID)
    cs += _sweep(f'{tag}_set1', ks, 1, default_queued)
    cs.append(_real_case(tag, 128, None, plan(128, env_sched(128))))
    return cs


@functools.lru_cache(maxsize=None)
def env_table():
    """name -> (variables, cases). One fresh child process per entry: the
    ARROW_* kernel variables are read once per process."""
    return {
        'default': ({}, _env_default()),
        'qwave1': ({'ARROW_QWAVE': '1'}, _env_qwave1()),
        'qwave0': ({'ARROW_QWAVE': '0'}, _env_qwave0()),
        'k16g8': ({'ARROW_K16_G8': '1'}, _env_k16g8()),
        'g64': ({'ARROW_SPMM_G64': '1'}, _env_g64()),
        'nt0': ({'ARROW_SPMM_NT': '0'}, _env_nt0()),
        'chunk1': ({'ARROW_Q_CHUNK': '1', 'ARROW_QW_CHUNK': '1',
                    'ARROW_Q_BLOCKS': '8'},
                   _env_chunk('chunk1', q_mult=1, qw_mult=1, q_blocks=8)),
        'chunk64': ({'ARROW_Q_CHUNK': '64', 'ARROW_QW_CHUNK': '64'},
                    _env_chunk('chunk64', q_mult=64, qw_mult=64)),
        'min_nnz0': ({'ARROW_Q_MIN_NNZ': '0'}, _env_min_nnz0()),
        'queue1': ({'ARROW_QUEUE': '1'}, _env_queue('queue1', True)),
        # ARROW_Q_MIN_NNZ=0 as well: were ARROW_QUEUE=0 ignored, the policy
        # default would queue these and the asserted plan would be wrong
        'queue0': ({'ARROW_QUEUE': '0', 'ARROW_Q_MIN_NNZ': '0'},
                   _env_queue('queue0', False)),
    }


KERNEL_VARS = ('ARROW_SPMM_G64', 'ARROW_K16_G8', 'ARROW_SPMM_NT',
               'ARROW_QUEUE', 'ARROW_QWAVE', 'ARROW_Q_MIN_NNZ',
               'ARROW_Q_CHUNK', 'ARROW_Q_BLOCKS', 'ARROW_QW_CHUNK')


def child_env(base, variables):
    """`base` without any kernel variable, plus this entry's."""
    env = {k: v for k, v in base.items() if k not in KERNEL_VARS}
    env.update(variables)
    return env


# ---------------------------------------------------------------------------
# route / permute kernels
# ---------------------------------------------------------------------------

ROUTE_OPS = ('gather', 'scatter', 'scatter_add', 'permute', 'permute_add')
# (n, k); the last has n * k_vec = 4 257 000 > 16384 x 256 threads
ROUTE_SHAPES = [(n, k) for n in (0, 1, 500) for k in (1, 3, 4, 33, 128)] \
    + [(33000, 129)]


def route_case(op, n, k, draw=None, seed_prefix=(), add=np.add):
    """Operands and the numpy fancy-indexing reference, bit for bit (a
    single fp32 add per element is the same on both sides). Indices are
    duplicate-free partial permutations into larger arrays. The other
    precisions pass how they draw an operand (default: real_values), the
    prefix of their RNG seed and how `+=` is computed."""
    draw = draw or real_values
    rng = np.random.default_rng([*seed_prefix, ROUTE_OPS.index(op), n, k])
    big = n + 13
    src_rows = n if op in ('scatter', 'scatter_add') else big
    dst_rows = n if op == 'gather' else big
    src = draw(rng, (src_rows, k))
    dst0 = draw(rng, (dst_rows, k))
    src_idx = rng.permutation(src_rows)[:n].astype(np.int64)
    dst_idx = rng.permutation(dst_rows)[:n].astype(np.int64)
    ref = dst0.copy()
    if op == 'gather':
        ref[:] = src[src_idx]
        dst_idx = None
    elif op == 'scatter':
        ref[dst_idx] = src
        src_idx = None
    elif op == 'scatter_add':
        ref[dst_idx] = add(ref[dst_idx], src)
        src_idx = None
    elif op == 'permute':
        ref[dst_idx] = src[src_idx]
    else:
        ref[dst_idx] = add(ref[dst_idx], src[src_idx])
    return dict(src=src, dst0=dst0, src_idx=src_idx, dst_idx=dst_idx, ref=ref)
