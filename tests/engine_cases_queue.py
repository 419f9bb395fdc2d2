"""Layouts, feature widths, queue environments, the exact-valued class and the
job names of the queued engine tests (test_engine_cases_queue.py on the CPU;
engine_queue_driver.py / test_gpu_queue_engine.py on the GPU).

The engines never call set_queue: a resident structure gets a per-XCD queue
scheduler only through the launch policy (handle mode -1, GROUP >= 4, nnz >=
ARROW_Q_MIN_NNZ), and the structures of the engine tests hold a few thousand
nonzeros. QUEUE_ENVS lowers the threshold to 0, so that every structure of
every layout of LAYOUTS is launched by the queue kernels, at the widths of
K_OF. Shapes, layout variables and the real-valued class come from the
engine drivers unchanged; this module adds only what is below. It imports
numpy/scipy (and the drivers' host-side helpers) only: it never touches the
GPU.

Exact class. exact_decomposition(layout) is the layout's synth decomposition
with every part's values redrawn from spmm_cases.EXACT_VALS {+-0.5, +-1, +-2};
features and residual hold integers in [-8, 8]; (alpha, gamma) = (0.5, 2.0).
Every product is a multiple of 0.5 of magnitude <= 16. A row of the
recomposed matrix receives at most MAX_ROW_TERMS = 8192 stored values over all
parts (asserted below, for every layout), so whatever is summed into one
output element, in any grouping and order (one launch or one per part, split-
row atomics, fma or not), is a multiple of 0.5 below 2**17; alpha = 0.5 makes
it a multiple of 0.25 below 2**16, applied per partial or once; gamma * R is a
multiple of 2 of magnitude <= 16. Everything stays below 2**20 quarter-units:
exact in float32 (24 bits) and in float64. One step therefore equals the
float64 evaluation on the recomposed matrix bit for bit, and for bfloat16
features, where exactly one rounding happens per element (the single-launch
layouts), its one cast to bf16.
"""
import functools

import numpy as np

from tests import engine_affine_driver as ead
from tests import engine_scale_driver as esd
from tests import spmm_cases as sc
from tests import spmm_cases_affine as sa
from tests import spmm_cases_bf16 as s16
from tests import spmm_cases_f64 as s64

GRID, QBLOCK, QWAVE = sc.GRID, sc.QBLOCK, sc.QWAVE
SCHED_NAME = {GRID: 'GRID', QBLOCK: 'QBLOCK', QWAVE: 'QWAVE'}

# name -> (variables, the multipliers spmm_cases.plan takes for them)
_CHUNK1 = sc.env_table()['chunk1'][0]
QUEUE_ENVS = {
    # the product's own switch, with the threshold lowered
    'policy': {'ARROW_Q_MIN_NNZ': '0'},
    # a few hundred items drained by 8 workgroups, one round per grab: the
    # grab loop loops, queues run dry and steal
    'chunk1': {'ARROW_Q_MIN_NNZ': '0', **_CHUNK1},
}
PLAN_OPTS = {'policy': {},
             'chunk1': dict(q_mult=1, qw_mult=1, q_blocks=8)}
assert _CHUNK1 == {'ARROW_Q_CHUNK': '1', 'ARROW_QW_CHUNK': '1',
                   'ARROW_Q_BLOCKS': '8'}

PRECISIONS = ead.PRECISIONS
# precision -> ((k, vec, group, scheduler), ...): one width whose policy plan
# is wave grabs (GROUP 4) and one whose plan is block grabs. Written out by
# hand; test_engine_cases_queue.py asks the library.
K_OF = {
    'float32': ((16, 4, 4, QWAVE), (128, 4, 32, QBLOCK)),
    'float64': ((8, 2, 4, QWAVE), (64, 2, 32, QBLOCK)),
    'bfloat16': ((32, 8, 4, QWAVE), (128, 8, 16, QBLOCK)),
}
_PLAN = {'float32': sc.plan, 'float64': s64.plan, 'bfloat16': s16.plan}
_LOOKUP = {'float32': sc.vec_group_launches,
           'float64': s64.vec_group_launches,
           'bfloat16': s16.vec_group_launches}
for _p, _rows in K_OF.items():
    for _k, _vec, _group, _sched in _rows:
        assert _LOOKUP[_p](_k)[:2] == (_vec, _group), (_p, _k)
        assert _sched == (QWAVE if _group < 8 else QBLOCK) and _group >= 4


def expected_plan(queue_env, precision, k):
    """arrow_spmm_plan's fields for a structure of any nnz at handle mode -1
    in a process started with QUEUE_ENVS[queue_env]."""
    sched = {row[0]: row[3] for row in K_OF[precision]}[k]
    return _PLAN[precision](k, sched, **PLAN_OPTS[queue_env])


# ---------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------

_FUSE0 = {'ARROW_FUSE_ALL': '0'}
# name -> (layout variables, build arguments; k is replaced per K_OF)
LAYOUTS = {
    'default': ({}, ead.L1),
    'hub': ({}, ead.HUB),                       # split rows
    **{name: ead.MODES[name][:2]
       for name in ('fuse_all0', 'fold0', 'fold1', 'fold2', 'banded')},
    'split_col': ({**_FUSE0, 'ARROW_SPLIT_COL': '1'},
                  dict(ead.L1, hub_rows=2)),
    'row0_chunks': ({**_FUSE0, 'ARROW_ROW0_CHUNKS': '4'}, ead.L1),
    'rest_chunks': ({**_FUSE0, 'ARROW_REST_CHUNK_NNZ': '500'}, ead.L1),
}
CHUNK1_LAYOUTS = ('default', 'hub', 'fuse_all0', 'fold1')
# the launches of these carry the affine step (no tail kernel) / measure the
# step norms themselves (no stand-alone pass): engine_affine_driver.MODES and
# engine_norm_driver.MODES say the same of the layouts they hold
AFFINE_INSIDE = ('default', 'hub', 'fold1', 'fold2')
NORM_FUSED = ('default', 'hub')
# bfloat16 features are rounded exactly once per element here
BF16_ROUNDS_ONCE = ('default', 'hub')


def children():
    """The (queue_env, layout) pairs, one child process each."""
    return [('policy', layout) for layout in LAYOUTS] \
        + [('chunk1', layout) for layout in CHUNK1_LAYOUTS]


def child_variables(queue_env, layout):
    return {**QUEUE_ENVS[queue_env], **LAYOUTS[layout][0]}


def build_args(layout, k):
    return dict(LAYOUTS[layout][1], k=k)


TIERS = ('plain', 'affine', 'affine_norm')


def job_name(precision, k, tier):
    return f'{precision}_k{k}_{tier}'


def jobs(queue_env, layout):
    """[(name, precision, k, tier)] of one child: the driver runs them and
    the GPU test expects their names. The same for every child."""
    assert (queue_env, layout) in children()
    return [(job_name(p, row[0], tier), p, row[0], tier)
            for p in PRECISIONS for row in K_OF[p] for tier in TIERS]


# (precision, layout, k) of the capture child's jobs
CAPTURE_JOBS = (('float32', 'default', 128), ('float32', 'default', 16),
                ('bfloat16', 'hub', 128))


def capture_job_name(precision, layout, k):
    return f'{precision}_{layout}_k{k}'


# ---------------------------------------------------------------------------
# the exact class
# ---------------------------------------------------------------------------

MAX_ROW_TERMS = 8192                     # spmm_cases_affine's budget
EXACT_ALPHA, EXACT_GAMMA = sa.EXACT_PAIRS[0][:2]
assert (EXACT_ALPHA, EXACT_GAMMA) == (0.5, 2.0)
X_MAX = 8
_SEED = 20260


def pair(tier):
    """(alpha, gamma) of the exact step of a tier."""
    return (1.0, 0.0) if tier == 'plain' else (EXACT_ALPHA, EXACT_GAMMA)


@functools.lru_cache(maxsize=None)
def exact_decomposition(layout):
    """The layout's synth decomposition, pattern and permutations unchanged,
    every part's data redrawn from EXACT_VALS by a fixed seed."""
    shape = LAYOUTS[layout][1]
    rng = np.random.default_rng([_SEED, shape['seed']])
    out = []
    for B, perm in esd.make_decomp(**shape):
        B = B.copy()
        B.data = sc.EXACT_VALS[rng.integers(0, sc.EXACT_VALS.size, B.nnz)]
        out.append((B, perm))
    return out


def _recompose(decomp, transform):
    from arrow_matrix_amd import synth
    return synth.recompose([(transform(B.astype(np.float64)), p)
                            for B, p in decomp]).tocsr()


def _ones(B):
    B = B.copy()
    B.data[:] = 1.0
    return B


@functools.lru_cache(maxsize=None)
def exact_matrix(layout):
    """The recomposed exact-valued matrix, float64, original row order."""
    return _recompose(exact_decomposition(layout), lambda B: B)


def row_terms(decomp):
    """Per row of the recomposed matrix, the stored values of all parts that
    fall into it: what an engine adds into one output row."""
    return np.asarray(_recompose(decomp, _ones).sum(axis=1)).ravel()


def exact_budget(layout):
    """(longest row in stored values, the largest magnitude any partial sum
    of one output element can reach, in quarter-units)."""
    longest = int(row_terms(exact_decomposition(layout)).max())
    vmax = float(np.abs(sc.EXACT_VALS).max())
    quarter_units = (longest * vmax * X_MAX          # alpha applied late
                     + abs(EXACT_GAMMA) * X_MAX) / 0.25
    return longest, quarter_units


for _layout in LAYOUTS:
    _longest, _units = exact_budget(_layout)
    assert _longest <= MAX_ROW_TERMS, (_layout, _longest)
    assert _units < 2 ** 24, (_layout, _units)
# alpha and gamma keep every term on the quarter-unit grid
assert all(float(EXACT_ALPHA * v * x / 0.25).is_integer()
           for v in sc.EXACT_VALS for x in range(-X_MAX, X_MAX + 1))
assert float(EXACT_GAMMA).is_integer()
# the hub layout has rows that one work item cannot hold
assert np.diff(exact_decomposition('hub')[0][0].indptr).max() > sc.SEG_NNZ


def n_rows(layout):
    shape = LAYOUTS[layout][1]
    return shape['n_blocks'][0] * shape['width']


def exact_operands(layout, k):
    """(X, R, perm0): float64 integers in [-8, 8], original row order, and
    part 0's permutation (the engine takes X[perm0], R[perm0])."""
    rng = np.random.default_rng([_SEED, LAYOUTS[layout][1]['seed'], k])
    shape = (n_rows(layout), k)
    X = rng.integers(-X_MAX, X_MAX + 1, shape).astype(np.float64)
    R = rng.integers(-X_MAX, X_MAX + 1, shape).astype(np.float64)
    return X, R, exact_decomposition(layout)[0][1]


def exact_reference(layout, k, tier):
    """alpha * A @ X + gamma * R in float64 on the recomposed matrix, in
    part 0's order: what the engine's result tile holds after one step."""
    X, R, perm0 = exact_operands(layout, k)
    alpha, gamma = pair(tier)
    G = alpha * np.asarray(exact_matrix(layout) @ X) + gamma * R
    return G[perm0]


# ---------------------------------------------------------------------------
# the real class: the plain step's bound
# ---------------------------------------------------------------------------

def plain_step_bound(A, absA, X, L, precision):
    """engine_affine_driver.step_bound at alpha 1, gamma 0, R 0 (its
    constants are the affine pair's): (golden, bound) of X <- A @ X."""
    n_row = np.diff(A.indptr).astype(np.float64)
    u = 2.0 ** -53 if precision == 'float64' else 2.0 ** -24
    s = L + 1 if precision == 'bfloat16' else 0
    factor = s * 2.0 ** -8 + (2.0 * n_row + 2.0 * L + 8.0) * u
    return np.asarray(A @ X), factor[:, None] * np.asarray(absA @ np.abs(X))
