"""Cases, names, references and the bound of the multi-rank engine tests
(test_engine_cases_ranks.py on the CPU; engine_ranks_driver.py /
test_gpu_rank_engine.py on the GPU, where the ranks of a world share one
device under the gloo backend).

Everything the engines do only at comm.size > 1 is reached from here: the
chunked C_0 reduce of ArrowSlimMPI._spmm_gpu and its branch for a rank that
owns no block, the deferred C_0 allreduce of the iterated loop
(allreduce_x0), the X_0 broadcast overlapped with the row-0 launch, the
overlapped forward exchange and the aggregate of ArrowDecompositionMPI at
L > 1, and the staged halo exchange of the banded engine. Shapes are the
small ones the suite already uses (test_distributed_gloo._worker,
engine_affine_driver.L1 / L2 / BANDED); widths are engine_cases_queue.K_OF's.
This module imports numpy/scipy and the drivers' host-side helpers only: it
never touches the GPU.

A case is Case(world, shape, precision, k, options, variables): `shape` names
an entry of SHAPES, `options` is the engines' allreduce_x0 setting (OPTIONS),
`variables` what the child process starts with. A child (CHILDREN) is one
world and one set of variables; its jobs are its cases, run in order by every
rank.

Exact class. exact_decomposition(shape) is the shape's synth decomposition
with every part's values redrawn from spmm_cases.EXACT_VALS {+-0.5, +-1,
+-2}; features hold integers in [-8, 8]. Every product is a multiple of 0.5
of magnitude <= 16, and a row of the recomposed matrix receives at most
MAX_ROW_TERMS stored values over all parts (asserted below, for every shape),
so whatever is summed into one output element stays a multiple of 0.5 below
2**17: exact in float32 and float64 in any grouping and order, over any
number of ranks, chunks and parts. One plain step from freshly set features
therefore equals the float64 evaluation on the recomposed matrix bit for
bit. Every exact step sets new integer features first, so magnitudes never
compound.

Real class. Four steps with X := C on the engine's own result; the golden of
a step is the float64 evaluation on the engine's own previous output, read
back exactly, to step_bound below.
"""
import functools
from typing import NamedTuple

import numpy as np

from tests import engine_affine_driver as ead
from tests import engine_cases_queue as ecq
from tests import engine_scale_driver as esd
from tests import spmm_cases as sc

PRECISIONS = ('float32', 'float64')
# per precision one width planned for wave grabs and one for block grabs
K_OF = {p: tuple(row[0] for row in ecq.K_OF[p]) for p in PRECISIONS}
assert K_OF == {'float32': (16, 128), 'float64': (8, 64)}


# ---------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------

def _gloo(n_blocks, width, seed, banded=False):
    """A tuple of test_distributed_gloo._worker (its k is replaced)."""
    shape = dict(n_blocks=n_blocks, width=width, seed=seed)
    if banded:
        shape.update(block_diagonal=False, slim=False)
    return shape


def _no_k(shape):
    return {key: value for key, value in shape.items() if key != 'k'}


SHAPES = {
    # slim, L = 1. width 64: the C_0 reduce runs in four chunks
    'w64x4': dict(_no_k(ead.L1), n_blocks=[4]),   # two blocks a rank at W = 2
    'w64x3': _no_k(ead.L1),                       # uneven spans at W = 2
    'w64x2': _gloo([2], 64, 9),     # W = 3: one rank owns nothing
    'w6x4': _gloo([4], 6, 0),       # below 64: one reduce, odd tile
    # L > 1: overlapped forward exchange, aggregate
    'l2_3_2': _gloo([3, 2], 4, 2),
    'l2_4_2': _no_k(ead.L2),
    'l3_4_3_2': _gloo([4, 3, 2], 4, 3),
    # banded: halo tiles
    'band4': _no_k(ead.BANDED),
    'band5': _gloo([5], 4, 8, banded=True),       # uneven spans
}
SLIM_L1 = ('w64x4', 'w64x3', 'w64x2', 'w6x4')
PARTS = ('l2_3_2', 'l2_4_2', 'l3_4_3_2', 'band4', 'band5')
assert set(SLIM_L1 + PARTS) == set(SHAPES)


def n_parts(shape):
    return len(SHAPES[shape]['n_blocks'])


def n_rows(shape):
    return SHAPES[shape]['n_blocks'][0] * SHAPES[shape]['width']


def build_args(shape, k):
    return dict(SHAPES[shape], k=k)


def owned_blocks(n_blocks, world, rank):
    """[first, last) of the block rows of a part of n_blocks that `rank`
    owns: ArrowSlimMPI's contiguous spans."""
    bpr = -(-n_blocks // world)
    first = min(rank * bpr, n_blocks)
    return first, min(first + bpr, n_blocks)


# ---------------------------------------------------------------------------
# cases and children
# ---------------------------------------------------------------------------

# which engines get allreduce_x0 = True: none; part 0's (at L = 1 that is
# every engine, what bench.py sets for the iterated loop); every part's
OPTIONS = ('plain', 'x0', 'x0all')


class Case(NamedTuple):
    world: int
    shape: str
    precision: str
    k: int
    options: str
    variables: dict


def case_name(case):
    return f'{case.shape}_{case.precision}_k{case.k}_{case.options}'


REFUSAL = 'refuse_bf16_zero_rhs'
# jobs whose branch exists on the 'cuda' device only
GPU_ONLY = (REFUSAL,)

_QUEUE = ecq.QUEUE_ENVS['policy']
assert _QUEUE == {'ARROW_Q_MIN_NNZ': '0'}
# child -> (world, variables, ((shape, options), ...), refusal job)
CHILDREN = {
    # the chunked reduce and the broadcast; the deferred allreduce
    'w2': (2, {}, [(s, 'plain') for s in ('w64x4', 'w64x3', 'w6x4')]
           + [(s, 'x0') for s in ('w64x4', 'w64x3')], True),
    # w64x2 and w64x4 leave the last rank without a block
    'w3': (3, {}, [(s, 'plain') for s in ('w64x2', 'w64x4', 'w64x3')]
           + [(s, 'x0') for s in ('w64x2', 'w64x4')], False),
    # the same allreduce_x0 jobs, waited inside their step; and every part's
    # engine with the cached X_0 at L = 2 (valid without deferral only: the
    # aggregate adds into part 0's head rows after its spmm)
    'w2_nodefer': (2, {'ARROW_X0_DEFER': '0'},
                   [(s, 'x0') for s in ('w64x4', 'w64x3')]
                   + [('l2_4_2', 'x0all')], False),
    'w3_nodefer': (3, {'ARROW_X0_DEFER': '0'},
                   [(s, 'x0') for s in ('w64x2', 'w64x4')], False),
    'w2_chunks8': (2, {'ARROW_ROW0_CHUNKS': '8'},
                   [('w64x4', 'plain'), ('w64x4', 'x0')], False),
    # the collectives are posted while the side stream is current
    'w2_par': (2, {'ARROW_PAR_ROW0': '1'},
               [('w64x4', 'plain'), ('w64x4', 'x0')], False),
    'w2_parts': (2, {}, [(s, 'plain') for s in PARTS], False),
    'w3_parts': (3, {}, [(s, 'plain') for s in PARTS], False),
    # the multi-rank structures launched by the queue kernels
    'w2_queue': (2, dict(_QUEUE),
                 [('w64x4', 'plain'), ('w64x4', 'x0'), ('l2_4_2', 'plain'),
                  ('band4', 'plain')], False),
}
QUEUE_CHILD = 'w2_queue'
# (deferred child, child started with ARROW_X0_DEFER=0) at world 2, where
# the sum of two ranks does not depend on its order
DEFER_PAIRS = (('w2', 'w2_nodefer'),)


def world_of(child):
    return CHILDREN[child][0]


def child_variables(child):
    return dict(CHILDREN[child][1])


def cases(child):
    """The child's cases, in the order every rank runs them."""
    world, variables, pairs, _ = CHILDREN[child]
    return [Case(world, shape, p, k, options, dict(variables))
            for shape, options in pairs for p in PRECISIONS for k in K_OF[p]]


def job_names(child):
    """What the ranks run and the launcher prints, one line each."""
    names = [case_name(c) for c in cases(child)]
    return names + [REFUSAL] if CHILDREN[child][3] else names


def x0_names(child):
    """The real-class allreduce_x0 jobs of a child at L = 1: their lines
    carry per-step digests."""
    return [case_name(c) for c in cases(child) if c.options == 'x0']


for _child, (_world, _vars, _pairs, _) in CHILDREN.items():
    for _shape, _opt in _pairs:
        assert _shape in SHAPES and _opt in OPTIONS
        # the cached X_0 of one part is the iterated loop's, at L = 1
        assert _opt != 'x0' or n_parts(_shape) == 1
        assert _opt != 'x0all' or _vars.get('ARROW_X0_DEFER') == '0'
for _a, _b in DEFER_PAIRS:
    assert world_of(_a) == world_of(_b) == 2
    assert x0_names(_a) == x0_names(_b) and x0_names(_a)


# time limits: a child costs process start-up of its ranks plus a few
# seconds. EXPECTED_S is each child's wall time measured once on an MI355X
# (profiles/engine_rank_children.txt), rounded up for a cold start; the
# child's limit is TIMEOUT_FACTOR times that, as in test_gpu_queue_engine.py.
# A rank's own limit (the launcher's) sits below the child's, and the
# collectives' timeout well below the rank's: a mismatched collective
# schedule raises in every rank instead of hanging.
EXPECTED_S = {'w2': 20, 'w3': 20, 'w2_parts': 20, 'w3_parts': 20}
EXPECTED_DEFAULT_S = 15
TIMEOUT_FACTOR = 4


def child_limit(child):
    return TIMEOUT_FACTOR * EXPECTED_S.get(child, EXPECTED_DEFAULT_S)


def rank_limit(child):
    return 0.75 * child_limit(child)


def collective_timeout(child):
    return 0.25 * child_limit(child)


# ---------------------------------------------------------------------------
# the exact class
# ---------------------------------------------------------------------------

MAX_ROW_TERMS = ecq.MAX_ROW_TERMS
X_MAX = ecq.X_MAX
_SEED = 20261
EXACT_STEPS = 4


@functools.lru_cache(maxsize=None)
def decomposition(shape):
    """The shape's synth decomposition (the real class)."""
    return esd.make_decomp(**SHAPES[shape])


@functools.lru_cache(maxsize=None)
def exact_decomposition(shape):
    """decomposition(shape), pattern and permutations unchanged, every part's
    data redrawn from EXACT_VALS by a fixed seed."""
    rng = np.random.default_rng([_SEED, SHAPES[shape]['seed']])
    out = []
    for B, perm in decomposition(shape):
        B = B.copy()
        B.data = sc.EXACT_VALS[rng.integers(0, sc.EXACT_VALS.size, B.nnz)]
        out.append((B, perm))
    return out


def recomposed(decomp):
    """The float64 matrix of a decomposition, original row order: where
    parts overlap the engine adds their contributions in its own precision,
    it never forms a sum of A's values."""
    from arrow_matrix_amd import synth
    return synth.recompose([(B.astype(np.float64), p)
                            for B, p in decomp]).tocsr()


@functools.lru_cache(maxsize=None)
def exact_matrix(shape):
    return recomposed(exact_decomposition(shape))


@functools.lru_cache(maxsize=None)
def real_matrix(shape):
    return recomposed(decomposition(shape))


def exact_budget(shape):
    """(longest row in stored values over all parts, the largest magnitude a
    partial sum of one output element can reach, in half-units)."""
    longest = int(ecq.row_terms(exact_decomposition(shape)).max())
    vmax = float(np.abs(sc.EXACT_VALS).max())
    return longest, longest * vmax * X_MAX / 0.5


for _shape in SHAPES:
    _longest, _units = exact_budget(_shape)
    assert _longest <= MAX_ROW_TERMS, (_shape, _longest)
    assert _units < 2 ** 24, (_shape, _units)
assert all(float(v * x / 0.5).is_integer()
           for v in sc.EXACT_VALS for x in range(-X_MAX, X_MAX + 1))


def exact_features(shape, k, step):
    """Integers in [-8, 8] as float64, original row order; new ones for
    every step."""
    rng = np.random.default_rng([_SEED, SHAPES[shape]['seed'], k, step])
    return rng.integers(-X_MAX, X_MAX + 1,
                        (n_rows(shape), k)).astype(np.float64)


def exact_reference(shape, k, step):
    """A @ X in float64 on the recomposed exact matrix, in part 0's order:
    what the gathered result holds after a step from exact_features."""
    perm0 = exact_decomposition(shape)[0][1]
    return np.asarray(exact_matrix(shape)
                      @ exact_features(shape, k, step))[perm0]


# ---------------------------------------------------------------------------
# the real class
# ---------------------------------------------------------------------------

REAL_STEPS = 4


def real_features(shape, k, precision):
    """Uniform in [-1, 1) in the engine's precision, original row order."""
    rng = np.random.default_rng([_SEED, SHAPES[shape]['seed'], k, 77])
    dt = np.float64 if precision == 'float64' else np.float32
    return (2 * rng.random((n_rows(shape), k)) - 1).astype(dt)


def head_rows(decomp, width):
    """The rows, in original numbering, that are block row 0 of some part:
    the rows whose result is reduced over the ranks."""
    head = np.zeros(decomp[0][1].size, dtype=bool)
    for _, perm in decomp:
        head[perm[:width]] = True
    return head


def step_bound(A, absA, X, L, precision, world, head):
    """(golden, bound) of one plain step X <- A @ X over `world` ranks from
    the float64 features X (original row order). Per element

        |C - G| <= (2 n_row + 2 L + 8 + 2 W [row in head]) u  |A| @ |X|

    The first three terms are engine_affine_driver.step_bound's at (alpha,
    gamma) = (1, 0): one rounding per product and per add of the row's
    chain, one add per part that is accumulated, its constant, all doubled
    so that it holds with fma or without; u = 2**-24 (float64: 2**-53). The
    last is the C_0 reduce: block row 0 of every part is computed as one
    partial per rank and the W partials are added, in whatever order the
    backend chooses: at most one more add per rank, doubled like the rest.
    Every partial sum is bounded by the row's |A| @ |X|. Derived, not
    measured."""
    n_row = np.diff(A.indptr).astype(np.float64)
    u = 2.0 ** -53 if precision == 'float64' else 2.0 ** -24
    factor = (2.0 * n_row + 2.0 * L + 8.0 + 2.0 * world * head) * u
    return np.asarray(A @ X), factor[:, None] * np.asarray(absA @ np.abs(X))
