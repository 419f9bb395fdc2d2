"""tests/engine_cases_ranks.py and tests/engine_ranks_driver.py without a GPU:
the exactness budget of every shape, the bound, the job names, the rank role
itself on the cpu device over gloo at world 2 and 3 (which shows that the
references and bounds can be met and that the checks are right), and the
launcher's three outcomes with stub ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import child_harness as ch
from tests import engine_affine_driver as ead
from tests import engine_cases_queue as ecq
from tests import engine_cases_ranks as ecr
from tests import engine_ranks_driver as erd
from tests import gpu_children as gc
from tests import spmm_cases as sc
from tests import test_distributed_gloo as tdg

ENV_STRIP = erd.START_VARS + ('RANK', 'WORLD_SIZE', 'LOCAL_RANK',
                              'MASTER_ADDR', 'MASTER_PORT')


# ---------------------------------------------------------------------------
# shapes, budget, bound
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('shape', list(ecr.SHAPES))
def test_exactness_budget(shape):
    """The longest row of the recomposed pattern, counted in stored values
    over all parts, is within the budget; pattern and permutations are the
    synth decomposition's; values and features are of the exact class."""
    decomp, synth = ecr.exact_decomposition(shape), ecr.decomposition(shape)
    assert len(decomp) == len(synth) == ecr.n_parts(shape)
    for (B, p), (S, q) in zip(decomp, synth):
        assert (B.indptr == S.indptr).all() and (B.indices == S.indices).all()
        assert (p == q).all()
        assert np.isin(B.data, sc.EXACT_VALS).all() and B.dtype == np.float32
    terms = ecq.row_terms(decomp)
    assert terms.sum() == sum(B.nnz for B, _ in decomp)
    longest, units = ecr.exact_budget(shape)
    assert longest == terms.max() <= ecr.MAX_ROW_TERMS == 8192
    assert units == longest * 2 * 8 / 0.5 < 2 ** 24
    for k in sorted({k for p in ecr.PRECISIONS for k in ecr.K_OF[p]}):
        seen = []
        for step in range(ecr.EXACT_STEPS):
            X = ecr.exact_features(shape, k, step)
            assert X.shape == (ecr.n_rows(shape), k)
            assert (X == np.round(X)).all() and np.abs(X).max() == 8
            assert not any((X == Y).all() for Y in seen)
            seen.append(X)
            G = ecr.exact_reference(shape, k, step)
            assert (G.astype(np.float32).astype(np.float64) == G).all()
            assert np.abs(G).max() > 0


def test_shapes_are_the_suites():
    """The shapes are test_distributed_gloo._worker's tuples and the engine
    drivers' L1 / L2 / BANDED; only k moves, to engine_cases_queue.K_OF's."""
    import ast
    import inspect
    source = inspect.getsource(tdg._worker)
    for name, text in (('w64x2', '([2], 64, 4, 9, False)'),
                       ('w6x4', '([4], 6, 5, 0, False)'),
                       ('l2_3_2', '([3, 2], 4, 4, 2, False)'),
                       ('l3_4_3_2', '([4, 3, 2], 4, 6, 3, False)'),
                       ('band5', '([5], 4, 3, 8, True)')):
        assert text in source
        n_blocks, width, _, seed, banded = ast.literal_eval(text)
        shape = ecr.SHAPES[name]
        assert (shape['n_blocks'], shape['width'], shape['seed']) == \
            (n_blocks, width, seed)
        assert (shape.get('slim', True), shape.get('block_diagonal', True)) \
            == (not banded, not banded)
    for name, base in (('w64x3', ead.L1), ('l2_4_2', ead.L2),
                       ('band4', ead.BANDED)):
        assert ecr.build_args(name, base['k']) == base
    assert ecr.build_args('w64x4', 32) == dict(ead.L1, n_blocks=[4])
    for p in ecr.PRECISIONS:
        assert ecr.K_OF[p] == tuple(row[0] for row in ecq.K_OF[p])
        assert [row[3] for row in ecq.K_OF[p]] == [ecq.QWAVE, ecq.QBLOCK]


def test_spans_cover_what_the_issue_names():
    own = ecr.owned_blocks
    # two blocks a rank; four chunks from width 64 on
    assert [own(4, 2, r) for r in range(2)] == [(0, 2), (2, 4)]
    assert ecr.SHAPES['w64x4']['width'] == 64 > ecr.SHAPES['w6x4']['width']
    # a rank that owns nothing, with one peer or two that do
    assert [own(2, 3, r) for r in range(3)] == [(0, 1), (1, 2), (2, 2)]
    assert [own(4, 3, r) for r in range(3)] == [(0, 2), (2, 4), (4, 4)]
    # uneven spans
    assert [own(3, 2, r) for r in range(2)] == [(0, 2), (2, 3)]
    assert [own(5, 2, r) for r in range(2)] == [(0, 3), (3, 5)]
    assert [own(5, 3, r) for r in range(3)] == [(0, 2), (2, 4), (4, 5)]


def test_step_bound_is_the_affine_drivers_plus_the_reduce():
    """At W = 0 it is engine_cases_queue.plain_step_bound (the affine
    driver's at alpha 1, gamma 0); W ranks add 2 W u |A|@|X| on the rows
    that are block row 0 of a part, and nothing elsewhere."""
    shape = 'l2_4_2'
    decomp = ecr.decomposition(shape)
    A = ecr.real_matrix(shape)
    absA = abs(A)
    X = ecr.real_features(shape, 8, 'float64').astype(np.float64)
    w = ecr.SHAPES[shape]['width']
    head = ecr.head_rows(decomp, w)
    assert w <= head.sum() <= 2 * w
    assert head[decomp[0][1][:w]].all() and head[decomp[1][1][:w]].all()
    mag = np.asarray(absA @ np.abs(X))
    for precision, u in (('float32', 2.0 ** -24), ('float64', 2.0 ** -53)):
        G0, b0 = ecr.step_bound(A, absA, X, 2, precision, 0, head)
        G1, b1 = ecq.plain_step_bound(A, absA, X, 2, precision)
        assert (G0 == G1).all() and (b0 == b1).all()
        for world in (2, 3):
            G, b = ecr.step_bound(A, absA, X, 2, precision, world, head)
            assert (G == G0).all()
            np.testing.assert_allclose(
                b - b0, 2 * world * u * head[:, None] * mag, rtol=1e-9,
                atol=0)
            assert (b[~head] == b0[~head]).all() and (b[head] > b0[head]).any()


# ---------------------------------------------------------------------------
# children and job names
# ---------------------------------------------------------------------------

def test_children_and_job_names():
    assert list(ecr.CHILDREN) == [
        'w2', 'w3', 'w2_nodefer', 'w3_nodefer', 'w2_chunks8', 'w2_par',
        'w2_parts', 'w3_parts', 'w2_queue']
    every = []
    for child in ecr.CHILDREN:
        world, variables = ecr.world_of(child), ecr.child_variables(child)
        assert world in (2, 3) and child.startswith(f'w{world}')
        assert set(variables) <= set(erd.START_VARS)
        cases = ecr.cases(child)
        names = ecr.job_names(child)
        assert len(set(names)) == len(names)
        assert names[:len(cases)] == [ecr.case_name(c) for c in cases]
        assert names[len(cases):] in ([], [ecr.REFUSAL])
        for c in cases:
            assert c.world == world and c.variables == variables
            assert c.k in ecr.K_OF[c.precision]
            assert ecr.case_name(c) == \
                f'{c.shape}_{c.precision}_k{c.k}_{c.options}'
        # both precisions, both widths of each
        for shape, options in {(c.shape, c.options) for c in cases}:
            assert {(c.precision, c.k) for c in cases
                    if (c.shape, c.options) == (shape, options)} == \
                {(p, k) for p in ecr.PRECISIONS for k in ecr.K_OF[p]}
        every += [(child, n) for n in names]
        # limits: a rank's below the child's, the collectives' well below
        assert ecr.collective_timeout(child) * 2 < ecr.rank_limit(child) \
            < ecr.child_limit(child)
    assert len(every) == len(set(every))
    # what the issue asks to be covered
    has = {(ecr.world_of(ch_), c.shape, c.options,
            tuple(sorted(c.variables.items())))
           for ch_ in ecr.CHILDREN for c in ecr.cases(ch_)}
    for want in [(2, 'w64x4', 'plain', ()), (3, 'w64x2', 'plain', ()),
                 (2, 'w64x4', 'plain', (('ARROW_ROW0_CHUNKS', '8'),)),
                 (2, 'w64x4', 'x0', ()), (3, 'w64x4', 'x0', ()),
                 (2, 'w64x4', 'x0', (('ARROW_X0_DEFER', '0'),)),
                 (3, 'w64x4', 'x0', (('ARROW_X0_DEFER', '0'),)),
                 (2, 'w64x4', 'plain', (('ARROW_PAR_ROW0', '1'),)),
                 (2, 'w64x4', 'x0', (('ARROW_PAR_ROW0', '1'),)),
                 (2, 'w64x4', 'x0', (('ARROW_Q_MIN_NNZ', '0'),))] \
            + [(w, s, 'plain', ()) for w in (2, 3) for s in ecr.PARTS]:
        assert want in has, want
    assert ecr.child_variables(ecr.QUEUE_CHILD) == ecq.QUEUE_ENVS['policy']
    assert ecr.REFUSAL in ecr.job_names('w2')
    assert ecr.DEFER_PAIRS == (('w2', 'w2_nodefer'),)


# ---------------------------------------------------------------------------
# the rank role on the cpu device, through the launcher
# ---------------------------------------------------------------------------

def _launch(child):
    env = {k: v for k, v in os.environ.items() if k not in ENV_STRIP}
    env.update(ecr.child_variables(child))
    p = subprocess.run([sys.executable, erd.DRIVER, 'launch', child, 'cpu'],
                       env=env, cwd=ch.REPO, capture_output=True, text=True,
                       timeout=ecr.child_limit(child))
    return p.returncode, gc.json_lines(p.stdout), p.stderr[-3000:]


@pytest.mark.parametrize('child', ['w2', 'w3', 'w2_parts', 'w3_parts'])
def test_rank_role_on_the_cpu_device(child):
    """The same rank role, device='cpu' over gloo: every job that is not
    GPU-only passes on every rank, the exact class bit for bit, the real
    class within the bound; the launcher prints the job names, merged."""
    rc, lines, stderr = _launch(child)
    assert rc == 0, stderr
    skipped = [n for n in ecr.job_names(child) if n not in lines]
    assert skipped == ([ecr.REFUSAL] if child == 'w2' else [])
    assert set(skipped) <= set(ecr.GPU_ONLY)
    assert list(lines) == [n for n in ecr.job_names(child)
                           if n not in ecr.GPU_ONLY]
    world = ecr.world_of(child)
    for case in ecr.cases(child):
        ln = lines[ecr.case_name(case)]
        assert ln['ok'] is True and 'rank' not in ln
        assert (ln['child'], ln['world'], ln['ranks'], ln['device']) == \
            (child, world, world, 'cpu')
        assert ln['exact_mismatch'] == 0
        assert 0 < ln['max_err_over_bound'] <= 1.0
        assert ('digests' in ln) == (case.options == 'x0')


# ---------------------------------------------------------------------------
# merge
# ---------------------------------------------------------------------------

def test_merge():
    ok = dict(case='a', ok=True, rank=0, max_err_over_bound=0.25,
              exact_mismatch=0, plans=['QWAVE'], digests=['x', 'y'], ms=3.0)
    other = dict(ok, rank=1, max_err_over_bound=0.5, plans=['QBLOCK'],
                 digests=['no'], ms=5.0)
    m, = erd.merge(['a', 'b'], [{'a': ok}, {'a': other}])
    assert m == dict(case='a', ok=True, ranks=2, max_err_over_bound=0.5,
                     exact_mismatch=0, plans=['QBLOCK', 'QWAVE'],
                     digests=['x', 'y'], ms=5.0)
    bad = dict(case='a', ok=False, rank=1, error='differs')
    m, = erd.merge(['a'], [{'a': ok}, {'a': bad}])
    assert m['ok'] is False and m['error'] == 'rank 1: differs'
    assert 'errored' not in m
    m, = erd.merge(['a'], [{'a': ok}, {}, {'a': dict(bad, errored=True)}])
    assert m['ok'] is False and m['errored'] is True and m['ranks'] == 3
    assert m['error'] == 'rank 1: no line; rank 2: differs'


# ---------------------------------------------------------------------------
# the launcher's outcomes, with stub ranks
# ---------------------------------------------------------------------------

def _stub(code):
    return [sys.executable, '-c', code]


LINE = "import json; print(json.dumps(dict(case='a', ok=True)), flush=True); "
WAIT = "import time; time.sleep(60)"
# started in the repository root, as the launcher starts every rank
RAISES = ("import sys; sys.path.insert(0, '.'); "
          "from tests import engine_ranks_driver as d; "
          "sys.exit(d.guarded(lambda: 1 / 0))")


@pytest.fixture
def starts(monkeypatch):
    started = []
    popen = subprocess.Popen

    def counted(argv, **kwargs):
        started.append(kwargs['env']['RANK'])
        return popen(argv, **kwargs)
    monkeypatch.setattr(erd.subprocess, 'Popen', counted)
    return started


def test_launcher_all_ranks_ok(starts):
    code = LINE + "import os; assert os.environ['WORLD_SIZE'] == '3' and " \
        "os.environ['MASTER_ADDR'] == '127.0.0.1' and " \
        "int(os.environ['MASTER_PORT']) > 0"
    status, texts = erd.run_ranks([_stub(code)] * 3, 60)
    assert status == 0 and starts == ['0', '1', '2']
    assert [json.loads(t)['case'] for t in texts] == ['a'] * 3


def test_launcher_passes_on_a_failed_rank(starts):
    """A rank that exits 1: the peers (waiting for it) are ended, nothing
    more is started, the launcher's status is 1 and does not latch."""
    status, texts = erd.run_ranks(
        [_stub(LINE + WAIT), _stub(LINE + "raise SystemExit(1)"),
         _stub(WAIT)], 60)
    assert status == 1 and starts == ['0', '1', '2']
    assert status not in gc.FATAL_STATUS + (ch.EXIT_ERRORED,)
    assert [t.count('"case"') for t in texts] == [1, 1, 0]


def test_launcher_passes_on_an_errored_rank(starts):
    status, _ = erd.run_ranks([_stub(WAIT), _stub(RAISES)], 60)
    assert status == ch.EXIT_ERRORED and starts == ['0', '1']


def test_launcher_ends_every_rank_at_the_limit(starts):
    """A rank past its limit is killed along with its peers: status 124, one
    of gpu_children.FATAL_STATUS."""
    status, texts = erd.run_ranks([_stub(LINE + WAIT), _stub(WAIT)], 0.5)
    assert status == 124 in gc.FATAL_STATUS and starts == ['0', '1']
    assert len(texts) == 2


def test_exit_status_of_a_signal():
    assert [erd.exit_status(rc) for rc in (0, 1, 70, -6, -11, -9)] == \
        [0, 1, 70, 134, 139, 137]
    assert erd.exit_status(-15) == ch.EXIT_ERRORED      # latches all the same
    for rc in (-6, -11, -9, -15, -7):
        assert erd.exit_status(rc) in gc.FATAL_STATUS + (ch.EXIT_ERRORED,)
