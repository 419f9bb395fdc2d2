"""Engine steps under the per-XCD queue schedulers, and the child entry point
of test_gpu_queue_engine.py:

    python tests/engine_queue_driver.py <queue_env> <layout>
    python tests/engine_queue_driver.py capture

The first form runs one (queue environment, layout) pair of
tests/engine_cases_queue.py in a process that starts with both sets of
variables: one job per (precision, k of K_OF, tier), each printing one JSON
line through the job loop of tests/child_harness.py. A job asserts that every
resident structure of its engines is planned for the queue scheduler meant,
runs one step of the exact class against the float64 reference bit for bit,
three steps of the real class to the engine drivers' bound, and the tail and
norm counters of its tier. The second form replays a captured pair of queued
steps three times against the same pair run eagerly. Built on the other
engine drivers; this is a plain module, not a test file.
"""
import sys

import numpy as np

if not __package__:         # started as a script: see tests/child_harness.py
    import child_harness  # noqa: F401
from tests import child_harness as ch  # noqa: E402

from tests import engine_affine_driver as ead  # noqa: E402
from tests import engine_cases_queue as ecq  # noqa: E402
from tests import engine_norm_driver as end  # noqa: E402
from tests import engine_scale_driver as esd  # noqa: E402
from tests import spmm_cases_bf16 as s16  # noqa: E402
from tests import spmm_cases_norm as sn  # noqa: E402
from tests.gpu_children import ENGINE_VARS  # noqa: E402
from tests.spmm_cases import KERNEL_VARS  # noqa: E402

REAL_STEPS = 3


# ---------------------------------------------------------------------------
# 1. the scheduler that runs is the one meant
# ---------------------------------------------------------------------------

def resident_structures(arrow):
    """Every structure a step of `arrow` launches, once each."""
    seen = {}
    for eng in arrow.engines:
        for blk, *_ in eng._operator_structures():
            seen[id(blk)] = blk
        if eng._A_col is not None:
            seen[id(eng._A_col)] = eng._A_col
    for blk in arrow._folded or []:
        seen[id(blk)] = blk
    return list(seen.values())


def check_layout(layout, arrow):
    """The layout the environment asked for is the one that was built."""
    esd.assert_layout(layout, arrow, 'gpu')
    eng0 = arrow.engines[0]
    if layout == 'split_col':
        assert eng0._A_all is None and eng0._A_col is not None
    elif layout == 'row0_chunks':
        assert eng0._A_all is None and len(eng0._A_row0) == 4
    elif layout == 'rest_chunks':
        assert eng0._A_all is None and len(eng0._A_rest) > 1
    if layout.startswith('fold') and layout != 'fold0':
        assert len(arrow._folded) == arrow.decomposition_length - 1


def check_plans(queue_env, layout, arrow, precision, k):
    """Every resident structure, at its own nnz and the handle mode the
    engines leave (-1), gets the plan of the table under this process's
    environment. Returns the scheduler names seen."""
    from arrow_matrix_amd import hip
    check_layout(layout, arrow)
    want = ecq.expected_plan(queue_env, precision, k)
    assert want['scheduler'] in (ecq.QWAVE, ecq.QBLOCK)
    blocks = resident_structures(arrow)
    assert blocks, "no resident structure"
    seen = set()
    for blk in blocks:
        got = hip.spmm_plan(k, blk.nnz, -1, ead.dtype_of(precision))
        assert got == want, f"nnz {blk.nnz}: plan {got}, expected {want}"
        seen.add(ecq.SCHED_NAME[got['scheduler']])
    return seen


# ---------------------------------------------------------------------------
# 2. the exact class: one step, bit for bit
# ---------------------------------------------------------------------------

def np_dtype(precision):
    return np.float64 if precision == 'float64' else np.float32


def result_bits(arrow, precision):
    """The result tile's raw bits on the host."""
    import torch
    C = arrow.B.result_tile().contiguous()
    word = {'float32': torch.int32, 'float64': torch.int64,
            'bfloat16': torch.int16}[precision]
    return C.view(word).cpu().numpy().view(
        {'float32': np.uint32, 'float64': np.uint64,
         'bfloat16': np.uint16}[precision])


def reference_bits(G, precision):
    if precision == 'bfloat16':
        return s16.bf16_bits(G)
    ref = G.astype(np_dtype(precision))
    assert (ref.astype(np.float64) == G).all()
    return ref.view(np.uint64 if precision == 'float64' else np.uint32)


def load_exact(layout, precision, k, tier):
    """An engine on exact_decomposition(layout) with the tier's step set."""
    dt = np_dtype(precision)
    arrow = esd.load(ecq.exact_decomposition(layout), precision, 'gpu',
                     **ecq.build_args(layout, k))
    X, R, perm0 = ecq.exact_operands(layout, k)
    arrow.B.set_features(X[perm0].astype(dt))
    if tier != 'plain':
        arrow.set_affine_step(ecq.EXACT_ALPHA, ecq.EXACT_GAMMA,
                              R[perm0].astype(dt))
    if tier == 'affine_norm':
        arrow.track_step_norms()
    return arrow


def run_exact(queue_env, layout, precision, k, tier):
    """Returns (schedulers seen, tail calls). bfloat16 features compare
    where one rounding happens per element; elsewhere the real class is
    their check."""
    import torch
    arrow = load_exact(layout, precision, k, tier)
    seen = check_plans(queue_env, layout, arrow, precision, k)
    tails = ead.TailCounter(arrow.engines[0].backend)
    x64 = arrow.B.feature_tile().to(torch.float64).cpu().numpy()
    arrow.step()
    G = ecq.exact_reference(layout, k, tier)
    assert np.abs(G).max() > 0
    if precision != 'bfloat16' or layout in ecq.BF16_ROUNDS_ONCE:
        got, want = result_bits(arrow, precision), \
            reference_bits(G, precision)
        if not (got == want).all():
            c64 = arrow.B.result_tile().to(torch.float64).cpu().numpy()
            raise ch.Mismatch(
                f"exact {precision} k={k} {tier}: {int((got != want).sum())} "
                f"of {got.size} elements differ in "
                f"{int((got != want).any(axis=1).sum())} rows, max |diff| "
                f"{float(np.abs(c64 - G).max())}")
    c64 = arrow.B.result_tile().to(torch.float64).cpu().numpy()
    assert np.isfinite(c64).all() and np.abs(c64).max() > 0
    if tier == 'affine_norm':
        acc = end._acc(arrow)
        s0, s1 = sn.host_sums(c64, x64)
        b0, b1 = sn.norm_bound(end.PREC_TAG[precision], c64.size, s0, s1)
        assert abs(acc[0] - s0) <= b0 and abs(acc[1] - s1) <= b1, \
            f"exact step norms: acc {acc} host {[s0, s1]} bound {[b0, b1]}"
    return seen, tails.calls


# ---------------------------------------------------------------------------
# 3. the real class: three steps to the bound
# ---------------------------------------------------------------------------

def run_plain_steps(arrow, A, perm0, precision, iters=REAL_STEPS):
    """engine_affine_driver.run_steps for the plain step X <- A @ X."""
    L = arrow.decomposition_length
    absA = abs(A)
    worst = 0.0
    for step in range(iters):
        Xin = ead.held(arrow.B.feature_tile(), perm0)
        arrow.step()
        C = arrow.B.allgather_result().astype(np.float64)
        G, bound = ecq.plain_step_bound(A, absA, Xin, L, precision)
        err = np.abs(C - G[perm0])
        ratio = float((err / np.maximum(bound[perm0], 1e-300)).max())
        print(f"# {precision} plain step {step}: max err/bound {ratio:.3f}, "
              f"max |G| {float(np.abs(G).max()):.3f}", file=sys.stderr)
        assert np.isfinite(C).all()
        assert (err <= bound[perm0]).all(), \
            f"{precision} plain step {step}: max err/bound {ratio}"
        assert np.abs(G).max() > 0
        worst = max(worst, ratio)
        arrow.B.set_features(arrow.B.result_tile())
    return worst


def run_real(queue_env, layout, precision, k, tier):
    """Returns (schedulers seen, tail calls, worst err / bound)."""
    arrow, A, perm0, X, R = ead.build(precision=precision,
                                      **ecq.build_args(layout, k))
    seen = check_plans(queue_env, layout, arrow, precision, k)
    tails = ead.TailCounter(arrow.engines[0].backend)
    arrow.B.set_features(X[perm0].copy())
    if tier == 'plain':
        worst = run_plain_steps(arrow, A, perm0, precision)
    else:
        arrow.set_affine_step(ead.ALPHA, ead.GAMMA, R[perm0].copy())
        if tier == 'affine_norm':
            arrow.track_step_norms()
        worst = max(f[0] for f in ead.run_steps(arrow, A, perm0, precision,
                                                iters=REAL_STEPS))
    return seen, tails.calls, worst


# ---------------------------------------------------------------------------
# the job of one (precision, k, tier)
# ---------------------------------------------------------------------------

def expected_tails(layout, tier, steps):
    """No tail kernel without an affine step or where the launches carry it;
    else one per step."""
    return 0 if tier == 'plain' or layout in ecq.AFFINE_INSIDE else steps


def run_job(queue_env, layout, precision, k, tier):
    seen, tails = run_exact(queue_env, layout, precision, k, tier)
    assert tails == expected_tails(layout, tier, 1), \
        f"exact step: {tails} tail calls"
    seen_real, tails, worst = run_real(queue_env, layout, precision, k, tier)
    assert tails == expected_tails(layout, tier, REAL_STEPS), \
        f"real steps: {tails} tail calls"
    info = dict(tails=tails, max_err_over_bound=worst)
    seen |= seen_real
    if tier == 'affine_norm':
        # tracked next to untracked, bit for bit; both accumulators to
        # spmm_cases_norm.norm_bound; who measured
        arrow, n_fused, n_alone, worst_norm = end.run_tracked(
            precision, True, **ecq.build_args(layout, k))
        seen |= check_plans(queue_env, layout, arrow, precision, k)
        end.check_counters(layout in ecq.NORM_FUSED, n_fused, n_alone)
        info.update(fused_launches=n_fused, stand_alone=n_alone,
                    norm_err_over_bound=worst_norm)
    info['plans'] = sorted(seen)
    want = ecq.SCHED_NAME[ecq.expected_plan(queue_env, precision,
                                            k)['scheduler']]
    assert info['plans'] == [want], info['plans']
    return info


# ---------------------------------------------------------------------------
# capture: a replayed pair of queued steps against the eager pair
# ---------------------------------------------------------------------------

REPLAYS = 3


def assert_order_free(arrow, layout, precision):
    """The step about to run is exact in every order: over the features as
    they are held, sum |a| |x| of every row, scaled by alpha, plus |gamma R|
    stays below 2**24 units of the grid its terms lie on (alpha * a * x with
    x a multiple of `grid`). Split-row atomics then land on the same bits
    whichever way they are scheduled, so an eager run and a replay can be
    compared bit for bit."""
    perm0 = ecq.exact_decomposition(layout)[0][1]
    x = ead.held(arrow.B.feature_tile(), perm0)
    r = ead.held(arrow.engines[0]._R, perm0)
    grid = 1.0
    while not (np.mod(x / grid, 1) == 0).all():
        grid /= 2
        assert grid >= 2.0 ** -20
    assert (np.mod(r, 1) == 0).all()
    unit = ecq.EXACT_ALPHA * 0.5 * grid      # |a| is a multiple of 0.5
    absA = abs(ecq.exact_matrix(layout))
    mag = ecq.EXACT_ALPHA * np.asarray(absA @ np.abs(x)) \
        + abs(ecq.EXACT_GAMMA) * np.abs(r)
    assert mag.max() / unit < 2 ** 24, \
        f"{precision} {layout}: {mag.max() / unit} units of {unit}"


def run_capture(precision, layout, k):
    import torch
    arrow = load_exact(layout, precision, k, 'affine')
    seen = check_plans('policy', layout, arrow, precision, k)
    eng0 = arrow.engines[0]
    F = eng0.feature_tile()              # the engine's copy of the features
    saved = F.clone()

    def pair(record):
        """step; X := C; step. record: called before each step."""
        outs = []
        for _ in range(2):
            if record:
                record()
            arrow.step()
            outs.append(eng0.result_tile())
            eng0.set_features(eng0.result_tile())
        return outs

    # warm-up: every allocation (the bf16 split-row scratch, the ping-pong
    # pool) happens here, outside any capture
    pair(None)
    torch.cuda.synchronize()
    # the eager pair, from the saved features; each step is checked to be
    # exact in every order first, so its bits do not depend on scheduling
    F.copy_(saved)
    eng0.set_features(F)
    eager = [t.clone() for t in
             pair(lambda: assert_order_free(arrow, layout, precision))]
    torch.cuda.synchronize()
    assert all(float(t.float().abs().max()) > 0 for t in eager)
    assert not torch.equal(eager[0], eager[1])
    # the same pair, captured as bench.py captures its two steps
    eng0.set_features(F)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = pair(None)
    assert len({F.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr()}) == 3
    for replay in range(REPLAYS):
        F.copy_(saved)
        for t in outs:                   # a row no workgroup takes stays NaN
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        for step, (got, want) in enumerate(zip(outs, eager)):
            same = got.view(torch.uint8) == want.view(torch.uint8)
            if not bool(same.all()):
                bad = (~same).any(dim=1)
                raise ch.Mismatch(
                    f"replay {replay} step {step}: {int(bad.sum())} of "
                    f"{bad.numel()} rows differ from the eager step, "
                    f"{int(torch.isnan(got.float()).any(dim=1).sum())} hold "
                    f"NaN")
    return dict(plans=sorted(seen), replays=REPLAYS,
                split_rows=layout == 'hub')


# ---------------------------------------------------------------------------

def main(argv):
    names = KERNEL_VARS + ENGINE_VARS
    if argv[1] == 'capture':
        variables = ecq.QUEUE_ENVS['policy']
        jobs = [(ecq.capture_job_name(p, layout, k),
                 lambda p=p, layout=layout, k=k: run_capture(p, layout, k))
                for p, layout, k in ecq.CAPTURE_JOBS]
        tags = {'queue_env': 'policy', 'mode': 'capture'}
    else:
        queue_env, layout = argv[1], argv[2]
        variables = ecq.child_variables(queue_env, layout)
        jobs = [(name, lambda p=p, k=k, tier=tier:
                 run_job(queue_env, layout, p, k, tier))
                for name, p, k, tier in ecq.jobs(queue_env, layout)]
        tags = {'queue_env': queue_env, 'mode': layout}
    ch.started_with(KERNEL_VARS, variables)
    ch.started_with(ENGINE_VARS, variables)
    assert set(variables) <= set(names)
    ch.open_gpu("the queue engine driver needs a GPU", set_device=False)
    return ch.run_jobs(jobs, tags)


if __name__ == '__main__':
    sys.exit(main(sys.argv))
