"""Engine steps under the per-XCD queue schedulers, every layout.

The engines never call set_queue, and the structures of the engine tests are
far below the policy's nnz threshold: without ARROW_Q_MIN_NNZ every engine
step of the suite is launched grid-stride. Each (queue environment, layout)
pair of tests/engine_cases_queue.py runs in a fresh child
(tests/engine_queue_driver.py) that starts with the kernel variables and the
layout variables together, one after another; one more child replays a
captured pair of queued steps three times. The children assert the launch
plan of every resident structure, compare the exact class bit for bit with
the float64 reference and the real class to the engine drivers' bounds, and
log one JSON line per job. This module never initialises the GPU itself.

If a child ends with a signal, an abort/segfault/timeout status, errored or
at its time limit, nothing further is started on the GPU
(tests/gpu_children.py).
"""
import os

import pytest

from tests import engine_cases_queue as ecq
from tests import gpu_children
from tests.spmm_cases import KERNEL_VARS

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(gpu_children.REPO, 'tests', 'engine_queue_driver.py')
STRIP = KERNEL_VARS + gpu_children.ENGINE_VARS

# expected seconds per child: each measured once on an MI355X, 2.6-3.4 s with
# warm file caches (profiles/engine_queue_children.txt; process start and GPU
# initialisation are most of it), allowing for a cold start. The limit is a
# few times that.
EXPECTED_S = {'hub': 12}
EXPECTED_DEFAULT_S = 10
TIMEOUT_FACTOR = 4


def _limit(name):
    return TIMEOUT_FACTOR * EXPECTED_S.get(name, EXPECTED_DEFAULT_S)


@pytest.mark.parametrize('queue_env,layout', ecq.children())
def test_layout_under_queue_scheduler(queue_env, layout):
    """Every job of the child ran and passed, and every resident structure
    it launched was planned for the queue scheduler K_OF names.

    [policy-split_col] caught the engine storing a bf16 element three times
    under ARROW_SPLIT_COL=1 with an affine step (rest launch, hub-sorted
    beta = 1 launch, tail): bfloat16_k32_affine reached 1.0756 of
    engine_affine_driver.step_bound, which counts two roundings, whatever
    the scheduler. The layout's launches now carry the step
    (ArrowSlimMPI._split_col_carries)."""
    jobs = ecq.jobs(queue_env, layout)
    lines = gpu_children.child_ok(
        (DRIVER, queue_env, layout), [DRIVER, queue_env, layout],
        ecq.child_variables(queue_env, layout), STRIP, _limit(layout),
        f"queue engine child '{queue_env} {layout}'",
        [name for name, *_ in jobs])
    assert set(lines) == {name for name, *_ in jobs}
    for name, precision, k, tier in jobs:
        ln = lines[name]
        want = ecq.expected_plan(queue_env, precision, k)['scheduler']
        assert ln['plans'] == [ecq.SCHED_NAME[want]], name
        assert want in (ecq.QWAVE, ecq.QBLOCK)
        assert (ln['queue_env'], ln['mode']) == (queue_env, layout)
        assert ln['max_err_over_bound'] <= 1.0
        inside = tier == 'plain' or layout in ecq.AFFINE_INSIDE
        assert ln['tails'] == (0 if inside else 3), name
        if tier == 'affine_norm':
            fused = layout in ecq.NORM_FUSED
            assert (ln['fused_launches'], ln['stand_alone']) == \
                ((2, 0) if fused else (0, 2)), name


def test_captured_queued_steps_replay_to_the_eager_bits():
    """A captured pair of queued steps, replayed three times from restored
    features into NaN-filled results, gives the eager pair's bits every
    time: the chunk counters' reset is a node of the graph."""
    names = [ecq.capture_job_name(*job) for job in ecq.CAPTURE_JOBS]
    lines = gpu_children.child_ok(
        (DRIVER, 'capture'), [DRIVER, 'capture'], ecq.QUEUE_ENVS['policy'],
        STRIP, _limit('capture'), "queue engine child 'capture'", names)
    assert set(lines) == set(names)
    for (precision, layout, k), name in zip(ecq.CAPTURE_JOBS, names):
        want = ecq.expected_plan('policy', precision, k)['scheduler']
        assert lines[name]['plans'] == [ecq.SCHED_NAME[want]], name
        assert lines[name]['replays'] == 3
