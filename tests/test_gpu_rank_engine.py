"""The multi-rank engine on the GPU, with the ranks of a world sharing one
device under gloo.

Everything the engines do only at comm.size > 1 (the chunked C_0 reduce and
its branch for a rank that owns nothing, the deferred C_0 allreduce of the
iterated loop, the overlapped X_0 broadcast, the overlapped forward exchange
and the aggregate at L > 1, the staged halo exchange of the banded engine,
all of it in float32 and float64) ran on the cpu device only, or at world 1.
Each child of tests/engine_cases_ranks.py is one world and one set of start-up
variables: this module starts its launcher (tests/engine_ranks_driver.py
launch <child>), which starts the W ranks as fresh processes and merges their
verdicts, one child after another, at most 3 ranks on the device at a time.
Every rank compares its own stripe and the gathered result: the exact class
bit for bit with the float64 reference, the real class to
engine_cases_ranks.step_bound. This module never initialises the GPU itself.

If a launcher ends with a signal, an abort/segfault/timeout status (a rank's
own is passed on), errored or at its time limit, nothing further is started
on the GPU (tests/gpu_children.py).
"""
import os

import pytest

from tests import engine_cases_ranks as ecr
from tests import gpu_children
from tests.spmm_cases import KERNEL_VARS

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(gpu_children.REPO, 'tests', 'engine_ranks_driver.py')
STRIP = KERNEL_VARS + gpu_children.ENGINE_VARS + (
    'ARROW_X0_DEFER', 'RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR',
    'MASTER_PORT')


def _child(child):
    """The merged lines of a child: every job ran on every rank, all ok."""
    names = ecr.job_names(child)
    lines = gpu_children.child_ok(
        (DRIVER, 'launch', child), [DRIVER, 'launch', child],
        ecr.child_variables(child), STRIP, ecr.child_limit(child),
        f"rank engine child '{child}'", names)
    assert list(lines) == names
    return lines


@pytest.mark.parametrize('child', list(ecr.CHILDREN))
def test_ranks_sharing_one_device(child):
    """Every job of the child ran on each of its W ranks and passed there:
    no bit of the exact class differs from the float64 reference, on any
    rank's own stripe or in the gathered result, and the real class stays
    within engine_cases_ranks.step_bound over four iterated steps. Under
    engine_cases_queue.QUEUE_ENVS['policy'] every resident structure of
    every rank is planned for a queue scheduler.

    [w2_parts], [w3_parts], [w2_queue] caught the banded engine adding a
    boundary off-diagonal's halo term into the wrong rows on the rank that
    owns block row 0: ArrowSlimMPI._spmm_gpu indexed C_i by the row offset
    inside the rest structure, which on that rank starts one tile below the
    stripe. band4_float32_k16_plain, rank 0, exact step 0: 384 of 1024
    elements of its own stripe differed, all in block row 1 (its halo term
    landed in block row 0, which the reduced C_0 then overwrote). The other
    ranks, world 1 and the cpu device were right. The launch now adds the
    structure's offset."""
    lines = _child(child)
    world = ecr.world_of(child)
    for case in ecr.cases(child):
        ln = lines[ecr.case_name(case)]
        assert (ln['child'], ln['world'], ln['ranks'], ln['device']) == \
            (child, world, world, 'gpu')
        assert ln['exact_mismatch'] == 0
        assert ln['max_err_over_bound'] <= 1.0
        if child == ecr.QUEUE_CHILD:
            assert ln['plans'] and set(ln['plans']) <= {'QWAVE', 'QBLOCK'}
        else:
            assert ln['plans'] == ['GRID']
        assert ('digests' in ln) == (case.options == 'x0')
        if case.options == 'x0':
            assert len(ln['digests']) == ecr.REAL_STEPS
            assert len(set(ln['digests'])) == ecr.REAL_STEPS
    if ecr.REFUSAL in lines:
        assert lines[ecr.REFUSAL]['refused'] == 2


@pytest.mark.parametrize('deferred,waited', ecr.DEFER_PAIRS)
def test_deferral_moves_the_wait_point_only(deferred, waited):
    """At world 2 the sum of two ranks does not depend on its order, so the
    gathered result of every step of every real-class allreduce_x0 job has
    the same bytes in the child that defers the C_0 allreduce into the next
    step and in the child started with ARROW_X0_DEFER=0: "same values, same
    order, only the wait point moves" (DESIGN.md). Not asserted at world 3,
    where the backend's reduce order is its own."""
    a, b = _child(deferred), _child(waited)
    names = ecr.x0_names(deferred)
    assert names == ecr.x0_names(waited) and names
    for name in names:
        assert a[name]['digests'] == b[name]['digests'], name
