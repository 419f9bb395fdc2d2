"""Every SpMM kernel variant, each in a process that really selects it.

The ARROW_* kernel variables are read once per process, so each entry of
spmm_cases.env_table() runs in a fresh child (tests/spmm_driver.py f32), one
after another. The child asserts the launch plan before every launch,
compares exact-valued cases bit for bit with the float64 reference, checks
the sentinels around C, and logs one JSON line per case. This module never
initialises the GPU itself.

If a child ends with a signal, an abort/segfault/timeout status or at its
time limit, nothing further is started on the GPU: every remaining test
that needs a child fails at once (tests/gpu_children.py).
"""
import functools

import pytest

from tests import gpu_children
from tests import spmm_cases as sc
from tests.spmm_driver import PRECISIONS, route_case_names

pytestmark = pytest.mark.gpu

# expected seconds per child: measured 2-4 s each on an MI355X with warm
# file caches (a few hundred ms of cases; process start and GPU
# initialisation are the rest), allowing for a cold first start. The limit
# is a few times that.
EXPECTED_S = {'default': 15}
EXPECTED_DEFAULT_S = 10
TIMEOUT_FACTOR = 4

_assert_cases_ok = functools.partial(
    gpu_children.assert_cases_ok, 'f32', sc.env_table(),
    lambda name: TIMEOUT_FACTOR * EXPECTED_S.get(name, EXPECTED_DEFAULT_S))


@pytest.mark.parametrize('name', list(sc.env_table()))
def test_variant_env(name):
    """All cases of one environment ran, with the plan of the table."""
    _, cases = sc.env_table()[name]
    lines = _assert_cases_ok(name, [c['name'] for c in cases])
    for c in cases:
        assert lines[c['name']]['plan'] == c['plan'], c['name']
        assert lines[c['name']]['sentinels'] == 'intact'


def test_route_and_permute_kernels():
    """gather / scatter / scatter-add / permute / permute-add, bit for bit
    against numpy fancy indexing, including a size past the grid cap."""
    _assert_cases_ok('default', route_case_names(PRECISIONS['f32']))


def _legacy(env, prefix, sched, vec, group, betas):
    names = [f'{prefix}{mid}_b{b}' for b in betas for mid in ('', '_exact')]
    lines = _assert_cases_ok(env, names)
    for n in names:
        plan = lines[n]['plan']
        assert (plan['scheduler'], plan['vec'], plan['group']) == \
            (sched, vec, group), (n, plan)


@pytest.mark.parametrize("k", [32, 128])
def test_spmm_queue_wave_grabs(k):
    """Per-WAVE queue grabs at GROUP >= 8 (spmm_kernel_qw, ARROW_QWAVE=1):
    the matrices, k and betas of the former test_gpu_kernels test, launched
    in a process where the variable is live."""
    _legacy('qwave1', f'spmm_queue_wave_grabs_k{k}', sc.QWAVE, 4,
            sc.VEC_GROUP[k][1], (0, 1))


def test_spmm_queue_wave_grabs_hub():
    """Wave grabs with split (atomic) hub rows and empty rows."""
    _legacy('qwave1', 'spmm_queue_wave_grabs_hub', sc.QWAVE, 4, 4, (0,))


def test_spmm_k16_g8_layout():
    """ARROW_K16_G8=1: float2 x 8-lane groups really launched at k=16."""
    _legacy('k16g8', 'spmm_k16_g8_layout', sc.QBLOCK, 2, 8, (0, 1))
