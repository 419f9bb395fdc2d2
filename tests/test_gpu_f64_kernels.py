"""The float64 SpMM and routing kernels, each scheduler in a process that
really selects it.

The ARROW_* kernel variables are read once per process, so each entry of
spmm_cases_f64.env_table() runs in a fresh child (tests/spmm_driver.py f64),
one after another. The child asserts the float64 launch plan before every
launch, compares exact-valued cases bit for bit with the float64 reference
(operands that fp32 cannot represent), checks the sentinels around C, and
logs one JSON line per case. This module never initialises the GPU itself.

If a child ends with a signal, an abort/segfault/timeout status or at its
time limit, nothing further is started on the GPU: every remaining test
that needs a child fails at once (tests/gpu_children.py).
"""
import functools

import pytest

from tests import gpu_children
from tests import spmm_cases_f64 as s64
from tests.spmm_driver import PRECISIONS, route_case_names

pytestmark = pytest.mark.gpu

# expected seconds per child (process start and GPU initialisation, ~130
# small cases; the default child adds the routes and the k=1024 host
# reference). The limit is a few times that.
EXPECTED_S = {'default': 20}
EXPECTED_DEFAULT_S = 10
TIMEOUT_FACTOR = 4

_assert_cases_ok = functools.partial(
    gpu_children.assert_cases_ok, 'f64', s64.env_table(),
    lambda name: TIMEOUT_FACTOR * EXPECTED_S.get(name, EXPECTED_DEFAULT_S))


@pytest.mark.parametrize('name', list(s64.env_table()))
def test_f64_env(name):
    """All cases of one environment ran, with the plan of the table."""
    _, cases = s64.env_table()[name]
    lines = _assert_cases_ok(name, [c['name'] for c in cases])
    for c in cases:
        assert lines[c['name']]['plan'] == c['plan'], c['name']
        assert lines[c['name']]['sentinels'] == 'intact'


def test_f64_route_and_permute_kernels():
    """gather / scatter / scatter-add / permute / permute-add in float64,
    bit for bit against numpy fancy indexing, including a size past the
    grid cap."""
    _assert_cases_ok('default', route_case_names(PRECISIONS['f64']))


def test_handle_of_the_other_precision_is_refused():
    """A float32 handle at arrow_spmm_f64 / arrow_spmm_dual_f64 and a
    float64 handle at arrow_spmm / arrow_spmm_dual: negative code, a message
    naming both, C untouched; arrow_csr_dtype reports 32 and 64."""
    _assert_cases_ok('default', ['handle_misuse'])
