"""The bfloat16-feature SpMM and routing kernels, each scheduler in a process
that really selects it.

The ARROW_* kernel variables are read once per process, so each entry of
spmm_cases_bf16.env_table() runs in a fresh child (tests/spmm_driver.py
bf16), one after another. The child asserts the bf16 launch plan before every
launch, compares exact-valued cases bit for bit with bf16_RNE of the float64
reference (split rows of 2049 and 4097 nonzeros included), holds real-valued
cases to the derived bound, checks the sentinels around C, and logs one JSON
line per case. This module never initialises the GPU itself.

If a child ends with a signal, an abort/segfault/timeout status or at its
time limit, nothing further is started on the GPU: every remaining test
that needs a child fails at once (tests/gpu_children.py).
"""
import functools

import pytest

from tests import gpu_children
from tests import spmm_cases_bf16 as s16
from tests.spmm_driver import PRECISIONS, route_case_names

pytestmark = pytest.mark.gpu

# expected seconds per child (process start and GPU initialisation, a few
# dozen small cases; the default child adds the routes, whose largest shape
# is 33000 x 1024). The limit is a few times that.
EXPECTED_S = {'default': 30}
EXPECTED_DEFAULT_S = 12
TIMEOUT_FACTOR = 4

_assert_cases_ok = functools.partial(
    gpu_children.assert_cases_ok, 'bf16', s16.env_table(),
    lambda name: TIMEOUT_FACTOR * EXPECTED_S.get(name, EXPECTED_DEFAULT_S))


@pytest.mark.parametrize('name', list(s16.env_table()))
def test_bf16_env(name):
    """All cases of one environment ran, with the plan of the table."""
    _, cases = s16.env_table()[name]
    lines = _assert_cases_ok(name, [c['name'] for c in cases])
    for c in cases:
        assert lines[c['name']]['plan'] == c['plan'], c['name']
        assert lines[c['name']]['sentinels'] == 'intact'


def test_bf16_split_rows_repeat_bit_for_bit():
    """Two launches of the same split-row case give identical bits."""
    _assert_cases_ok('default', ['repeat_k128_b1'])


def test_bf16_route_and_permute_kernels():
    """gather / scatter / permute bit for bit against fancy indexing;
    scatter-add / permute-add equal bf16_RNE(float(dst) + float(src));
    including a size past the grid cap."""
    _assert_cases_ok('default', route_case_names(PRECISIONS['bf16']))


def test_bf16_misuse_is_refused():
    """A float64 handle at the bf16 entry points, and k = 12: negative code,
    a message naming the reason, C and its sentinels untouched."""
    _assert_cases_ok('default', ['misuse'])
