"""The bfloat16-feature SpMM and routing kernels, each scheduler in a process
that really selects it.

The ARROW_* kernel variables are read once per process, so each entry of
spmm_cases_bf16.env_table() runs in a fresh child (tests/spmm_bf16_driver.py),
one after another. The child asserts the bf16 launch plan before every
launch, compares exact-valued cases bit for bit with bf16_RNE of the float64
reference (split rows of 2049 and 4097 nonzeros included), holds real-valued
cases to the derived bound, checks the sentinels around C, and logs one JSON
line per case. This module never initialises the GPU itself.

If a child ends with a signal, an abort/segfault/timeout status or at its
time limit, nothing further is started on the GPU: every remaining test of
this module fails at once.
"""
import json
import os
import subprocess
import sys

import pytest

from tests import spmm_cases as sc
from tests import spmm_cases_bf16 as s16
from tests.spmm_bf16_driver import route_case_names

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(REPO, 'tests', 'spmm_bf16_driver.py')

# expected seconds per child (process start and GPU initialisation, a few
# dozen small cases; the default child adds the routes, whose largest shape
# is 33000 x 1024). The limit is a few times that.
EXPECTED_S = {'default': 30}
EXPECTED_DEFAULT_S = 12
TIMEOUT_FACTOR = 4

_gpu_stopped = None      # reason; set once, never cleared
_results = {}            # env name -> (returncode, {case name: json line}, stderr tail)


def _run_env(name):
    global _gpu_stopped
    if _gpu_stopped:
        pytest.fail(f"not started: {_gpu_stopped}", pytrace=False)
    if name in _results:
        return _results[name]
    variables, _ = s16.env_table()[name]
    limit = TIMEOUT_FACTOR * EXPECTED_S.get(name, EXPECTED_DEFAULT_S)
    try:
        p = subprocess.run([sys.executable, DRIVER, name], cwd=REPO,
                           env=sc.child_env(os.environ, variables),
                           capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        _gpu_stopped = f"bfloat16 child '{name}' hit its {limit}s limit"
        pytest.fail(_gpu_stopped, pytrace=False)
    lines = {}
    for raw in p.stdout.splitlines():
        if raw.startswith('{'):
            line = json.loads(raw)
            lines[line['case']] = line
    if p.returncode < 0 or p.returncode in (134, 139, 124, 137):
        _gpu_stopped = (f"bfloat16 child '{name}' ended with status "
                        f"{p.returncode} after {len(lines)} cases")
        pytest.fail(_gpu_stopped + "\n" + p.stderr[-2000:], pytrace=False)
    _results[name] = (p.returncode, lines, p.stderr[-2000:])
    return _results[name]


def _assert_cases_ok(name, case_names):
    rc, lines, stderr = _run_env(name)
    bad = [ln for ln in lines.values() if not ln['ok']]
    assert not bad, f"{name}: {bad[0]}"
    assert rc == 0, f"{name}: driver exit status {rc}\n{stderr}"
    missing = [c for c in case_names if c not in lines]
    assert not missing, f"{name}: cases not run: {missing[:5]}"
    return lines


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
    _assert_cases_ok('default', route_case_names())


def test_bf16_misuse_is_refused():
    """A float64 handle at the bf16 entry points, and k = 12: negative code,
    a message naming the reason, C and its sentinels untouched."""
    _assert_cases_ok('default', ['misuse'])
