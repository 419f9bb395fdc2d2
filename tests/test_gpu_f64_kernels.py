"""The float64 SpMM and routing kernels, each scheduler in a process that
really selects it.

The ARROW_* kernel variables are read once per process, so each entry of
spmm_cases_f64.env_table() runs in a fresh child (tests/spmm_f64_driver.py),
one after another. The child asserts the float64 launch plan before every
launch, compares exact-valued cases bit for bit with the float64 reference
(operands that fp32 cannot represent), checks the sentinels around C, and
logs one JSON line per case. This module never initialises the GPU itself.

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
from tests import spmm_cases_f64 as s64
from tests.spmm_f64_driver import route_case_names

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(REPO, 'tests', 'spmm_f64_driver.py')

# expected seconds per child (process start and GPU initialisation, ~130
# small cases; the default child adds the routes and the k=1024 host
# reference). The limit is a few times that.
EXPECTED_S = {'default': 20}
EXPECTED_DEFAULT_S = 10
TIMEOUT_FACTOR = 4

_gpu_stopped = None      # reason; set once, never cleared
_results = {}            # env name -> (returncode, {case name: json line}, stderr tail)


def _run_env(name):
    global _gpu_stopped
    if _gpu_stopped:
        pytest.fail(f"not started: {_gpu_stopped}", pytrace=False)
    if name in _results:
        return _results[name]
    variables, _ = s64.env_table()[name]
    limit = TIMEOUT_FACTOR * EXPECTED_S.get(name, EXPECTED_DEFAULT_S)
    try:
        p = subprocess.run([sys.executable, DRIVER, name], cwd=REPO,
                           env=sc.child_env(os.environ, variables),
                           capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        _gpu_stopped = f"float64 child '{name}' hit its {limit}s limit"
        pytest.fail(_gpu_stopped, pytrace=False)
    lines = {}
    for raw in p.stdout.splitlines():
        if raw.startswith('{'):
            line = json.loads(raw)
            lines[line['case']] = line
    if p.returncode < 0 or p.returncode in (134, 139, 124, 137):
        _gpu_stopped = (f"float64 child '{name}' ended with status "
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
    _assert_cases_ok('default', route_case_names())


def test_handle_of_the_other_precision_is_refused():
    """A float32 handle at arrow_spmm_f64 / arrow_spmm_dual_f64 and a
    float64 handle at arrow_spmm / arrow_spmm_dual: negative code, a message
    naming both, C untouched; arrow_csr_dtype reports 32 and 64."""
    _assert_cases_ok('default', ['handle_misuse'])
