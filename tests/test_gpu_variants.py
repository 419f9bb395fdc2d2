"""Every SpMM kernel variant, each in a process that really selects it.

The ARROW_* kernel variables are read once per process, so each entry of
spmm_cases.env_table() runs in a fresh child (tests/spmm_variant_driver.py),
one after another. The child asserts the launch plan before every launch,
compares exact-valued cases bit for bit with the float64 reference, checks
the sentinels around C, and logs one JSON line per case. This module never
initialises the GPU itself.

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
from tests.spmm_variant_driver import route_case_names

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(REPO, 'tests', 'spmm_variant_driver.py')

# expected seconds per child: measured 2-4 s each on an MI355X with warm
# file caches (a few hundred ms of cases; process start and GPU
# initialisation are the rest), allowing for a cold first start. The limit
# is a few times that.
EXPECTED_S = {'default': 15}
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
    variables, _ = sc.env_table()[name]
    limit = TIMEOUT_FACTOR * EXPECTED_S.get(name, EXPECTED_DEFAULT_S)
    try:
        p = subprocess.run([sys.executable, DRIVER, name], cwd=REPO,
                           env=sc.child_env(os.environ, variables),
                           capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        _gpu_stopped = f"variant child '{name}' hit its {limit}s limit"
        pytest.fail(_gpu_stopped, pytrace=False)
    lines = {}
    for raw in p.stdout.splitlines():
        if raw.startswith('{'):
            line = json.loads(raw)
            lines[line['case']] = line
    if p.returncode < 0 or p.returncode in (134, 139, 124, 137):
        _gpu_stopped = (f"variant child '{name}' ended with status "
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
    _assert_cases_ok('default', route_case_names())


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
