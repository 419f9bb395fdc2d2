"""Starts the child processes of the GPU tests, and decides when to start
no more of them.

The ARROW_* variables are read once per process, so a kernel variant or an
engine path can only be selected by the environment a process STARTS with:
the GPU test modules run tests/spmm_driver.py and the engine drivers as
children, one after another, through run_child.

One latch for the whole pytest process: after any child ends with a signal,
a status in FATAL_STATUS or at its time limit, every later caller fails at
once with "not started: ...", whichever test module it is in. The in-process
GPU tests of the engine modules consult the same latch (fail_if_stopped).
This is a plain module, not a test file and not a plugin.
"""
import json
import os
import subprocess
import sys

import pytest

from tests.spmm_cases import KERNEL_VARS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPMM_DRIVER = os.path.join(REPO, 'tests', 'spmm_driver.py')

# abort, segmentation fault, `timeout`'s own status, SIGKILL
FATAL_STATUS = (134, 139, 124, 137)

# read when the engine builds its structures; a child starts with exactly
# its mode's set (asserted at the top of each engine driver's main)
ENGINE_VARS = ('ARROW_FUSE_ALL', 'ARROW_FOLD', 'ARROW_SPLIT_COL',
               'ARROW_PAR_ROW0', 'ARROW_ROW0_CHUNKS', 'ARROW_REST_CHUNK_NNZ')

_stopped = None          # reason; set once, never cleared
_results = {}            # (precision, env name) -> run_child's result


def fail_if_stopped():
    if _stopped:
        pytest.fail(f"not started: {_stopped}", pytrace=False)


def _stop(reason, detail=''):
    global _stopped
    _stopped = reason
    pytest.fail(reason + detail, pytrace=False)


def json_lines(stdout):
    """{case name: line} of the JSON lines a driver printed."""
    lines = {}
    for raw in stdout.splitlines():
        if raw.startswith('{'):
            line = json.loads(raw)
            lines[line['case']] = line
    return lines


def run_child(argv, variables, strip_vars, limit_s, label):
    """`python argv...` with the parent's environment less strip_vars, plus
    `variables`. Returns (returncode, {case name: json line}, stderr tail)."""
    fail_if_stopped()
    env = {k: v for k, v in os.environ.items() if k not in strip_vars}
    env.update(variables)
    try:
        p = subprocess.run([sys.executable] + list(argv), cwd=REPO, env=env,
                           capture_output=True, text=True, timeout=limit_s)
    except subprocess.TimeoutExpired:
        _stop(f"{label} hit its {limit_s}s limit")
    lines = json_lines(p.stdout)
    if p.returncode < 0 or p.returncode in FATAL_STATUS:
        _stop(f"{label} ended with status {p.returncode} after "
              f"{len(lines)} cases", "\n" + p.stderr[-2000:])
    return p.returncode, lines, p.stderr[-2000:]


def assert_cases_ok(precision, table, limit_s, name, case_names):
    """The child of case set `name` of `table` (an env_table()) ran every one
    of case_names, all ok; it is started once per pytest process. limit_s
    maps the name to the child's time limit. Returns its JSON lines."""
    fail_if_stopped()
    if (precision, name) not in _results:
        _results[precision, name] = run_child(
            [SPMM_DRIVER, precision, name], table[name][0], KERNEL_VARS,
            limit_s(name), f"{precision} kernel child '{name}'")
    rc, lines, stderr = _results[precision, name]
    bad = [ln for ln in lines.values() if not ln['ok']]
    assert not bad, f"{name}: {bad[0]}"
    assert rc == 0, f"{name}: driver exit status {rc}\n{stderr}"
    missing = [c for c in case_names if c not in lines]
    assert not missing, f"{name}: cases not run: {missing[:5]}"
    return lines
