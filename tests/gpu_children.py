"""Starts the child processes of the GPU tests, and decides when to start
no more of them.

The ARROW_* variables are read once per process, so a kernel variant or an
engine path can only be selected by the environment a process STARTS with:
the GPU test modules run the kernel and engine drivers as children, one
after another, through run_child; child_ok adds the verdict every module
wants. The children's side is tests/child_harness.py.

One latch for the whole pytest process: after any child ends with a signal,
a status in FATAL_STATUS, EXIT_ERRORED (a job raised something that is not a
failed comparison, such as a library or HIP error) or at its time limit,
every later caller fails at once with "not started: ...", whichever test
module it is in. A child that exits 1 after a failed case does not latch: the
card is as it was. The in-process GPU tests of the engine modules consult the
same latch (need_gpu). This is a plain module, not a test file and not a
plugin.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests.child_harness import EXIT_ERRORED, REPO
from tests.spmm_cases import KERNEL_VARS

SPMM_DRIVER = os.path.join(REPO, 'tests', 'spmm_driver.py')

# abort, segmentation fault, `timeout`'s own status, SIGKILL
FATAL_STATUS = (134, 139, 124, 137)

# read when the engine builds its structures; a child starts with exactly
# its mode's set (asserted at the top of each engine driver's main)
ENGINE_VARS = ('ARROW_FUSE_ALL', 'ARROW_FOLD', 'ARROW_SPLIT_COL',
               'ARROW_PAR_ROW0', 'ARROW_ROW0_CHUNKS', 'ARROW_REST_CHUNK_NNZ')

_stopped = None          # reason; set once, never cleared
_results = {}            # child_ok's key -> run_child's result


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
    if p.returncode == EXIT_ERRORED:
        bad = [ln for ln in lines.values() if ln.get('errored')] \
            or [{'case': '?', 'error': 'no errored line'}]
        _stop(f"{label}: case '{bad[0]['case']}' errored: "
              f"{bad[0]['error']}", "\n" + p.stderr[-2000:])
    return p.returncode, lines, p.stderr[-2000:]


def child_ok(key, argv, variables, strip_vars, limit_s, label, expected):
    """The child `python argv...` (started as in run_child, once per pytest
    process and `key`) printed no bad line, exited 0 and ran every case of
    `expected`. Returns its JSON lines."""
    fail_if_stopped()
    if key not in _results:
        _results[key] = run_child(argv, variables, strip_vars, limit_s, label)
    rc, lines, stderr = _results[key]
    bad = [ln for ln in lines.values() if not ln['ok']]
    assert not bad, f"{label}: {bad[0]}\n{stderr}"
    assert rc == 0, f"{label}: driver exit status {rc}\n{stderr}"
    missing = [c for c in expected if c not in lines]
    assert not missing, f"{label}: cases not run: {missing[:5]}"
    return lines


def assert_cases_ok(precision, table, limit_s, name, case_names):
    """The spmm_driver child of case set `name` of `table` (an env_table())
    ran every one of case_names, all ok. limit_s maps the name to the child's
    time limit. Returns its JSON lines."""
    return child_ok((SPMM_DRIVER, precision, name),
                    [SPMM_DRIVER, precision, name], table[name][0],
                    KERNEL_VARS, limit_s(name),
                    f"{precision} kernel child '{name}'", case_names)


def need_gpu(clean=ENGINE_VARS):
    """Every in-process GPU test starts here: skipped without a GPU; after a
    child of any test module has aborted, faulted, errored or hit its limit,
    no later test starts GPU work, in-process or not; and none of `clean` is
    set in this process."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    fail_if_stopped()
    for var in clean:
        assert var not in os.environ, var
