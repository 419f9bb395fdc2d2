"""spmm_arrow --tol (cpu device, synthetic data): the damped loop stops on the
relative step, deterministically: a huge tolerance stops after one step, a
zero tolerance never does, whatever the matrix."""
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(REPO, 'scripts', 'spmm_arrow_main.py')
BASE = ['--width', '20', '--features', '4', '--device', 'cpu',
        '--ranksperside', '3', '--ba_neighbors', '4', '-z', '5']


def _run(*extra):
    with tempfile.TemporaryDirectory() as td:
        return subprocess.run([sys.executable, MAIN] + BASE + list(extra),
                              cwd=td, capture_output=True, text=True,
                              timeout=120)


def test_huge_tol_stops_after_one_step():
    r = _run('--damping', '0.5', '--tol', '1e30')
    assert r.returncode == 0, r.stderr + r.stdout
    assert 'Iteration 0' in r.stdout and 'Iteration 1' not in r.stdout
    assert 'STEPS 1 REL' in r.stdout
    assert 'FAILED' not in r.stdout


def test_zero_tol_runs_every_iteration():
    r = _run('--damping', '0.5', '--tol', '0')
    assert r.returncode == 0, r.stderr + r.stdout
    assert 'Iteration 4' in r.stdout
    assert 'STEPS 5 REL' in r.stdout


def test_tol_is_opt_in_and_needs_damping():
    r = _run('--damping', '0.5')
    assert r.returncode == 0, r.stderr + r.stdout
    assert 'Iteration 4' in r.stdout and 'STEPS' not in r.stdout
    assert "'tol'" not in r.stdout
    r = _run('--tol', '1e-3')
    assert r.returncode != 0
    assert '--tol needs --damping' in r.stderr
