"""spmm_arrow --normalize (cpu device, synthetic data): PageRank's loop
converges on the column-normalised operator and does not on the raw one
(16 neighbours of weight in [-1, 1] per vertex: the raw damped step diverges)."""
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(REPO, 'scripts', 'spmm_arrow_main.py')
BASE = ['--width', '20', '--features', '4', '--device', 'cpu',
        '--ranksperside', '3', '--ba_neighbors', '16', '-z', '60',
        '--damping', '0.85', '--tol', '1e-4']


def _run(*extra):
    with tempfile.TemporaryDirectory() as td:
        return subprocess.run([sys.executable, MAIN] + BASE + list(extra),
                              cwd=td, capture_output=True, text=True,
                              timeout=120)


def _steps_rel(stdout):
    m = re.search(r'STEPS (\d+) REL (\S+) TOL', stdout)
    assert m, stdout
    return int(m.group(1)), float(m.group(2))


def test_normalize_col_converges_and_raw_does_not():
    r = _run('--normalize', 'col', '--normalize-abs')
    assert r.returncode == 0, r.stderr + r.stdout
    assert 'FAILED' not in r.stdout and "'normalize': 'col'" in r.stdout
    steps, rel = _steps_rel(r.stdout)
    assert steps < 60 and rel <= 1e-4
    r = _run()
    assert r.returncode == 0, r.stderr + r.stdout
    assert "'normalize'" not in r.stdout
    steps, rel = _steps_rel(r.stdout)
    assert steps == 60 and not rel <= 1e-4


def test_normalize_flags_are_checked():
    r = _run('--normalize-abs')
    assert r.returncode != 0 and '--normalize-abs needs --normalize' in r.stderr
    r = _run('--normalize', 'diag')
    assert r.returncode != 0 and 'invalid choice' in r.stderr
