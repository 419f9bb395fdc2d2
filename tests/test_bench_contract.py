"""bench.py driver-contract tests: the exact launch pattern the round-end
driver uses (torchrun, one rank per device, JSON line on rank 0), run here
with --device cpu over gloo."""
import json
import os
import socket
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, 'bench.py')


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(args, world=None, timeout=240, env=None):
    if world:
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
               f'--nproc-per-node={world}', '--master-addr', '127.0.0.1',
               '--master-port', str(_free_port()), BENCH, '--gpus', str(world)]
    else:
        cmd = [sys.executable, BENCH]
    r = subprocess.run(cmd + args, capture_output=True, text=True,
                       timeout=timeout, cwd=REPO,
                       env=dict(os.environ, **env) if env else None)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-500:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, f"expected ONE JSON line, got {lines}"
    return json.loads(lines[0])


TINY = ['--rows', '4000', '--features', '8', '--n-blocks', '4',
        '--band', '16', '--device', 'cpu', '--no-cpu-baseline',
        '--steps', '2', '--warmup', '1']


def test_single_process_contract():
    d = _run(TINY)
    for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup',
                'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
                'dtype', 'data', 'config'):
        assert key in d, key
    assert d['n_gpus'] == 1 and d['data'] == 'synthetic'
    assert d['config']['workload'].startswith('cfg4_synth')


def test_plain_run_is_lean_and_steps_exact():
    """Without --full the secondary measurements stay off (no
    --no-cpu-baseline needed), and --steps is the timed step count as
    given, odd values included."""
    args = [a for a in TINY if a != '--no-cpu-baseline']
    args[args.index('--steps') + 1] = '3'
    d = _run(args)
    assert d['steps'] == 3 and d['warmup'] == 1
    assert d['ms_per_step'] > 0
    assert d['cpu_baseline'] is None and d['roofline'] is None


@pytest.fixture(scope='module')
def tiny_dump(tmp_path_factory):
    """One TINY cpu run with --dump-outputs, shared by the dump tests."""
    import numpy as np
    d = tmp_path_factory.mktemp('dump')
    _run(TINY + ['--dump-outputs', str(d)])
    assert sorted(os.listdir(d)) == ['C.npy']
    C = np.load(d / 'C.npy')
    C.setflags(write=False)
    return C


def test_dump_outputs_reproducible(tiny_dump, tmp_path):
    """--dump-outputs writes the last step's result stripe as float32
    .npy; the same arguments give the same inputs, hence (on the
    deterministic cpu device) bit-identical outputs."""
    import numpy as np
    _run(TINY + ['--dump-outputs', str(tmp_path)])
    again = np.load(tmp_path / 'C.npy')
    assert tiny_dump.dtype == np.float32 and tiny_dump.shape == (4000, 8)
    assert np.isfinite(tiny_dump).all() and np.abs(tiny_dump).max() > 0
    np.testing.assert_array_equal(tiny_dump, again)


def test_dump_outputs_matches_scipy_iteration(tiny_dump):
    """The dumped stripe is A^(warmup+steps) X0 for the bench's own
    deterministic blocks and seeded X0 (cpu device, float32)."""
    import numpy as np
    import torch
    from scipy import sparse
    import bench
    C = tiny_dump
    nb, w, k, band = 4, 1000, 8, 16
    grids, _, _ = bench.build_blocks_for_rank(0, 1, w, nb, 1, 'cpu', band)
    A = sparse.bmat(grids[0], format='csr')
    g = torch.Generator()
    g.manual_seed(42)
    G = (torch.rand((nb * w, k), generator=g) * 2 - 1).numpy().astype(np.float64)
    for _ in range(3):  # TINY: 1 warmup + 2 steps
        G = A.astype(np.float64) @ G
    # f32 accumulation over <= 3 chained products of ~10-nnz rows: a few
    # ulp per step relative to the result scale
    scale = float(np.abs(G).max())
    assert 1e-3 < scale <= 1.0
    assert np.abs(C - G).max() <= 1e-5 * scale


def test_workload_rows_sum_to_one():
    """The synthetic matrix is positive with unit row sums (hub rows and
    multi-part sums included), so iterating X := A X can neither overflow
    nor die out whatever --steps is."""
    import numpy as np
    from scipy import sparse
    import bench
    w = 4 * bench.HUB_NNZ + 8  # smallest width that gets hub rows
    for nb, parts in ((2, 1), (3, 2)):
        grids, _, _ = bench.build_blocks_for_rank(0, 1, w, nb, parts, 'cpu', 64)
        total = sum(sparse.bmat(g, format='csr') for g in grids)
        assert total.data.min() > 0
        sums = np.asarray(total.sum(axis=1)).ravel()
        # f32 values normalised in f64: <= 50k-term rows, ~1e-7 each
        np.testing.assert_allclose(sums, 1.0, rtol=0, atol=2e-5)


def test_many_steps_stay_finite_and_nontrivial(tmp_path):
    """300 iterations — far past where a growing iterate overflows f32 —
    still dump finite values of the inputs' order of magnitude."""
    import numpy as np
    args = list(TINY)
    args[args.index('--steps') + 1] = '300'
    _run(args + ['--dump-outputs', str(tmp_path)])
    C = np.load(tmp_path / 'C.npy')
    assert np.isfinite(C).all()
    # rows converge to a positive-weight average of X0 (uniform in [-1,1],
    # 4000 rows): bounded by 1, and of order 1/sqrt(4000) or more
    assert np.abs(C).max() <= 1.0
    assert np.abs(C).max() > 1e-4


@pytest.mark.gpu
def test_gpu_graph_odd_steps_match_plain_steps(tmp_path):
    """On the GPU the timed loop replays a captured two-step graph; an odd
    --steps adds one plain step. The result must be what the same number
    of uncaptured steps computes from the same seeded inputs."""
    import numpy as np
    # 40k rows keeps more than one block of work items per launch
    gpu = ['--rows', '40000', '--features', '16', '--n-blocks', '4',
           '--band', '64', '--steps', '3', '--dump-outputs']
    # the untimed first replay after capture is two more steps: 1 warmup
    # + 2 + 3 timed there equals 3 warmup + 3 timed here
    dg = _run(gpu + [str(tmp_path / 'graph'), '--graph', 'on',
                     '--warmup', '1'])
    de = _run(gpu + [str(tmp_path / 'eager'), '--graph', 'off',
                     '--warmup', '3'])
    assert dg['steps'] == de['steps'] == 3
    assert dg['config']['hipgraph'] and not de['config']['hipgraph']
    assert dg['roofline'] is None and dg['cpu_baseline'] is None
    Cg = np.load(tmp_path / 'graph' / 'C.npy')
    Ce = np.load(tmp_path / 'eager' / 'C.npy')
    assert Cg.dtype == np.float32 and Cg.shape == (40000, 16)
    # same kernels on the same inputs; only the order of fp32 atomic adds
    # on split rows may differ: a few ulp of the result scale over 6 steps
    # (<= 16 terms per row, eps 6e-8)
    scale = float(np.abs(Ce).max())
    assert 1e-4 < scale <= 1.0
    assert np.abs(Cg - Ce).max() <= 1e-5 * scale


def test_torchrun_world2_contract(tmp_path):
    import numpy as np
    d = _run(TINY + ['--dump-outputs', str(tmp_path)], world=2)
    assert d['n_gpus'] == 2
    assert d['value'] > 0
    # one file per rank, all of them together within the 64 MB allowed
    assert sorted(os.listdir(tmp_path)) == ['C_rank0.npy', 'C_rank1.npy']
    assert sum(os.path.getsize(tmp_path / f)
               for f in os.listdir(tmp_path)) <= 64_000_000
    for f in os.listdir(tmp_path):
        C = np.load(tmp_path / f)
        assert C.dtype == np.float32 and C.shape == (2000, 8)
        assert np.isfinite(C).all()


def test_dump_budget_is_shared_by_all_ranks(tmp_path):
    """Stripes larger than the budget: the files of one run stay within
    64 MB together at every world size, sampled rows are distinct and the
    same on every call."""
    import numpy as np
    import torch
    import bench

    class _Eng:
        def __init__(self, X):
            self.X = X

        def _flush_x0_pipeline(self):
            pass

        def feature_tile(self):
            return self.X

    k = 16
    n = 3 * bench.DUMP_MAX_BYTES // (4 * k)  # 3x the whole budget per rank
    X = torch.arange(n, dtype=torch.float32).unsqueeze(1).expand(n, k)
    for world in (1, 2, 8):
        d = tmp_path / f'w{world}'
        for rank in range(world):
            bench.dump_outputs(str(d), _Eng(X), rank, world)
        files = sorted(os.listdir(d))
        assert len(files) == world
        assert sum(os.path.getsize(d / f) for f in files) <= 64_000_000
        C = np.load(d / files[0])
        assert C.dtype == np.float32 and C.shape[1] == k
        rows = C[:, 0]  # row r holds the value r (exact in f32: n < 2^24)
        assert n < 2 ** 24 and np.all(np.diff(rows) > 0)
        if world == 1:
            bench.dump_outputs(str(tmp_path / 'again'), _Eng(X), 0, 1)
            np.testing.assert_array_equal(
                C, np.load(tmp_path / 'again' / 'C.npy'))


def test_full_fills_cpu_baseline():
    """--full turns the secondary measurements back on: the CPU baseline
    is measured (briefly here) unless --no-cpu-baseline is given."""
    args = [a for a in TINY if a != '--no-cpu-baseline']
    d = _run(args + ['--full', '--cpu-baseline-seconds', '0.2'])
    cb = d['cpu_baseline']
    assert cb is not None and cb['value'] > 0 and cb['unit'] == 'GFLOP/s'
    assert cb['cores'] >= 1 and cb['kind'] == 'port'
    assert d['steps'] == 2 and d['ms_per_step'] > 0


def test_full_no_cpu_baseline():
    d = _run(TINY + ['--full'])
    assert d['cpu_baseline'] is None


@pytest.mark.gpu
def test_gpu_full_fills_roofline():
    """On the GPU --full runs the HBM-peak and HIP-event roofline passes
    (the rocprofv3 traffic probe is switched off here: it re-runs the
    benchmark twice under the profiler)."""
    d = _run(['--rows', '40000', '--features', '16', '--n-blocks', '4',
              '--band', '64', '--steps', '2', '--warmup', '1', '--full',
              '--no-cpu-baseline'], env={'ARROW_TRAFFIC_PROBE': '0'})
    r = d['roofline']
    assert r is not None and r['bound'] == 'hbm'
    assert r['achieved'] > 0 and r['launches'] > 0
    assert r['peak_measured'] > 0 and r['frac_measured'] > 0
    assert r['traffic'] is None and d['cpu_baseline'] is None


def test_torchrun_world2_multi_part():
    d = _run(TINY + ['--parts', '2'], world=2)
    assert d['config']['parts'] == 2
    assert d['value'] > 0
