"""Operator scaling on the cpu-backend engine: operator_sums, scale_operator
and normalize_operator against scipy on the recomposed matrix, at L = 1 and
at L = 2 under ARROW_FOLD=0, 1 and 2 (tests/engine_scale_driver.py, one child
process per layout: the variables are read when the structures are built),
and the refusal at world size 2 under gloo."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from tests import engine_scale_driver as esd
from tests.gpu_children import ENGINE_VARS, json_lines

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(REPO, 'tests', 'engine_scale_driver.py')


@pytest.mark.parametrize('mode', ['default', 'fold0', 'fold1', 'fold2'])
def test_cpu_engine_layout(mode):
    env = {k: v for k, v in os.environ.items() if k not in ENGINE_VARS}
    env.update(esd.MODES[mode][0])
    p = subprocess.run([sys.executable, DRIVER, mode, 'cpu'], cwd=REPO,
                       env=env, capture_output=True, text=True, timeout=300)
    lines = json_lines(p.stdout)
    bad = [ln for ln in lines.values() if not ln['ok']]
    assert not bad, bad[0]
    assert p.returncode == 0, p.stderr[-2000:]
    assert sorted(lines) == sorted(esd.PRECISIONS['cpu'])
    for ln in lines.values():
        assert 1 < ln['steps'] < esd.end.ITER_MAX


def test_vectors_are_checked_and_none_is_no_factor():
    kwargs = esd.MODES['default'][1]
    decomp = esd.make_decomp(**kwargs)
    arrow = esd.load(decomp, 'float32', 'cpu', **kwargs)
    before = arrow.operator_sums()
    arrow.scale_operator()
    arrow.scale_operator(None, None)
    after = arrow.operator_sums()
    assert all((a == b).all() for a, b in zip(before, after))
    n = before[0].size
    with pytest.raises(ValueError, match='row_scale'):
        arrow.scale_operator(np.ones(n + 1))
    with pytest.raises(ValueError, match='kind'):
        arrow.normalize_operator('rows')
    # the slim engine has the same three methods, in its own layout
    eng = arrow.engines[0]
    assert all((a == b).all() for a, b in zip(eng.operator_sums(), before))
    eng.scale_operator(col_scale=np.full(n, 2.0))
    assert (arrow.operator_sums()[0] == 2.0 * before[0]).all()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, port, tmpdir, result_q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=2)
    try:
        from arrow_matrix_amd import graphio, synth
        from arrow_matrix_amd.arrow_dec import ArrowDecompositionMPI
        from arrow_matrix_amd.comm import TorchDistComm
        comm = TorchDistComm()
        width, n_blocks, k = 6, [4], 4
        decomp = synth.synth_arrow_decomposition(width, n_blocks, avg_deg=5,
                                                 seed=0)
        prefix = os.path.join(tmpdir, 'g')
        if rank == 0:
            graphio.save_decomposition_new(decomp, prefix, width)
        dist.barrier()
        blocks, nb, tp, tn = ArrowDecompositionMPI.load_decomposition_new(
            comm, prefix, width)
        arrow = ArrowDecompositionMPI.initialize(comm, nb, tp, tn, width, k,
                                                 device='cpu')
        arrow.load_data_from_blocks(blocks)
        refused = 0
        for target in (arrow, arrow.engines[0]):
            for call in (lambda t: t.operator_sums(),
                         lambda t: t.scale_operator(np.ones(24), None),
                         lambda t: t.normalize_operator('row', absolute=True)):
                try:
                    call(target)
                except NotImplementedError as e:
                    assert 'single-process' in str(e)
                    refused += 1
        if rank == 0:
            result_q.put(refused)
    finally:
        dist.destroy_process_group()


def test_world_size_two_is_refused(tmp_path):
    port = _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, port, str(tmp_path), q))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
    for p in procs:
        assert p.exitcode == 0, f"worker failed (exitcode {p.exitcode})"
    assert q.get(timeout=10) == 6
