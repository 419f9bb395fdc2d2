"""The affine step X <- alpha * A@X + gamma * R through the engine on one GPU,
in float32, float64 and bfloat16 features: three steps, each checked against
the float64 evaluation of the engine's own previous output on the recomposed
matrix, to the derived bound of tests/engine_affine_driver.py. The default
single-launch layout runs in-process; the layouts an environment variable
selects (two-launch, L = 2 sequential, full fold, row fold, banded ArrowMPI)
each run in a child process that starts with it.
"""
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import engine_affine_driver as drv
from tests import gpu_children
from tests.spmm_cases import SEG_NNZ

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(gpu_children.REPO, 'tests', 'engine_affine_driver.py')
CHILD_LIMIT_S = 150      # process start + GPU initialisation + 3 x 3 tiny steps


@pytest.mark.parametrize('precision', drv.PRECISIONS)
@pytest.mark.parametrize('shape', ['L1', 'HUB'])
def test_default_layout_is_fused_and_within_bound(shape, precision):
    """The single-launch layout carries the step in its write-back: within
    the bound and the tail kernel is never called. HUB has split rows."""
    gpu_children.need_gpu()
    kwargs = getattr(drv, shape)
    arrow, tails, figures = drv.run(precision, **kwargs)
    eng0 = arrow.engines[0]
    assert eng0._A_all is not None
    if shape == 'HUB':
        from arrow_matrix_amd import synth
        B0 = synth.synth_arrow_decomposition(
            kwargs['width'], kwargs['n_blocks'], avg_deg=6,
            seed=kwargs['seed'], hub_rows=2, hub_deg=8000)[0][0]
        assert np.diff(B0.indptr).max() > SEG_NNZ
    assert tails == 0
    assert len(figures) == 3
    assert eng0._R is not eng0.C_i and eng0._R is not eng0.X_i
    assert eng0._R.dtype == eng0.C_i.dtype


@pytest.mark.parametrize('mode', list(drv.MODES))
def test_environment_selected_layouts(mode):
    """Each layout in a child that starts with its environment; both folds
    are fused (no tail call), the others run the tail kernel once a step."""
    gpu_children.need_gpu()
    variables, _, inside = drv.MODES[mode]
    lines = gpu_children.child_ok(
        (DRIVER, mode), [DRIVER, mode], variables, gpu_children.ENGINE_VARS,
        CHILD_LIMIT_S, f"affine engine child '{mode}'", drv.PRECISIONS)
    assert set(lines) == set(drv.PRECISIONS)
    for ln in lines.values():
        assert ln['tails'] == (0 if inside else 3)


@pytest.mark.parametrize('precision', drv.PRECISIONS)
def test_split_col_launches_carry_the_step(monkeypatch, precision):
    """ARROW_SPLIT_COL=1 writes a row below block row 0 twice (rest launch,
    hub-sorted beta = 1 launch): those launches carry the step, and the tail
    runs on block row 0 alone, so no element is stored more than twice (the
    bound counts two roundings of bf16 features). The layout variables are
    read when the structures are built, so this runs in-process,
    grid-stride."""
    gpu_children.need_gpu()
    from arrow_matrix_amd.backends import GpuBackend
    monkeypatch.setenv('ARROW_FUSE_ALL', '0')
    monkeypatch.setenv('ARROW_SPLIT_COL', '1')
    tail_rows = []
    inner = GpuBackend.axpby_rows

    def recorded(self, C, *args, **kwargs):
        tail_rows.append(C.shape[0])
        return inner(self, C, *args, **kwargs)
    monkeypatch.setattr(GpuBackend, 'axpby_rows', recorded)
    shape = dict(drv.L1, hub_rows=2)
    arrow, tails, figures = drv.run(precision, **shape)
    eng0 = arrow.engines[0]
    assert eng0._A_all is None and eng0._A_col is not None and eng0._A_rest
    assert len(figures) == 3
    assert tails == 3 and tail_rows == [shape['width']] * 3


@pytest.mark.parametrize('shape,precision', [('L1', 'float32'),
                                             ('HUB', 'bfloat16')])
def test_captured_step_equals_the_uncaptured_step(shape, precision):
    """set_affine_step allocates; step() does not: after one warm-up step a
    step captured under torch.cuda.graph replays to the bits of the same
    step run directly."""
    gpu_children.need_gpu()
    arrow, A, perm0, X, R = drv.build(precision=precision,
                                      **getattr(drv, shape))
    arrow.B.set_features(X[perm0].copy())
    arrow.set_affine_step(drv.ALPHA, drv.GAMMA, R[perm0].copy())
    arrow.step()                                     # warm-up
    arrow.step()          # features unchanged: the same step, same buffers
    torch.cuda.synchronize()
    C = arrow.B.result_tile()
    direct = C.clone()
    C.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        arrow.step()
    g.replay()
    torch.cuda.synchronize()
    assert arrow.B.result_tile() is C
    assert torch.equal(C.view(torch.uint8), direct.view(torch.uint8))
    assert float(direct.float().abs().max()) > 0


@pytest.mark.parametrize('precision', drv.PRECISIONS)
def test_clear_affine_step_restores_the_plain_step(precision):
    gpu_children.need_gpu()
    a, A, perm0, X, R = drv.build(precision=precision, **drv.L1)
    b, *_ = drv.build(precision=precision, **drv.L1)
    a.B.set_features(X[perm0].copy())
    a.set_affine_step(drv.ALPHA, drv.GAMMA, R[perm0].copy())
    a.step()
    a.clear_affine_step()
    assert a.engines[0]._R is None
    tails = drv.TailCounter(a.engines[0].backend)
    a.B.set_features(X[perm0].copy())
    a.step()
    b.B.set_features(X[perm0].copy())
    b.step()
    assert tails.calls == 0
    assert torch.equal(a.B.result_tile().view(torch.uint8),
                       b.B.result_tile().view(torch.uint8))


def test_refusals_on_the_gpu_engine():
    gpu_children.need_gpu()
    from arrow_matrix_amd.arrow_slim import ArrowSlimMPI
    e = ArrowSlimMPI(None, tiles_per_side=2, device='gpu')
    e.zero_rhs(8, 8)
    with pytest.raises(ValueError, match='residual'):
        e.set_affine_step(0.85, 0.15)
    with pytest.raises(ValueError, match='shape'):
        e.set_affine_step(0.85, 0.15, np.zeros((16, 4), dtype=np.float32))
    with pytest.raises(TypeError, match='dtype'):
        e.set_affine_step(0.85, 0.15, torch.zeros((16, 8),
                                                  dtype=torch.float64))
    e.set_affine_step(0.85, 0.15, np.ones((16, 8), dtype=np.float32))
    assert e._R.is_cuda and e._R.dtype == torch.float32
    h = ArrowSlimMPI(None, tiles_per_side=2, device='gpu', dtype='bfloat16')
    h.zero_rhs(8, 8, dtype='bfloat16')
    h.set_affine_step(0.85, 0.15, np.full((16, 8), 257.0, dtype=np.float32))
    assert h._R.dtype == torch.bfloat16
    assert float(h._R.float().max()) == 256.0        # rounded once


def test_bench_spmm_gpu_damping():
    gpu_children.need_gpu()
    from arrow_matrix_amd.arrow_bench import bench_spmm
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as td:
        try:
            os.chdir(td)
            arrow = bench_spmm(None, 64, 8, 3, True, 'gpu', damping=0.85)
            assert arrow is not None
            assert arrow._affine[:2] == (0.85, 1 - 0.85)
            C = arrow.B.allgather_result()
            assert np.isfinite(C).all() and np.abs(C).max() > 0
        finally:
            os.chdir(cwd)
