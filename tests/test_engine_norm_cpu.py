"""Step norms and iterate() on the cpu device: the float64 numpy statement of
the definition, checked against numpy on the step's own input and output."""
import os
import tempfile

import numpy as np
import pytest

from arrow_matrix_amd import graphio, synth
from arrow_matrix_amd.arrow_dec import ArrowDecompositionMPI
from arrow_matrix_amd.backends import CpuBackend


def _build(n_blocks, width=16, k=4, seed=3, dtype=np.float32, scale=None):
    decomp = synth.synth_arrow_decomposition(width, n_blocks, avg_deg=5,
                                             seed=seed, dtype=np.float32)
    if scale is not None:
        A = synth.recompose([(B.astype(np.float64), p) for B, p in decomp])
        s = np.float32(scale / abs(A).sum(axis=1).max())
        decomp = [((B * s).astype(np.float32), p) for B, p in decomp]
    with tempfile.TemporaryDirectory() as td:
        prefix = os.path.join(td, 'g')
        graphio.save_decomposition_new(decomp, prefix, width)
        blocks, nb, tp, tn = ArrowDecompositionMPI.load_decomposition_new(
            None, prefix, width, datatype=dtype)
        arrow = ArrowDecompositionMPI.initialize(None, nb, tp, tn, width, k,
                                                 device='cpu', dtype=dtype)
        arrow.load_data_from_blocks(blocks)
        arrow.zero_rhs(width, k, dtype=dtype)
    rng = np.random.default_rng(seed)
    X = (2 * rng.random((n_blocks[0] * width, k)) - 1).astype(dtype)
    return arrow, X


def test_cpu_backend_diffnorm_is_the_definition():
    import torch
    be = CpuBackend(np.float32)
    rng = np.random.default_rng(0)
    C = rng.standard_normal((7, 5)).astype(np.float32)
    D = rng.standard_normal((7, 5)).astype(np.float32)
    acc = be.norm_acc()
    assert acc.dtype == torch.float64 and acc.tolist() == [0.0, 0.0]
    be.diffnorm_rows(torch.from_numpy(C), torch.from_numpy(D), acc)
    c, d = C.astype(np.float64), D.astype(np.float64)
    assert acc.tolist() == [float(np.square(c - d).sum()),
                            float(np.square(c).sum())]
    be.diffnorm_rows(torch.from_numpy(C), None, acc)      # adds; D None is 0
    assert acc[1].item() == 2 * float(np.square(c).sum())
    assert acc[0].item() == float(np.square(c - d).sum()) + \
        float(np.square(c).sum())


@pytest.mark.parametrize('n_blocks', [[3], [4, 2]])
@pytest.mark.parametrize('affine', [False, True])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_last_step_norms_equal_numpy(n_blocks, affine, dtype):
    arrow, X = _build(n_blocks, dtype=dtype)
    arrow.B.set_features(X.copy())
    if affine:
        arrow.set_affine_step(0.85, 0.15, X.copy())
    with pytest.raises(RuntimeError, match='track_step_norms'):
        arrow.last_step_norms()
    arrow.track_step_norms()
    for _ in range(2):
        x = arrow.B.feature_tile().numpy().astype(np.float64).copy()
        arrow.step()
        c = arrow.B.result_tile().numpy().astype(np.float64)
        d, n = arrow.last_step_norms()
        assert d == float(np.sqrt(np.square(c - x).sum()))
        assert n == float(np.sqrt(np.square(c).sum()))
        assert d > 0 and n > 0
        arrow.B.set_features(arrow.B.result_tile())
    arrow.track_step_norms(False)
    with pytest.raises(RuntimeError, match='track_step_norms'):
        arrow.last_step_norms()


def _contraction(n_blocks=(3,)):
    arrow, X = _build(list(n_blocks), scale=0.999)
    arrow.B.set_features(X.copy())
    arrow.set_affine_step(0.5, 0.5, X.copy())
    return arrow


@pytest.mark.parametrize('n_blocks', [(3,), (4, 2)])
def test_iterate_stops_at_the_first_check_or_never(n_blocks):
    steps, rel = _contraction(n_blocks).iterate(5, tol=1e30)
    assert steps == 1 and 0 < rel < 1e30
    steps, rel0 = _contraction(n_blocks).iterate(5, tol=0.0)
    assert steps == 5 and rel0 > 0
    steps, rel_none = _contraction(n_blocks).iterate(5)
    assert steps == 5 and rel_none == rel0


def test_iterate_honours_check_every():
    steps, _ = _contraction().iterate(7, tol=1e30, check_every=3)
    assert steps == 3
    # never a multiple of check_every below max_steps: read after the last
    steps, rel = _contraction().iterate(5, tol=1e30, check_every=8)
    assert steps == 5 and rel == rel
    # the contraction: stops where a step-by-step loop first meets tol
    a = _contraction()
    a.track_step_norms()
    want = None
    for t in range(1, 40):
        a.step()
        a.B.set_features(a.B.result_tile())
        d, n = a.last_step_norms()
        if d / n <= 1e-3:
            want = t
            break
    assert want is not None and want > 1
    assert _contraction().iterate(40, tol=1e-3)[0] == want
    got = _contraction().iterate(40, tol=1e-3, check_every=4)[0]
    assert got == -(-want // 4) * 4
    with pytest.raises(ValueError):
        _contraction().iterate(0)


class _World2:
    size, rank = 2, 0


def test_world_above_one_is_refused():
    arrow = _contraction()
    arrow.comm = _World2()
    with pytest.raises(NotImplementedError):
        arrow.iterate(3, tol=1e-3)
    with pytest.raises(NotImplementedError):
        arrow.track_step_norms()
    eng = arrow.engines[0]
    eng.comm = _World2()
    with pytest.raises(NotImplementedError):
        eng.track_step_norms()
