"""Which backend launches a step makes, in which order and with which step
arguments, for every layout and step kind: the engines drive a recording
backend that claims device 'cuda' and does the arithmetic in numpy. Runs
without a GPU and without the built library."""
import os
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from scipy import sparse

from arrow_matrix_amd import arrow_slim, graphio, synth
from arrow_matrix_amd.arrow_dec import ArrowDecompositionMPI
from arrow_matrix_amd.backends import CpuBackend

WIDTH, K = 4, 4
ALPHA, GAMMA = 0.85, 0.15


class _RecordingBackend(CpuBackend):
    """CpuBackend storage, the GPU backend's launch surface: every launch
    appends (method, beta, alpha, gamma, R is not None, norm is not None)."""
    device = 'cuda'
    bf16 = False
    feat_dtype = np.dtype(np.float32)
    feat_itemsize = 4

    def __init__(self, dtype=np.float32):
        super().__init__(dtype)
        self.calls = []

    def upload_arrays(self, shape, indptr, indices, data, row_ids=None,
                      col_items=False):
        return SimpleNamespace(
            shape=shape, indptr=np.asarray(indptr), indices=np.asarray(indices),
            data=np.asarray(data), nnz=int(len(indices)),
            row_ids=None if row_ids is None else np.asarray(row_ids),
            set_qblocks=lambda blocks: None)

    def _launch(self, method, h, X0, X1, C, beta, alpha, gamma, R, norm):
        self.calls.append((method, beta, alpha, gamma, R is not None,
                           norm is not None))
        # the dual-X kernel in numpy: a column c >= 0 reads X0[c], c < 0
        # reads X1[-c - 1]; structure row r writes output row row_ids[r]
        neg = h.indices < 0
        A0 = sparse.csr_matrix((np.where(neg, 0, h.data),
                                np.where(neg, 0, h.indices), h.indptr),
                               shape=(h.shape[0], X0.shape[0]))
        A1 = sparse.csr_matrix((np.where(neg, h.data, 0),
                                np.where(neg, -h.indices - 1, 0), h.indptr),
                               shape=(h.shape[0], X1.shape[0]))
        rows = np.arange(h.shape[0]) if h.row_ids is None else h.row_ids
        dt = self.np_dtype.type
        res = dt(alpha) * (A0 @ X0.numpy() + A1 @ X1.numpy())
        if R is not None:
            res = res + dt(gamma) * R.numpy()[rows]
        c = C.numpy()
        c[rows] = res + c[rows] if beta else res
        if norm is not None:
            D, acc = norm
            super().diffnorm_rows(C[rows], None if D is None else D[rows], acc)

    def spmm_block(self, block, X, C, beta, alpha=1.0, gamma=0.0, R=None,
                   norm=None):
        self._launch('spmm_block', block, X, X, C, beta, alpha, gamma, R, norm)

    def spmm_dual(self, block, X0, X1, C, beta, alpha=1.0, gamma=0.0, R=None,
                  norm=None):
        self._launch('spmm_dual', block, X0, X1, C, beta, alpha, gamma, R, norm)

    def axpby_rows(self, C, R, alpha, gamma):
        self.calls.append(('axpby_rows', None, alpha, gamma, R is not None,
                           False))
        super().axpby_rows(C, R, alpha, gamma)

    def diffnorm_rows(self, C, D, acc):
        self.calls.append(('diffnorm_rows', None, None, None, False, True))
        super().diffnorm_rows(C, D, acc)


# one launch each; the literals below were recorded at the parent commit of
# the change that introduced this file and checked against the layout tables
# of DESIGN.md (affine step, step norms)
def _dual(beta=0, alpha=1.0, gamma=0.0, R=False, norm=False):
    return ('spmm_dual', beta, alpha, gamma, R, norm)


def _block(beta=0, alpha=1.0, gamma=0.0, R=False, norm=False):
    return ('spmm_block', beta, alpha, gamma, R, norm)


TAIL = ('axpby_rows', None, ALPHA, GAMMA, True, False)
MEASURE = ('diffnorm_rows', None, None, None, False, True)

LAYOUTS = {
    'default': ([3], {}),
    'two_launch': ([3], {'ARROW_FUSE_ALL': '0'}),
    'sequential': ([3, 2], {'ARROW_FOLD': '0'}),
    'full_fold': ([3, 2], {'ARROW_FOLD': '1'}),
    'row_fold': ([3, 2], {'ARROW_FOLD': '2'}),
}

# (layout, affine, tracked) -> the launches of ONE step; a run is two steps
ONE_STEP = {
    # the single launch carries the step and measures it
    ('default', False, False): [_dual()],
    ('default', True, False): [_dual(0, ALPHA, GAMMA, R=True)],
    ('default', False, True): [_dual(norm=True)],
    ('default', True, True): [_dual(0, ALPHA, GAMMA, R=True, norm=True)],
    # row-0 launch, rest launch, then the tail, then the stand-alone pass
    ('two_launch', False, False): [_block(), _dual()],
    ('two_launch', True, False): [_block(), _dual(), TAIL],
    ('two_launch', False, True): [_block(), _dual(), MEASURE],
    ('two_launch', True, True): [_block(), _dual(), TAIL, MEASURE],
    # each part's single launch, plain; tail and pass on part 0's aggregate
    ('sequential', False, False): [_dual(), _dual()],
    ('sequential', True, False): [_dual(), _dual(), TAIL],
    ('sequential', False, True): [_dual(), _dual(), MEASURE],
    ('sequential', True, True): [_dual(), _dual(), TAIL, MEASURE],
    # part 0's launch carries alpha and gamma * R, the folded beta=1 launch
    # alpha alone; the pass follows the last folded launch
    ('full_fold', False, False): [_dual(), _block(1)],
    ('full_fold', True, False): [_dual(0, ALPHA, GAMMA, R=True),
                                 _block(1, ALPHA)],
    ('full_fold', False, True): [_dual(), _block(1), MEASURE],
    ('full_fold', True, True): [_dual(0, ALPHA, GAMMA, R=True),
                                _block(1, ALPHA), MEASURE],
    ('row_fold', False, False): [_dual(), _block(1)],
    ('row_fold', True, False): [_dual(0, ALPHA, GAMMA, R=True),
                                _block(1, ALPHA)],
    ('row_fold', False, True): [_dual(), _block(1), MEASURE],
    ('row_fold', True, True): [_dual(0, ALPHA, GAMMA, R=True),
                               _block(1, ALPHA), MEASURE],
}


def _build(monkeypatch, n_blocks, env):
    for key in ('ARROW_FUSE_ALL', 'ARROW_FOLD', 'ARROW_SPLIT_COL',
                'ARROW_PAR_ROW0', 'ARROW_ROW0_CHUNKS', 'ARROW_REST_CHUNK_NNZ'):
        monkeypatch.delenv(key, raising=False)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    backends = []

    def make(device, dtype=np.float32):
        backends.append(_RecordingBackend(dtype))
        return backends[-1]
    monkeypatch.setattr(arrow_slim, 'make_backend', make)
    monkeypatch.setattr(torch.cuda, 'mem_get_info',
                        lambda *a: (1 << 40, 1 << 40))
    decomp = synth.synth_arrow_decomposition(WIDTH, n_blocks, avg_deg=3,
                                             seed=5, dtype=np.float32)
    with tempfile.TemporaryDirectory() as td:
        prefix = os.path.join(td, 'g')
        graphio.save_decomposition_new(decomp, prefix, WIDTH)
        blocks, nb, tp, tn = ArrowDecompositionMPI.load_decomposition_new(
            None, prefix, WIDTH)
        arrow = ArrowDecompositionMPI.initialize(None, nb, tp, tn, WIDTH, K,
                                                 device='gpu')
        arrow.load_data_from_blocks(blocks)
    arrow.zero_rhs(WIDTH, K)
    return arrow, backends


def trace(monkeypatch, n_blocks, env, affine, tracked):
    """The launches of two steps, in order, over all parts' backends."""
    arrow, backends = _build(monkeypatch, n_blocks, env)
    log = []
    for be in backends:
        be.calls = log
    rng = np.random.default_rng(1)
    shape = (n_blocks[0] * WIDTH, K)
    eng0 = arrow.engines[0]
    eng0.set_features((2 * rng.random(shape) - 1).astype(np.float32))
    if affine:
        arrow.set_affine_step(ALPHA, GAMMA,
                              (2 * rng.random(shape) - 1).astype(np.float32))
    if tracked:
        arrow.track_step_norms()
    for _ in range(2):
        step_before = eng0._affine
        arrow.step()
        assert eng0._affine is step_before
        if tracked:
            d, c = arrow.last_step_norms()
            assert d > 0 and c > 0
        eng0.set_features(eng0.result_tile())
    return log


@pytest.mark.parametrize('layout,affine,tracked', sorted(ONE_STEP))
def test_step_launch_sequence(monkeypatch, layout, affine, tracked):
    n_blocks, env = LAYOUTS[layout]
    got = trace(monkeypatch, n_blocks, env, affine, tracked)
    assert got == 2 * ONE_STEP[layout, affine, tracked]


def test_layouts_are_the_ones_named(monkeypatch):
    """The environment of each entry of LAYOUTS builds the layout its name
    says."""
    shape = {}
    for layout, (n_blocks, env) in LAYOUTS.items():
        with monkeypatch.context() as mp:
            arrow, _ = _build(mp, n_blocks, env)
        shape[layout] = (arrow.engines[0]._A_all is not None,
                         arrow._folded is not None, arrow._fold_cols)
    assert shape == {'default': (True, False, True),
                     'two_launch': (False, False, True),
                     'sequential': (True, False, True),
                     'full_fold': (True, True, True),
                     'row_fold': (True, True, False)}
