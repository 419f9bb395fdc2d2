"""The affine-step test inputs check themselves, the new ABI symbols resolve,
the refusals that need no device refuse, and the cpu device computes
X <- alpha * A@X + gamma * R: on the CPU, against the built library."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import spmm_cases as sc
from tests import spmm_cases_affine as sa
from tests import spmm_cases_bf16 as s16

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def hip():
    from arrow_matrix_amd import hip
    if not hip.is_built():
        subprocess.run(['make', '-C',
                        os.path.join(REPO, 'arrow_matrix_amd', 'csrc')],
                       check=True, capture_output=True)
    return hip


def _case(matrix, kind, k, beta, pair, **opts):
    return sa.case('t', matrix, kind, k, beta, 0, pair, **opts)


# ---------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('prec', sa.PRECISIONS)
@pytest.mark.parametrize('matrix,opts', [('std', {}), ('std_dual', {}),
                                         ('std', dict(row_ids=True))])
def test_reference_equals_a_dense_float64_evaluation(prec, matrix, opts):
    k = 8
    for beta in (0, 1):
        for pair in sa.EXACT_PAIRS:
            c = _case(matrix, 'exact', k, beta, pair, **opts)
            ops = sa.operands(prec, c)
            rows, ref = sa.reference(prec, c, *ops)
            rows_d, dense = sa.dense_reference(prec, c, *ops)
            np.testing.assert_array_equal(rows, rows_d)
            np.testing.assert_array_equal(ref, dense)    # both exact
            assert ops[3].shape == ops[2].shape == (sc.out_rows(c), k)


@pytest.mark.parametrize('prec', sa.PRECISIONS)
def test_real_reference_is_within_its_own_bound_of_the_dense_one(prec):
    c = _case('real', 'real', 24, 1, sa.REAL_PAIR)
    ops = sa.operands(prec, c)
    _, ref = sa.reference(prec, c, *ops)
    _, dense = sa.dense_reference(prec, c, *ops)
    bound = sa.real_bound(prec, c, *ops, ref)
    assert (bound > 0).all()
    # the float64 dense evaluation carries float64 error only
    b64 = sa.real_bound('f64', c, *ops, ref)
    assert (np.abs(ref.astype(np.float64) - dense) <= b64).all()
    if prec != 'f64':
        assert (b64 < 2.0 ** -20 * bound).all()


def test_exact_class_really_is_exact():
    """Every term a multiple of 0.25 (float64: of 2**-32), the sum of all
    magnitudes below 2**20 such units' worth of fp32 significand: any order
    of fp32 operations, fused or not, alpha per partial or once, is exact."""
    lens = np.diff(sc.matrix('std')['indptr'])
    assert sorted(lens[lens > sc.SEG_NNZ]) == [2049, 4097]
    assert (lens == 0).sum() >= 20
    for prec, unit in (('f32', 0.25), ('bf16', 0.25), ('f64', 2.0 ** -32)):
        for matrix in ('std', 'std_dual'):
            for beta in (0, 1):
                for pair in sa.EXACT_PAIRS:
                    c = _case(matrix, 'exact', 16, beta, pair)
                    X0, X1, C0, R = sa.operands(prec, c)
                    assert (np.abs(R) <= 8).all() and (R == np.rint(R)).all()
                    mag = abs(pair[0]) * sa.abs_product(prec, c, X0, X1) \
                        + abs(pair[1]) * np.abs(R) + np.abs(C0)
                    assert (mag / unit).max() < 2 ** 20 / unit * 0.25
                    _, ref = sa.reference(prec, c, X0, X1, C0, R)
                    q = ref / unit
                    assert (q == np.rint(q)).all()
    # alpha applied to each split-row partial in fp32 == applied once
    c = _case('std', 'exact', 4, 0, sa.EXACT_PAIRS[0])
    m = sc.matrix('std')
    X0, X1, C0, R = sa.operands('f32', c)
    _, ref = sa.reference('f32', c, X0, X1, C0, R)
    r = int(np.argmax(lens))
    acc = (np.float32(2.0) * R[r]).astype(np.float32)
    for s in range(m['indptr'][r], m['indptr'][r + 1], sc.SEG_NNZ):
        t = slice(s, min(s + sc.SEG_NNZ, m['indptr'][r + 1]))
        part = np.zeros(4, dtype=np.float32)
        for v, col in zip(m['vals'][t], m['cols'][t]):
            part = (v * X0[col] + part).astype(np.float32)
        acc = (acc + np.float32(0.5) * part).astype(np.float32)
    np.testing.assert_array_equal(acc.astype(np.float64), ref[r])


def test_bf16_exact_class_catches_a_second_rounding():
    """Rounding alpha * sum to bf16 before adding gamma * R (what a separate
    tail pass after a bf16 launch does) lands on other bits somewhere."""
    c = _case('std', 'exact', 8, 1, sa.EXACT_PAIRS[0])
    X0, X1, C0, R = sa.operands('bf16', c)
    rows, ref = sa.reference('bf16', c, X0, X1, C0, R)
    P = sa.plain_product('bf16', c, X0, X1)
    twice = s16.bf16_to_f64(s16.bf16_bits(P + C0[rows])) * 0.5 + 2.0 * R[rows]
    assert (s16.bf16_bits(twice) != s16.bf16_bits(ref)).any()


def test_case_lists_are_well_formed():
    for prec in sa.PRECISIONS:
        for env in sa.ENVS:
            cases = sa.gpu_cases(prec, env)
            names = [c['name'] for c in cases]
            assert len(names) == len(set(names))
            std = [c for c in cases if c['matrix'] == 'std'
                   and not c.get('row_ids') and not c.get('col_items')
                   and not c.get('qblocks')]
            assert {c['k'] for c in std} == set(sa.ks(prec))
            assert {(c['alpha'], c['gamma'], c['has_R']) for c in std} \
                == set(sa.EXACT_PAIRS)
            assert {c['beta'] for c in cases} == {0, 1}
            assert {c['queue'] for c in cases} == {0, 1}
            assert any(c.get('row_ids') for c in cases)
            assert {c.get('col_items', 0) for c in cases} == {0, 1, 2}
            assert any(c.get('qblocks') for c in cases)
            assert any(c['kind'] == 'real' for c in cases)
            assert ('zero_rows' in {c['matrix'] for c in cases}) \
                == (env == 'default')
    assert set(sa.K_F) == {1, 3, 4, 16, 36, 128, 130, 260}
    assert {'default', 'qwave1', 'qwave0', 'nt0'} <= set(sa.ENVS)
    last = sa.AXPBY_SHAPES['f32'][-1]
    assert last[0] * last[1] > 16384 * 256
    last = sa.AXPBY_SHAPES['bf16'][-1]
    assert last[0] * last[1] // 8 > 16384 * 256


# ---------------------------------------------------------------------------
# the library and the binding
# ---------------------------------------------------------------------------

def test_abi_version_and_symbols(hip):
    assert hip.abi_version() >= 1005
    lib = hip._load()
    for sfx in ('', '_f64', '_bf16'):
        for name in ('arrow_spmm_affine', 'arrow_spmm_dual_affine'):
            fn = getattr(lib, name + sfx)
            assert fn.argtypes.count(ctypes.c_double) == 2
    for sfx in ('_f32', '_f64', '_bf16'):
        assert getattr(lib, 'arrow_axpby_rows' + sfx).argtypes[-3:-1] \
            == [ctypes.c_double, ctypes.c_double]
    # the plain entry points keep their symbols
    for name in ('arrow_spmm', 'arrow_spmm_dual', 'arrow_spmm_plan'):
        for sfx in ('', '_f64', '_bf16'):
            assert getattr(lib, name + sfx)


def test_refusals_that_need_no_device(hip):
    # the plan describes an affine launch too: bf16 k % 8 is refused there
    with pytest.raises(hip.ArrowSpmmError, match='k % 8'):
        hip.spmm_plan(12, 1000, -1, dtype='bfloat16')
    lib = hip._load()
    # a bad handle is refused before anything else is looked at
    assert lib.arrow_spmm_affine(0, None, None, None, 8, 1.0, 0.0, 0,
                                 None) < 0
    assert 'arrow_spmm_affine' in lib.arrow_last_error().decode()
    assert lib.arrow_axpby_rows_bf16(None, None, 0, 12, 1.0, 0.0, None) < 0
    assert 'k % 8' in lib.arrow_last_error().decode()
    # refused before C is looked at: any non-null pointer will do
    c = ctypes.c_void_p(64)
    assert lib.arrow_axpby_rows_f32(c, None, 1, 4, 1.0, 2.0, None) < 0
    assert 'R is NULL' in lib.arrow_last_error().decode()
    assert lib.arrow_axpby_rows_f64(c, c, 1, 4, 1.0, 2.0, None) < 0
    assert 'R must not be C' in lib.arrow_last_error().decode()
    assert lib.arrow_axpby_rows_f64(None, None, 0, 4, 1.0, 2.0, None) == 0

    from arrow_matrix_amd.arrow_dec import ArrowDecompositionMPI
    from arrow_matrix_amd.arrow_slim import ArrowSlimMPI
    from arrow_matrix_amd.comm import Comm

    class TwoRanks(Comm):
        size = 2

    e = ArrowSlimMPI(TwoRanks(), tiles_per_side=2, device='cpu')
    with pytest.raises(NotImplementedError, match='single-process'):
        e.set_affine_step(0.85, 0.15, np.zeros((8, 8), dtype=np.float32))
    # device='gpu': refused before any device work (no backend is needed)
    for cls in (ArrowSlimMPI, ArrowDecompositionMPI):
        g = cls.__new__(cls)
        g.comm, g.device = TwoRanks(), 'gpu'
        with pytest.raises(NotImplementedError, match='single-process'):
            g.set_affine_step(0.85, 0.15, None)

    one = ArrowSlimMPI(None, tiles_per_side=2, device='cpu')
    one.zero_rhs(4, 8)
    with pytest.raises(ValueError, match='residual'):
        one.set_affine_step(0.85, 0.15, None)
    with pytest.raises(ValueError, match='shape'):
        one.set_affine_step(0.85, 0.15, np.zeros((8, 4), dtype=np.float32))
    with pytest.raises(TypeError, match='dtype'):
        one.set_affine_step(0.85, 0.15, np.zeros((8, 8), dtype=np.float64))
    one.set_affine_step(0.85, 0.15, np.ones((8, 8), dtype=np.float32))
    assert one._R is not one.C_i and one._R is not one.X_i
    with pytest.raises(ValueError, match='clear_affine_step'):
        one.zero_rhs(4, 16)
    one.clear_affine_step()
    assert one._affine is None and one._R is None
    one.set_affine_step(2.0)          # alpha alone needs no residual
    assert one._affine == (2.0, 0.0, None)


def test_cpu_backend_is_the_parity_reference():
    from scipy import sparse
    from arrow_matrix_amd.backends import CpuBackend
    be = CpuBackend()
    rng = np.random.default_rng(5)
    A = sparse.random(6, 5, density=0.5, format='csr', random_state=3,
                      dtype=np.float32)
    X = rng.integers(-8, 9, (5, 3)).astype(np.float32)
    R = rng.integers(-8, 9, (6, 3)).astype(np.float32)
    C0 = rng.integers(-8, 9, (6, 3)).astype(np.float32)
    for beta in (0, 1):
        C = torch.from_numpy(C0.copy())
        be.spmm_block(A, torch.from_numpy(X), C, beta, alpha=0.5, gamma=2.0,
                      R=torch.from_numpy(R))
        want = np.float32(0.5) * (A @ X) + 2.0 * R + beta * C0
        np.testing.assert_array_equal(C.numpy(), want.astype(np.float32))
    C = torch.from_numpy(C0.copy())
    be.spmm_block(A, torch.from_numpy(X), C, 0)      # the plain call
    np.testing.assert_array_equal(C.numpy(), A @ X)
    C = torch.from_numpy(C0.copy())
    be.axpby_rows(C, torch.from_numpy(R), -2.0, -0.5)
    np.testing.assert_array_equal(C.numpy(), -2.0 * C0 - 0.5 * R)
    C = torch.from_numpy(C0.copy())
    be.axpby_rows(C, None, 0.5, 0.0)
    np.testing.assert_array_equal(C.numpy(), 0.5 * C0)


# ---------------------------------------------------------------------------
# the cpu engine
# ---------------------------------------------------------------------------

def _cpu_engine(n_blocks, width, k, seed):
    from arrow_matrix_amd import graphio, synth
    from arrow_matrix_amd.arrow_dec import ArrowDecompositionMPI
    decomp = synth.synth_arrow_decomposition(width, n_blocks, avg_deg=5,
                                             seed=seed)
    with tempfile.TemporaryDirectory() as td:
        prefix = os.path.join(td, 'g')
        graphio.save_decomposition_new(decomp, prefix, width)
        blocks, nb, tp, tn = ArrowDecompositionMPI.load_decomposition_new(
            None, prefix, width, is_block_diagonal=True)
        arrow = ArrowDecompositionMPI.initialize(None, nb, tp, tn, width, k,
                                                 device='cpu')
        arrow.load_data_from_blocks(blocks)
        arrow.zero_rhs(width, k)
    A = synth.recompose(decomp).astype(np.float64).tocsr()
    return arrow, A, decomp[0][1]


@pytest.mark.parametrize('n_blocks,width,k,seed', [([3], 5, 4, 0),
                                                   ([4, 2], 5, 8, 3)])
def test_cpu_engine_affine_steps(n_blocks, width, k, seed):
    """Three steps of X <- 0.85 A@X + 0.15 R on the cpu device, each against
    the float64 evaluation of the engine's own previous features on the
    recomposed matrix, to the fp32 gate of tests/test_engine_cpu.py's
    iterated test. Then clear_affine_step(): the plain step again."""
    arrow, A, perm0 = _cpu_engine(n_blocks, width, k, seed)
    n = n_blocks[0] * width
    rng = np.random.default_rng(seed)
    X = (2 * rng.random((n, k)) - 1).astype(np.float32)
    R = (2 * rng.random((n, k)) - 1).astype(np.float32)
    arrow.B.set_features(X[perm0].copy())
    arrow.set_affine_step(0.85, 0.15, R[perm0].copy())
    for step in range(4):
        if step == 3:
            arrow.clear_affine_step()
        Xin = np.empty((n, k))
        Xin[perm0] = arrow.B.feature_tile().numpy().astype(np.float64)
        arrow.step()
        C = arrow.B.allgather_result()
        G = A @ Xin
        if step < 3:
            G = 0.85 * G + 0.15 * R.astype(np.float64)
        np.testing.assert_allclose(C, G[perm0], rtol=1e-4, atol=1e-4)
        assert np.abs(G).max() > 0
        arrow.B.set_features(arrow.B.result_tile())


def test_cpu_slim_engine_alone_and_residual_is_a_copy():
    arrow, A, perm0 = _cpu_engine([3], 5, 4, 1)
    eng = arrow.B
    n = 15
    rng = np.random.default_rng(9)
    X = (2 * rng.random((n, 4)) - 1).astype(np.float32)
    R = torch.from_numpy((2 * rng.random((n, 4)) - 1).astype(np.float32))
    Rp = R[torch.from_numpy(perm0)].contiguous()
    eng.set_features(X[perm0].copy())
    eng.set_affine_step(0.5, 2.0, Rp)
    keep = Rp.clone()
    Rp.zero_()                                       # the engine holds a copy
    eng.spmm()
    G = 0.5 * (A @ X.astype(np.float64)) + 2.0 * R.numpy().astype(np.float64)
    np.testing.assert_allclose(eng.allgather_result(), G[perm0], rtol=1e-4,
                               atol=1e-4)
    np.testing.assert_array_equal(eng._R.numpy(), keep.numpy())
