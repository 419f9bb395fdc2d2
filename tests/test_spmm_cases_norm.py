"""The step-norm case module and the device-free part of the C ABI, without a
GPU: the integer reference agrees with a dense float64 computation, the exact
class really is exact in double, the library exports ABI 1006, and the
refusals that launch nothing refuse."""
import ctypes

import numpy as np
import pytest

from arrow_matrix_amd import hip
from tests import spmm_cases_affine as sa
from tests import spmm_cases_norm as sn

# (matrix, k) per exact precision: two column tiles of fp32 and of bf16, the
# dual structure, and the 1025 split rows of `zero_rows`
EXACT = [('f32', 'std', 260), ('bf16', 'std', 520), ('f32', 'std_dual', 128),
         ('bf16', 'std_dual', 128), ('f32', 'zero_rows', 1024),
         ('bf16', 'zero_rows', 1024)]


@pytest.mark.parametrize('prec,matrix,k', EXACT)
def test_exact_class_is_exact_in_double(prec, matrix, k):
    worst = 0
    for pair in sa.EXACT_PAIRS:
        case = sn.case('t', matrix, 'exact', k, 0, pair)
        X0, X1, C0, R = sa.operands(prec, case)
        rows, ref = sa.reference(prec, case, X0, X1, C0, R)
        _, dense = sa.dense_reference(prec, case, X0, X1, C0, R)
        assert (ref == dense).all()
        c = sn.stored(prec, ref)
        d = sn.operand_D(prec, case)[rows].astype(np.float64)
        # c - d is formed in fp32 on the device: it must hold it exactly
        diff = c - d
        assert (diff.astype(np.float32).astype(np.float64) == diff).all()
        u0, u1 = sn.exact_units(c, d)
        assert u0 < 2 ** 53 and u1 < 2 ** 53
        worst = max(worst, u0, u1)
        # the integer reference against plain float64 numpy, which is exact
        # too below 2**53 units, in numpy's own (pairwise) order
        s0, s1 = sn.exact_sums(c, d)
        assert s0 == float(np.square(diff).sum())
        assert s1 == float(np.square(c).sum())
        assert (s0, s1) == sn.host_sums(c, d)
        n0, n1 = sn.exact_sums(c, None)
        assert n0 == n1 == s1
    assert worst > 0


def test_bound_is_the_derived_one():
    u, e = 2.0 ** -24, 2.0 ** -53
    b0, b1 = sn.norm_bound('f32', 1000, 4.0, 2.0)
    assert b0 == pytest.approx(4.0 * (2 * u + 1001 * e), rel=1e-6)
    assert b1 == pytest.approx(2.0 * 1001 * e, rel=1e-6)
    b0, b1 = sn.norm_bound('f64', 1000, 4.0, 2.0)
    assert b0 == pytest.approx(4.0 * 1003 * e, rel=1e-6)


def test_case_lists():
    for prec in sn.PRECISIONS:
        for env in sn.ENVS:
            cs = sn.gpu_cases(prec, env)
            names = [c['name'] for c in cs]
            assert len(set(names)) == len(names)
            assert all(c['beta'] == 0 for c in cs)
            assert {c['queue'] for c in cs} == {0, 1}
            assert any(c.get('row_ids') for c in cs)
            assert ('zero_rows_k1024' in names) == (env == 'default')


def test_abi_and_symbols():
    assert hip.abi_version() >= 1006
    lib = hip._load()
    for sfx in ('', '_f64', '_bf16'):
        assert hasattr(lib, 'arrow_spmm_affine_norm' + sfx)
        assert hasattr(lib, 'arrow_spmm_dual_affine_norm' + sfx)
    for sfx in ('_f32', '_f64', '_bf16'):
        assert hasattr(lib, 'arrow_diffnorm_rows' + sfx)


def _err():
    return hip._load().arrow_last_error().decode()


@pytest.mark.parametrize('sfx,dtype', [('_f32', np.float32),
                                       ('_f64', np.float64),
                                       ('_bf16', np.uint16)])
def test_diffnorm_refusals_launch_nothing(sfx, dtype):
    """The refusals of the stand-alone pass come before any device call, so
    host pointers do: a negative code, the message, acc untouched."""
    fn = getattr(hip._load(), 'arrow_diffnorm_rows' + sfx)
    C = np.ones((4, 8), dtype=dtype)
    D = np.ones((4, 8), dtype=dtype)
    acc = np.array([3.5, -2.25])
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert fn(p(C), p(D), 4, 8, None, None) < 0
    assert 'acc is NULL' in _err()
    assert fn(p(C), p(C), 4, 8, p(acc), None) < 0
    assert 'D must not be C' in _err()
    assert fn(p(C), p(D), -1, 8, p(acc), None) < 0
    assert 'bad arguments' in _err()
    if sfx == '_bf16':
        assert fn(p(C), p(D), 4, 12, p(acc), None) < 0
        assert 'k % 8' in _err()
    assert acc.tolist() == [3.5, -2.25]


@pytest.mark.parametrize('sfx', ['', '_f64', '_bf16'])
def test_norm_entry_points_refuse_a_bad_handle(sfx):
    lib = hip._load()
    acc = np.array([3.5, -2.25])
    a = acc.ctypes.data_as(ctypes.c_void_p)
    rc = getattr(lib, 'arrow_spmm_affine_norm' + sfx)(
        -1, a, a, None, None, a, 8, 1.0, 0.0, 0, None)
    assert rc < 0 and 'arrow_spmm_affine_norm' + sfx in _err()
    rc = getattr(lib, 'arrow_spmm_dual_affine_norm' + sfx)(
        -1, a, a, a, None, None, a, 8, 1.0, 0.0, 0, None)
    assert rc < 0 and 'bad handle' in _err()
    assert acc.tolist() == [3.5, -2.25]
