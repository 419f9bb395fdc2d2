"""The operator-scaling case module, the cpu backend's two passes and the
device-free part of the C ABI, without a GPU: the exact class is exact, the
cpu backend's block_sums / block_scale agree with the module's references
(the same indexing, the same rounding formula), the library exports ABI 1007
and the refusals that launch nothing refuse."""
import ctypes

import numpy as np
import pytest
from scipy import sparse

from arrow_matrix_amd import hip
from arrow_matrix_amd.backends import CpuBackend
from tests import spmm_cases_scale as ss

CASE = {c['name']: c for c in ss.CASES}


def test_case_list_covers_what_it_must():
    lens = np.diff(ss.matrix('std')['indptr'])
    for n in (0, 1, 2047, 2048, 2049, 4097):
        assert (lens == n).any()
    assert (ss.matrix('std_dual')['cols'] < 0).any()
    assert np.diff(ss.matrix('real')['indptr']).max() <= 64   # no split row
    assert ss.matrix('empty')['cols'].size == 0
    rid = ss.row_ids(CASE['std_rowids'])
    assert np.unique(rid).size == rid.size < ss.out_rows(CASE['std_rowids'])
    assert (np.diff(rid) < 0).any()


@pytest.mark.parametrize('name', ['std', 'std_dual', 'std_rowids'])
def test_exact_class_is_exact(name):
    c = CASE[name]
    r, c0, c1 = ss.factors(c)
    scaled = ss.scaled_values(c, 'f32', r, c0, c1)
    assert scaled.dtype == np.float32
    exact = ss.scaled_values(c, 'f64', r, c0, c1)   # no rounding in double
    assert (scaled.astype(np.float64) == exact).all()
    assert np.abs(scaled).max() <= 8 and (scaled / 0.125 % 1 == 0).all()
    X0, X1 = ss.operands(c, 4)
    _, ref = ss.product(c, scaled, X0, X1)
    # fp32 holds every reference value: below 2**24 units of 0.125
    assert (ref.astype(np.float32).astype(np.float64) == ref).all()
    assert np.abs(ref).max() / 0.125 < 2 ** 24
    # sums: exact in double, so any order gives the same bits
    for absolute in (False, True):
        sums = ss.host_sums(c, 'f32', absolute)
        m = ss.matrix(c['matrix'])
        v = np.abs(m['vals']) if absolute else m['vals']
        dense = np.bincount(ss.nnz_rows(c), weights=v.astype(np.float64),
                            minlength=ss.out_rows(c))
        assert (sums[0] == dense).all()
        for s in sums:
            assert (s / 0.5 % 1 == 0).all() and np.abs(s).max() / 0.5 < 2 ** 53


def _backend_block(c, prec):
    """The case as the cpu backend holds a structure: a scipy matrix, or the
    folded (csr, row_ids) pair. Negative columns stay as they are in the raw
    index array (scipy never canonicalises here)."""
    m = ss.matrix(c['matrix'])
    csr = sparse.csr_matrix((m['rows'], m['n0']), dtype=ss.NP_DTYPE[prec])
    csr.indptr = m['indptr'].copy()
    csr.indices = m['cols'].astype(np.int64)
    csr.data = ss.values(c, prec).copy()
    rid = ss.row_ids(c)
    return csr if rid is None else (csr, rid)


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('name', sorted(CASE))
def test_cpu_backend_matches_the_references(name, prec):
    c = CASE[name]
    be = CpuBackend(ss.NP_DTYPE[prec])
    blk = _backend_block(c, prec)
    m = ss.matrix(c['matrix'])
    for absolute in (False, True):
        outs = [be.scale_vector(np.zeros(n))
                for n in (ss.out_rows(c), m['n0'], ss.n1(c))]
        be.block_sums(blk, *outs, absolute)
        be.block_sums(blk, outs[0], None, None, absolute)   # adds, skips
        want = ss.host_sums(c, prec, absolute)
        bound = ss.sum_bound(c, prec)
        for j, (got, w, b) in enumerate(zip(outs, want, bound)):
            calls = 2 if j == 0 else 1
            assert (np.abs(got.numpy() - calls * w) <= calls * b).all()
    with pytest.raises(ValueError):
        be.block_sums(blk, None, None, None)
    r, c0, c1 = ss.factors(c)
    be.block_scale(blk, None, None, None)
    csr = blk[0] if isinstance(blk, tuple) else blk
    assert (csr.data == ss.values(c, prec)).all()
    be.block_scale(blk, *(be.scale_vector(v) for v in (r, c0, c1)))
    want = ss.scaled_values(c, prec, r, c0, c1)
    assert csr.data.dtype == want.dtype
    assert (csr.data.view(np.uint8) == want.view(np.uint8)).all()


def test_abi_and_symbols():
    assert hip.abi_version() >= 1007
    lib = hip._load()
    assert hasattr(lib, 'arrow_csr_sums') and hasattr(lib, 'arrow_csr_scale')
    assert len(lib.arrow_csr_sums.argtypes) == 6
    assert len(lib.arrow_csr_scale.argtypes) == 5
    assert hasattr(hip.CsrBlockGPU, 'sums') and hasattr(hip.CsrBlockGPU, 'scale')


def _err():
    return hip._load().arrow_last_error().decode()


def test_refusals_launch_nothing():
    """Both refusals come before any device call, so host pointers do: a
    negative code, the message, the vectors untouched."""
    lib = hip._load()
    v = np.array([3.5, -2.25])
    p = v.ctypes.data_as(ctypes.c_void_p)
    for handle in (-1, 0, 1 << 40):
        assert lib.arrow_csr_sums(handle, p, p, p, 0, None) < 0
        assert 'arrow_csr_sums: bad handle' in _err()
        assert lib.arrow_csr_scale(handle, p, p, p, None) < 0
        assert 'arrow_csr_scale: bad handle' in _err()
        # a bad handle is refused even where there is nothing to do
        assert lib.arrow_csr_scale(handle, None, None, None, None) < 0
    assert lib.arrow_csr_sums(-1, None, None, None, 1, None) < 0
    assert 'all NULL' in _err()
    assert v.tolist() == [3.5, -2.25]
