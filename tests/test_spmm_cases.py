"""The variant tests' inputs meet the conditions their checks rest on (runs
without a GPU): exact cases are exact, the real-valued bound holds for plain
fp32 sums in either order, and the standard case has the structure the
kernels' edges need."""
import numpy as np
import pytest

from tests import spmm_cases as sc


def _all_cases():
    seen, out = set(), []
    for _, cases in sc.env_table().values():
        for c in cases:
            key = (c['matrix'], c['kind'], c['k'], c['beta'],
                   bool(c.get('row_ids')), str(c.get('legacy')))
            if key not in seen:
                seen.add(key)
                out.append(c)
    return out


def test_exact_cases_are_exact_in_fp32():
    """For every generated exact case scipy's fp32 product equals the
    float64 product exactly, and every row stays inside the headroom the
    argument needs (sum|a||x| + |C0| below 2**18 units of 0.5)."""
    n = 0
    for c in _all_cases():
        if c['kind'] != 'exact':
            continue
        X0, X1, C0 = sc.operands(c)
        m = sc.matrix(c['matrix'])
        assert set(np.unique(np.abs(m['vals']))) <= {0.5, 1.0, 2.0}
        for a in (X0, X1, C0):
            assert np.abs(a).max() <= 8 and (a == np.rint(a)).all()
        assert np.diff(m['indptr']).max() <= 8192
        _, ref64 = sc.reference(c, X0, X1, C0, dtype=np.float64)
        _, ref32 = sc.reference(c, X0, X1, C0, dtype=np.float32)
        assert ref32.dtype == np.float32
        np.testing.assert_array_equal(ref32.astype(np.float64), ref64)
        mag = sc.product(c, X0, X1, np.float64, absolute=True) + 8
        assert 2 * mag.max() < 2 ** 18
        n += 1
    assert n > 50


def _fp32_row_sums(c, X0, X1, C0, reverse):
    m = sc.matrix(c['matrix'])
    vals = m['real_vals'] if c['kind'] == 'legacy' else m['vals']
    X = np.vstack([X0, X1])
    cols = np.where(m['cols'] < 0, m['n0'] - m['cols'].astype(np.int64) - 1,
                    m['cols'])
    out = np.zeros((m['rows'], c['k']), dtype=np.float32)
    for r in range(m['rows']):
        ts = range(m['indptr'][r], m['indptr'][r + 1])
        acc = np.zeros(c['k'], dtype=np.float32)
        for t in (reversed(ts) if reverse else ts):
            acc = acc + vals[t] * X[cols[t]]      # fp32 throughout
        out[r] = acc + C0[r] if c['beta'] else acc
    return out


def test_real_bound_holds_for_fp32_sums_in_both_orders():
    cases = [c for c in _all_cases() if c['kind'] == 'real']
    assert cases
    for c in cases:
        X0, X1, C0 = sc.operands(c)
        m = sc.matrix(c['matrix'])
        assert np.diff(m['indptr']).max() <= 64
        for a in (m['vals'], X0, C0):
            assert 0.25 <= np.abs(a).min() and np.abs(a).max() <= 1.0
        _, ref = sc.reference(c, X0, X1, C0)
        bound = sc.real_bound(c, X0, X1, C0)
        for reverse in (False, True):
            got = _fp32_row_sums(c, X0, X1, C0, reverse).astype(np.float64)
            assert (np.abs(got - ref) <= bound).all()
        # the bound is tight enough to see one dropped term: every term has
        # magnitude >= 1/16, the bound stays far below that
        assert bound.max() < 2.0 ** -4 / 100


def test_standard_case_structure():
    for name in ('std', 'std_dual'):
        m = sc.matrix(name)
        lens = np.diff(m['indptr'])
        assert m['rows'] == 330 and m['n0'] == 2304
        for g in sc.GROUPS:
            for want in (0, 1, g - 1, g, g + 1, 2 * g + 3):
                assert want in lens
        for want in (7, 8, 9, 12, 2047, 2048, 2049, 4097):
            assert want in lens
        empty = (lens == 0).astype(int)
        assert np.convolve(empty, np.ones(20, dtype=int), 'valid').max() == 20
        items = sc.n_items(m)
        assert items == m['rows'] + 1 + 2          # 2049 -> 2, 4097 -> 3 items
        for g in sc.GROUPS:
            assert items % (256 // g) != 0
    m = sc.matrix('std_dual')
    neg = m['cols'] < 0
    assert 0.25 < neg.mean() < 0.35
    assert (-m['cols'][neg] - 1).max() < m['n1']
    for r in np.flatnonzero(np.diff(m['indptr']) > sc.SEG_NNZ):
        assert neg[m['indptr'][r]:m['indptr'][r + 1]].any()
    assert sc.row_ids(dict(matrix='std', row_ids=True)).size == \
        np.unique(sc.row_ids(dict(matrix='std', row_ids=True))).size


def test_loop_cases_exceed_their_caps():
    assert sc.n_items(sc.matrix('stride')) > sc.GRID_STRIDE_CAP * 4
    for r, items in sc.REMAP_ITEMS.items():
        assert sc.n_items(sc.matrix(f'remap{r}')) == items
        assert -(-items // 8) % 8 == r
    z = sc.matrix('zero_rows')
    assert (np.diff(z['indptr']) > sc.SEG_NNZ).sum() * 1024 > 4096 * 256
    n, k = sc.ROUTE_SHAPES[-1]
    assert k % 4 and n * k > 16384 * 256


@pytest.mark.parametrize('op', sc.ROUTE_OPS)
def test_route_reference_leaves_other_rows_alone(op):
    rc = sc.route_case(op, 500, 33)
    if rc['dst_idx'] is not None:
        other = np.setdiff1d(np.arange(rc['dst0'].shape[0]), rc['dst_idx'])
        assert other.size == 13
        np.testing.assert_array_equal(rc['ref'][other], rc['dst0'][other])
        assert np.unique(rc['dst_idx']).size == 500
