"""The parts of tests/spmm_driver.py that need no GPU: the guard layout of
`guarded` on the 'cpu' device, and the comparators of every precision."""
import numpy as np
import pytest

from tests import spmm_driver as drv

PRECS = list(drv.PRECISIONS.values())
IDS = [p.name for p in PRECS]


def _values(shape):
    """Exact in bf16, so the same array serves every precision."""
    rng = np.random.default_rng(5)
    return rng.integers(1, 9, shape).astype(np.float64)


def _host(prec, a):
    return a if prec.name == 'f64' else a.astype(np.float32)


@pytest.mark.parametrize('prec', PRECS, ids=IDS)
def test_guard_layout(prec):
    bits = prec.bits(_host(prec, _values((5, 8))))
    n = bits.size * prec.words_per_element
    buf, view = drv.guarded(prec, bits, prec.c_guard, 'cpu')
    assert view.data_ptr() % 16 == 0
    assert buf.numel() == n + 2 * drv.PAD and view.numel() == n
    assert view.data_ptr() - buf.data_ptr() == drv.PAD * buf.element_size()
    assert (buf[:drv.PAD] == prec.c_guard).all()
    assert (buf[-drv.PAD:] == prec.c_guard).all()
    assert (drv.host_bits(prec, view, bits.shape) == bits).all()
    assert drv.guards_intact(buf, prec.c_guard)
    for at in (drv.PAD - 1, drv.PAD + n):   # just before, just after
        buf, _ = drv.guarded(prec, bits, prec.c_guard, 'cpu')
        buf[at] = 0
        assert not drv.guards_intact(buf, prec.c_guard)


@pytest.mark.parametrize('prec', PRECS, ids=IDS)
def test_exact_check(prec):
    ref = _values((6, 8))
    lens = np.arange(6)
    got = prec.bits(_host(prec, ref)).copy()
    prec.exact(got, ref, lens)
    low = got.copy()
    low[2, 3] ^= 1                          # the lowest bit of one element
    with pytest.raises(drv.Mismatch):
        prec.exact(low, ref, lens)
    nan = got.copy()
    nan[4, 0] = prec.bits(_host(prec, np.full((1,), np.nan)))[0]
    with pytest.raises(drv.Mismatch):
        prec.exact(nan, ref, lens)


@pytest.mark.parametrize('prec', PRECS, ids=IDS)
def test_real_check(prec):
    """got = ref + 1 exactly (small integers): inside a bound of 1, outside
    a bound whose one element is the next double below 1."""
    ref = _values((6, 8))
    if prec.name == 'f64':
        ref = ref.astype(np.longdouble)     # as reference_longdouble gives
    got = prec.bits(_host(prec, np.asarray(ref + 1, dtype=np.float64)))
    bound = np.ones(ref.shape)
    assert prec.real(got, ref, bound) == 1.0
    bound[3, 5] = np.nextafter(1.0, 0.0)
    with pytest.raises(drv.Mismatch):
        prec.real(got, ref, bound)
    with pytest.raises(drv.Mismatch):       # NaN fails too
        nan = got.copy()
        nan[0, 0] = prec.bits(_host(prec, np.full((1,), np.nan)))[0]
        prec.real(nan, ref, np.ones(ref.shape))
