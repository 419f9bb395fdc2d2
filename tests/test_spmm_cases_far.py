"""The far geometry (tests/spmm_cases_far.py) without a GPU: the placements
really cross 2**31 elements, a wrapped offset cannot land on right data, the
indices still fit the int32 the ABI gives them, the compact reference is the
existing modules' own, the contiguous formula is what the driver assumes, the
peak-memory figures follow from the shapes, and arrow_csr_create* refuses
what does not fit int32 before it touches a device."""
import ctypes

import numpy as np
import pytest

from arrow_matrix_amd import hip
from tests import spmm_cases as sc
from tests import spmm_cases_affine as sa
from tests import spmm_cases_far as far
from tests import spmm_cases_norm as sn

B = far.B
GiB = 1 << 30


def _placements(prec):
    """(label, k, placement) of every distinct placement of the precision."""
    for c in far.spmm_cases(prec):
        if c['queue'] == 0:
            yield c['name'], c['k'], far.placement(prec, c)
    for name, op, k, side in far.route_cases(prec):
        yield name, k, far.route_placement(prec, op, k, side)


def test_case_lists():
    assert far.PRECISIONS == ('f32', 'f64', 'bf16')
    assert far.K == {'f32': (3, 16, 130, 260), 'f64': (3, 16, 130),
                     'bf16': (16, 520)}
    for prec in far.PRECISIONS:
        cs = far.spmm_cases(prec)
        names = far.job_names(prec)
        assert len(set(names)) == len(names)
        seen = {(c['k'], c['role'], c['entry'], c['beta'], c['queue'])
                for c in cs}
        want = {(k, role, entry, beta, q) for k in far.K[prec]
                for role in ('read', 'write')
                for entry, beta in (('spmm', 0), ('spmm', 1), ('affine', 0),
                                    ('affine', 1), ('norm', 0))
                for q in (0, 1)}
        assert seen == want and len(cs) == len(want)
        for c in cs:
            assert c['kind'] == 'exact'
            assert c['matrix'] == {'read': 'std_dual', 'write': 'std'}[c['role']]
            assert bool(c.get('row_ids')) == (c['role'] == 'write')
            pair = (c['alpha'], c['gamma'], c['has_R'])
            assert pair == {'spmm': sa.EXACT_PAIRS[2],
                            'affine': sa.EXACT_PAIRS[0],
                            'norm': sn.PAIRS[0]}[c['entry']]
            assert c['plan']['scheduler'] == sc.GRID or c['queue'] == 1
            if c['k'] == far.TWO_LAUNCHES[prec]:
                assert c['plan']['launches'] == 2
        routes = far.route_cases(prec)
        assert len(routes) == len(sc.ROUTE_OPS) * 2 * 2
        assert {k for _, _, k, _ in routes} == set(far.ROUTE_K[prec])
        shapes = [(n, k) for _, kernel, n, k in far.contig_cases(prec)
                  if kernel == 'axpby']
        assert shapes[0] == (2 ** 24 + 3, 128)
        assert (len(shapes) == 2) == (prec != 'bf16')
        if prec != 'bf16':
            assert shapes[1] == (-(-B // 129) + 3, 129)
        assert names[-1] == 'rowid_misuse'
    assert far.ROUTE_K['bf16'] == (24, 128) and far.ROUTE_K['f32'] == (33, 128)


def test_the_matrices_hold_what_the_cases_need():
    for name in ('std', 'std_dual'):
        lens = np.diff(sc.matrix(name)['indptr'])
        assert {2049, 4097} <= set(lens.tolist()) and (lens == 0).any()
    assert sc.matrix('std_dual')['n1'] > 0 and sc.matrix('std')['n1'] == 0


@pytest.mark.parametrize('prec', far.PRECISIONS)
def test_indices_fit_int32(prec):
    for label, k, pl in _placements(prec):
        for buf, first, n in pl['windows'].values():
            assert first + n < 2 ** 31, label
            assert first + n == pl['tall'][buf] or buf == 'X', label
        for rows in pl['touched'].values():
            assert 0 <= rows.min() and rows.max() < 2 ** 31, label
        if pl.get('cols') is not None:
            m = sc.matrix('std_dual')
            _, base0, n0 = pl['windows']['X0']
            _, base1, n1 = pl['windows']['X1']
            c, f = m['cols'].astype(np.int64), pl['cols'].astype(np.int64)
            assert pl['cols'].dtype == np.int32
            assert (f[c >= 0] == c[c >= 0] + base0).all()
            assert (-f[c < 0] - 1 == (-c[c < 0] - 1) + base1).all()
            assert base1 >= base0 + n0 + 1      # NaN rows between the windows
            assert pl['tall']['X'] == base1 + n1
        if pl.get('row_ids') is not None:
            case = dict(matrix='std', row_ids=True)
            _, out_base, W = pl['windows']['C']
            assert (pl['row_ids'] == out_base + sc.row_ids(case)).all()
            assert W == sc.out_rows(case)
            assert np.unique(pl['row_ids']).size == pl['row_ids'].size


@pytest.mark.parametrize('prec', far.PRECISIONS)
def test_windows_straddle_and_wrapped_offsets_miss(prec):
    size = far.ITEMSIZE[prec]
    for label, k, pl in _placements(prec):
        by_buffer = {}
        for name, (buf, first, n) in pl['windows'].items():
            by_buffer.setdefault(buf, []).append((first * k, (first + n) * k))
        lows, highs = {}, {}
        for name, rows in pl['touched'].items():
            buf, first, n = pl['windows'][name]
            assert first <= rows.min() and rows.max() < first + n, label
            off = far.element_offsets(k, rows)
            lows[buf] = min(lows.get(buf, off.min()), off.min())
            highs[buf] = max(highs.get(buf, off.max()), off.max())
            if name != 'X1':         # X1's window follows X0's: all past B
                assert off.min() < B <= off.max(), label
                # the window starts at r_B - W // 2, and a row spans B
                assert first == far.r_B(k) - n // 2, label
                if B % k:
                    assert (far.r_B(k) - 1) * k < B < far.r_B(k) * k
                    assert first <= far.r_B(k) - 1 < first + n
            else:
                assert off.min() >= B
            past = off[off >= B]
            assert past.size and past.max() < 2 ** 32, label
            # an element offset formed in int, and a byte offset formed in
            # 32 bits of either sign: all differ and miss every window
            wrapped = [(past - 2 ** 32, 1)]
            byte = past * size
            u32 = byte % 2 ** 32
            wrapped += [(u32, size), (np.where(u32 >= 2 ** 31, u32 - 2 ** 32,
                                               u32), size)]
            for w, unit in wrapped:
                assert (w != past * unit).all(), label
                for lo, hi in by_buffer[buf]:
                    assert not ((w >= lo * unit) & (w < hi * unit)).any(), label
        for buf in by_buffer:
            assert lows[buf] < B <= highs[buf], label


def test_compact_reference_is_the_existing_one(monkeypatch):
    seen = {}
    for mod, fn in ((sa, 'operands'), (sa, 'reference'), (sn, 'operand_D')):
        def spy(*args, _orig=getattr(mod, fn), _fn=fn, **kw):
            out = _orig(*args, **kw)
            seen.setdefault(_fn, out)    # the first call: compact's own
            return out
        monkeypatch.setattr(mod, fn, spy)
    for prec in far.PRECISIONS:
        k = far.K[prec][1]
        for c in far.spmm_cases(prec):
            if c['k'] != k or c['queue']:
                continue
            seen.clear()
            cp = far.compact(prec, c)
            for key, arr in zip(('X0', 'X1', 'C0', 'R'), seen['operands']):
                assert cp[key] is arr
            assert cp['rows'] is seen['reference'][0]
            assert cp['ref'] is seen['reference'][1]
            if c['entry'] != 'norm':
                assert cp['D'] is None
            elif c['role'] == 'write':
                assert cp['D'] is cp['R']        # D = R
            else:
                assert cp['D'] is seen['operand_D']
            # and with the caller's shared product: the same bits
            X0, X1, C0, R = seen['operands']
            P = sa.plain_product(prec, c, X0, X1)
            again = far.compact(prec, c, shared=(X0, X1, C0, R, P))
            assert (again['ref'] == cp['ref']).all()
            assert (again['rows'] == cp['rows']).all()


def test_route_placements():
    for prec in far.PRECISIONS:
        for name, op, k, side in far.route_cases(prec):
            rp = far.route_placement(prec, op, k, side)
            rc = sa._mod(prec).route_case(op, far.ROUTE_N, k)
            for key in ('src', 'dst0', 'ref'):
                assert (rp['rc'][key] == rc[key]).all()
            W = (rc['src'] if side == 'src' else rc['dst0']).shape[0]
            assert W == far.route_window_rows(op, side)
            idx = rc[side + '_idx']
            if idx is None:
                assert rp['idx'] is None and rp['ptr_row'] == rp['base']
                # a vector lane needs 16-byte alignment of the moved pointer
                assert rp['base'] * k * far.ITEMSIZE[prec] % 16 == 0 \
                    or k * far.ITEMSIZE[prec] % 16
            else:
                assert rp['ptr_row'] == 0
                assert (rp['idx'] == idx + rp['base']).all()
                assert rp['idx'].dtype == np.int64


def test_contiguous_formula_and_sums():
    for which, (mult, shift) in enumerate(far.FORMULA):
        biggest = max(n * k for shapes in far.CONTIG_SHAPES.values()
                      for n, k in shapes)
        assert biggest * mult < 2 ** 63          # the int64 product holds
        for lo in (0, B - 5000, biggest - 10000):
            i = np.arange(lo, lo + 10000, dtype=np.int64)
            v = far.formula(i, which)
            assert v.dtype == np.int64
            assert v.min() >= -8 and v.max() <= 8
            assert v.tolist() == [((int(j) * mult) >> shift) % 17 - 8
                                  for j in i]
        i = np.arange(1 << 20, dtype=np.int64)
        assert set(far.formula(i, which).tolist()) == set(range(-8, 9))
    i = np.arange(4096, dtype=np.int64)
    assert (far.formula(i, 0) != far.formula(i, 1)).any()
    for prec, shapes in far.CONTIG_SHAPES.items():
        for n, k in shapes:
            assert B < n * k < B + 1024
            # (c - d)^2 <= 256 per element: both int64 sums are exact doubles
            assert n * k * 256 < 2 ** 40 < 2 ** 53
    assert far.CONTIG_PAIR['f64'] == sa.EXACT_PAIRS[2]
    assert far.CONTIG_PAIR['f32'] == far.CONTIG_PAIR['bf16'] \
        == sa.EXACT_PAIRS[0]
    assert 129 % 4 and 129 % 2      # the one-element-per-thread path


def test_peak_memory_from_the_shapes():
    """Two buffers of (2**31 + window) elements at the most: about 8 GiB in
    bf16, 16 GiB in f32, 32 GiB in f64 far-write affine / norm and 16 GiB in
    every other f64 case."""
    slack = 1 << 24         # the windows and the guard pads
    for prec in far.PRECISIONS:
        one = B * far.ITEMSIZE[prec]
        peaks = far.job_peaks(prec)
        for c in far.spmm_cases(prec):
            pl = far.placement(prec, c)
            n_tall = 2 if c['role'] == 'write' and c['has_R'] else 1
            assert len(pl['tall']) == n_tall
            want = sum(rows * c['k'] * far.ITEMSIZE[prec]
                       + 2 * far.PAD * far.WORDSIZE[prec]
                       for rows in pl['tall'].values())
            assert peaks[c['name']] == want
            assert n_tall * one < want < n_tall * one + slack
        for name, op, k, side in far.route_cases(prec):
            assert one < peaks[name] < one + slack
        for name, kernel, n, k in far.contig_cases(prec):
            n_tall = 1 if prec == 'f64' else 2
            assert n_tall * one < peaks[name] < n_tall * one + slack
        assert peaks['rowid_misuse'] == 0
        top = max(peaks.values())
        assert 2 * one < top < 2 * one + slack
        assert top // GiB == {'bf16': 8, 'f32': 16, 'f64': 32}[prec]
    others = [v for name, v in far.job_peaks('f64').items()
              if not (name.startswith('farwrite_affine')
                      or name.startswith('farwrite_norm'))]
    assert max(others) // GiB == 16


def test_guard_pad_is_the_drivers():
    from tests import spmm_driver as sd
    assert far.PAD == sd.PAD
    for prec, p in sd.PRECISIONS.items():
        assert np.dtype(p.word).itemsize == far.WORDSIZE[prec]
        assert np.dtype(p.bits_dtype).itemsize == far.ITEMSIZE[prec]


# ---------------------------------------------------------------------------
# arrow_csr_create*: what does not fit int32 is refused on the host
# ---------------------------------------------------------------------------

def _create(f64, rows, cols, row_ids, indptr=None):
    lib = hip._load()
    m = sc.matrix('std')
    indptr = np.ascontiguousarray(m['indptr'] if indptr is None else indptr,
                                  dtype=np.int64)
    idx = np.ascontiguousarray(m['cols'], dtype=np.int32)
    vals = np.ascontiguousarray(m['vals'],
                                dtype=np.float64 if f64 else np.float32)
    fn = lib.arrow_csr_create_f64 if f64 else lib.arrow_csr_create_opts
    ctype = ctypes.c_double if f64 else ctypes.c_float
    rid = None if row_ids is None else \
        row_ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    rc = fn(rows, cols, idx.size,
            indptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            vals.ctypes.data_as(ctypes.POINTER(ctype)), rid, 0)
    return rc, lib.arrow_last_error().decode()


@pytest.mark.parametrize('f64', [False, True])
def test_create_refuses_row_ids_outside_int32(f64):
    """The refusal comes before any allocation and any device call, so it
    needs no GPU."""
    m = sc.matrix('std')
    for at, bad in ((7, 2 ** 31), (0, 2 ** 31 + 5), (m['rows'] - 1, -1),
                    (7, 2 ** 40), (7, -2 ** 31)):
        rid = np.arange(m['rows'], dtype=np.int64)
        rid[at] = bad
        rc, msg = _create(f64, m['rows'], m['n0'], rid)
        assert rc == -1
        assert 'row id' in msg and 'int32' in msg
        assert str(bad) in msg and f'row {at}' in msg
    rid = np.arange(m['rows'], dtype=np.int64)
    rid[7] = 2 ** 31
    _, msg = _create(f64, m['rows'], m['n0'], rid)
    assert msg == 'arrow_csr_create: row id 2147483648 at row 7 exceeds int32'


@pytest.mark.parametrize('f64', [False, True])
def test_create_refuses_rows_and_cols_outside_int32(f64):
    m = sc.matrix('std')
    # refused before indptr is read: a short one does
    rc, msg = _create(f64, 2 ** 31, m['n0'], None, indptr=[0, 0])
    assert rc == -1 and 'rows 2147483648' in msg and 'int32' in msg
    rc, msg = _create(f64, m['rows'], 2 ** 31, None)
    assert rc == -1 and 'cols 2147483648' in msg and 'int32' in msg
