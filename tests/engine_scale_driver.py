"""The operator-scaling engine checks shared by test_engine_scale_cpu.py and
test_gpu_scale_engine.py, and their child entry point: `python
tests/engine_scale_driver.py <mode> <device>` runs one entry of MODES on the
cpu or gpu device, in every precision the device has, in a process whose
environment selects the engine layout (ARROW_FUSE_ALL / ARROW_FOLD are read
when the structures are built), and prints one JSON line per precision. Built
on tests/engine_affine_driver.py and the job loop of tests/child_harness.py.
This is a plain module, not a test file.

The oracle is scipy on synth.recompose, indexed by perm0: vectors of the
engine are in part 0's layout, as features are, so entry j belongs to
original row (column) perm0[j]. The engine sums every STORED value, so where
parts overlap the absolute sums are those of sum_i P_i^T |B_i| P_i, and the
term count n of a row is its number of stored values over all parts.

Bounds (derived, not measured; u_T is the rounding unit of the resident
values, 2**-24 for float32 and bfloat16 features, 2**-53 for float64):
  * a sum:        |err| <= n 2**-53 sum|v|          (spmm_cases_scale.sum_bound)
  * a normalised row or column of nonnegative values:
                  |sum - 1| <= u_T + n 2**-53       (.normalised_bound)
  * 'sym':        row i of D_r^-1/2 |A| D_c^-1/2 holds the values v r_i c_j,
                  each rounded once to T (u_T) after two double multiplies
                  (2 2**-53) by factors whose own sums and square roots err
                  by at most (n_i + 2) 2**-53 and (n_j + 2) 2**-53 relative;
                  with n_c the longest column, |err| <=
                  (u_T + (2 n_i + n_c + 8) 2**-53) S_i, the n_i of the check's
                  own sum included.
"""
import os
import sys
import tempfile

import numpy as np

if not __package__:         # started as a script: see tests/child_harness.py
    import child_harness  # noqa: F401
from tests import child_harness as ch  # noqa: E402

from tests import engine_affine_driver as ead  # noqa: E402
from tests import engine_norm_driver as end  # noqa: E402
from tests import spmm_cases_scale as ss  # noqa: E402
from tests.gpu_children import ENGINE_VARS  # noqa: E402

L1S = dict(end.ITER_SHAPE)        # widths and blocks of the iterate() check
# mode -> (variables, build arguments); from the engine drivers' mode tables
MODES = {
    'default': ({}, L1S),
    'fuse_all0': ({'ARROW_FUSE_ALL': '0'}, L1S),
    'fold0': ({'ARROW_FOLD': '0'}, ead.L2),
    'fold1': ({'ARROW_FOLD': '1'}, ead.L2),
    'fold2': ({'ARROW_FOLD': '2'}, ead.L2),
    'banded': ({'ARROW_FUSE_ALL': '0'}, ead.BANDED),
    'hub': ({}, ead.HUB),         # split rows: atomics in the step
}
PRECISIONS = {'cpu': ('float32', 'float64'),
              'gpu': ('float32', 'float64', 'bfloat16')}
PREC_TAG = end.PREC_TAG


def make_decomp(n_blocks, width, seed, hub_rows=0, hub_deg=None,
                block_diagonal=True, **_):
    from arrow_matrix_amd import synth
    return synth.synth_arrow_decomposition(
        width, n_blocks, avg_deg=6, seed=seed, hub_rows=hub_rows,
        hub_deg=hub_deg, block_diagonal=block_diagonal, dtype=np.float32)


def load(decomp, precision, device, width, k, block_diagonal=True, slim=True,
         **_):
    """save -> load_decomposition_new -> initialize -> zero_rhs."""
    from arrow_matrix_amd import graphio
    from arrow_matrix_amd.arrow_dec import ArrowDecompositionMPI
    dtype = ead.dtype_of(precision)
    with tempfile.TemporaryDirectory() as td:
        prefix = os.path.join(td, 'g')
        graphio.save_decomposition_new(decomp, prefix, width,
                                       block_diagonal=block_diagonal)
        blocks, nb, tp, tn = ArrowDecompositionMPI.load_decomposition_new(
            None, prefix, width, is_block_diagonal=block_diagonal,
            datatype=dtype)
        arrow = ArrowDecompositionMPI.initialize(
            None, nb, tp, tn, width, k, device=device,
            block_diagonal=block_diagonal, slim=slim, dtype=dtype)
        arrow.load_data_from_blocks(blocks)
        arrow.zero_rhs(width, k, dtype=dtype)
    return arrow


class Oracle:
    """scipy on the recomposed matrix, in float64, original row order."""

    def __init__(self, decomp):
        from arrow_matrix_amd import synth
        f8 = [(B.astype(np.float64), p) for B, p in decomp]
        self.A = synth.recompose(f8).tocsr()
        self.absA = synth.recompose([(abs(B), p) for B, p in f8]).tocsr()
        ones = []
        for B, p in f8:
            P = B.copy()
            P.data[:] = 1.0
            ones.append((P, p))
        count = synth.recompose(ones).tocsr()    # stored values per entry
        self.n_row = np.asarray(count.sum(axis=1)).ravel()
        self.n_col = np.asarray(count.sum(axis=0)).ravel()
        self.perm0 = decomp[0][1]

    def sums(self, absolute):
        M = self.absA if absolute else self.A
        return (np.asarray(M.sum(axis=1)).ravel(),
                np.asarray(M.sum(axis=0)).ravel())

    def sum_bounds(self):
        mr, mc = self.sums(True)
        return self.n_row * 2.0 ** -53 * mr, self.n_col * 2.0 ** -53 * mc


def check_sums(arrow, orc):
    p = orc.perm0
    worst = 0.0
    for absolute in (False, True):
        got_r, got_c = arrow.operator_sums(absolute=absolute)
        assert got_r.dtype == got_c.dtype == np.float64
        assert got_r.shape == got_c.shape == (p.size,)
        want_r, want_c = orc.sums(absolute)
        b_r, b_c = orc.sum_bounds()
        for got, want, b in ((got_r, want_r, b_r), (got_c, want_c, b_c)):
            err = np.abs(got - want[p])
            assert (err <= b[p]).all(), \
                f"sums absolute={absolute}: max err {err.max()}, " \
                f"max err/bound {(err / np.maximum(b[p], 1e-300)).max()}"
            worst = max(worst, float((err / np.maximum(b[p], 1e-300)).max()))
    assert np.abs(orc.sums(False)[0]).max() > 0
    return worst


def _bits(arrow):
    import torch
    t = arrow.B.result_tile()
    return t.contiguous().view(torch.uint8).cpu().numpy().copy()


def check_scaled_step(mode_kwargs, decomp, orc, precision, device, exact_bits):
    """scale_operator with power-of-two factors, then step(), against an
    engine loaded from the host-scaled decomposition (the scaling is exact in
    every precision, so both hold the same values)."""
    n = orc.perm0.size
    rng = np.random.default_rng(1007)
    r = 2.0 ** rng.integers(-2, 3, n)       # original order
    c = 2.0 ** rng.integers(-2, 3, n)
    a = load(decomp, precision, device, **mode_kwargs)
    a.scale_operator(r[orc.perm0], c[orc.perm0])
    from scipy import sparse
    scaled = [((sparse.diags(r[p]) @ B.astype(np.float64) @ sparse.diags(c[p]))
               .astype(np.float32).tocsr(), p) for B, p in decomp]
    for (B, _), (S, _) in zip(decomp, scaled):
        assert S.nnz == B.nnz
    b = load(scaled, precision, device, **mode_kwargs)
    k = mode_kwargs['k']
    np_dt = np.float64 if precision == 'float64' else np.float32
    X = (2 * rng.random((n, k)) - 1).astype(np_dt)
    for arrow in (a, b):
        arrow.B.set_features(X[orc.perm0].copy())
        arrow.step()
    if exact_bits:
        assert (_bits(a) == _bits(b)).all(), \
            "step on the device-scaled operator differs from the step on " \
            "the host-scaled one"
        return 0.0
    # split rows: their atomics land in any order, so the two runs agree as
    # two evaluations of the same step do, each within the engine drivers'
    # bound of the float64 golden (engine_affine_driver.step_bound at
    # alpha 1, gamma 0)
    from scipy import sparse as sp
    A = (sp.diags(r) @ orc.A @ sp.diags(c)).tocsr()
    n_row = np.diff(A.indptr).astype(np.float64)
    u = 2.0 ** -53 if precision == 'float64' else 2.0 ** -24
    s = a.decomposition_length + 1 if precision == 'bfloat16' else 0
    factor = s * 2.0 ** -8 + (2.0 * n_row + 2.0 * a.decomposition_length
                              + 8.0) * u
    X64 = ead.held(a.B.feature_tile(), orc.perm0)
    G = np.asarray(A @ X64)[orc.perm0]
    bound = (factor[:, None] * np.asarray(abs(A) @ np.abs(X64)))[orc.perm0]
    worst = 0.0
    for arrow in (a, b):
        err = np.abs(arrow.B.allgather_result().astype(np.float64) - G)
        assert (err <= bound).all(), f"scaled step: max err {err.max()}"
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


def check_normalize(mode_kwargs, decomp, orc, precision, device):
    """'row', 'col' and 'sym' with absolute=True, each on a fresh engine."""
    p = orc.perm0
    tag = PREC_TAG[precision]
    abs_r, abs_c = orc.sums(True)
    out = {}
    for kind in ('row', 'col', 'sym'):
        arrow = load(decomp, precision, device, **mode_kwargs)
        rs, cs = arrow.normalize_operator(kind, absolute=True)
        got_r, got_c = arrow.operator_sums(absolute=True)
        if kind in ('row', 'col'):
            got, n, before, applied, other = (
                (got_r, orc.n_row, abs_r, rs, cs) if kind == 'row'
                else (got_c, orc.n_col, abs_c, cs, rs))
            assert other is None
            zero = before[p] == 0
            assert (got[zero] == 0).all() and (applied[zero] == 0).all()
            err = np.abs(got[~zero] - 1.0)
            bound = ss.normalised_bound(tag, n[p][~zero])
            assert (~zero).any() and (err <= bound).all(), \
                f"{kind}: max |sum - 1| {err.max()}, max err/bound " \
                f"{(err / bound).max()}"
            out[kind] = float((err / bound).max())
        else:
            from scipy import sparse
            dr = np.where(abs_r > 0, 1 / np.sqrt(np.where(abs_r > 0, abs_r, 1)), 0)
            dc = np.where(abs_c > 0, 1 / np.sqrt(np.where(abs_c > 0, abs_c, 1)), 0)
            S = np.asarray((sparse.diags(dr) @ orc.absA @ sparse.diags(dc))
                           .sum(axis=1)).ravel()
            bound = (ss.U[tag] + (2 * orc.n_row + orc.n_col.max() + 8)
                     * 2.0 ** -53) * S
            err = np.abs(got_r - S[p])
            assert (err <= bound[p]).all(), \
                f"sym: max err {err.max()}, max err/bound " \
                f"{(err / np.maximum(bound[p], 1e-300)).max()}"
            assert (got_r[abs_r[p] == 0] == 0).all()
            out[kind] = float((err / np.maximum(bound[p], 1e-300)).max())
    # a signed operator has rows of negative sum: 'sym' names one
    arrow = load(decomp, precision, device, **mode_kwargs)
    try:
        arrow.normalize_operator('sym')
        raise AssertionError("'sym' accepted a negative sum")
    except ValueError as e:
        assert 'absolute=True' in str(e) and 'negative' in str(e), str(e)
    return out


def run_iterate(decomp, orc, precision, device, mode_kwargs, tol=None):
    """iterate() with damping 0.5 after normalize_operator('row',
    absolute=True) on the RAW decomposition: no host scaling anywhere. tol
    defaults to the precision's ITER_TOL."""
    tol = end.ITER_TOL[precision] if tol is None else tol
    arrow = load(decomp, precision, device, **mode_kwargs)
    arrow.normalize_operator('row', absolute=True)
    rng = np.random.default_rng(7)
    np_dt = np.float64 if precision == 'float64' else np.float32
    X = (2 * rng.random((orc.perm0.size, mode_kwargs['k'])) - 1).astype(np_dt)
    arrow.B.set_features(X[orc.perm0].copy())
    arrow.set_affine_step(end.DAMPING, 1.0 - end.DAMPING, X[orc.perm0].copy())
    return arrow.iterate(end.ITER_MAX, tol=tol)


def assert_layout(mode, arrow, device):
    """The layout the environment asked for is the one that was built."""
    eng0 = arrow.engines[0]
    if mode in ('fold0',):
        assert arrow._folded is None
    elif mode == 'fold1':
        assert arrow._folded is not None and arrow._fold_cols
    elif mode == 'fold2':
        assert arrow._folded is not None and not arrow._fold_cols
    if device != 'gpu':
        return
    if mode in ('default', 'hub'):
        assert eng0._A_all is not None
    elif mode in ('fuse_all0', 'banded'):
        assert eng0._A_all is None and eng0._A_row0 and eng0._A_rest
        assert eng0.banded == (mode == 'banded')


def run_mode(mode, device, precision):
    _, kwargs = MODES[mode]
    decomp = make_decomp(**kwargs)
    orc = Oracle(decomp)
    arrow = load(decomp, precision, device, **kwargs)
    assert_layout(mode, arrow, device)
    info = dict(sums=check_sums(arrow, orc))
    info['scaled_step'] = check_scaled_step(kwargs, decomp, orc, precision,
                                            device, exact_bits=mode != 'hub')
    info.update(check_normalize(kwargs, decomp, orc, precision, device))
    if mode != 'hub':
        steps, rel = run_iterate(decomp, orc, precision, device, kwargs)
        assert steps < end.ITER_MAX and rel <= end.ITER_TOL[precision], \
            f"iterate: {steps} steps, rel {rel}"
        if device == 'gpu':
            # the cpu device has no bf16 features: its float32 run, at the
            # tolerance of the gpu run
            cpu_prec = 'float32' if precision == 'bfloat16' else precision
            cpu_steps, _ = run_iterate(decomp, orc, cpu_prec, 'cpu', kwargs,
                                       tol=end.ITER_TOL[precision])
            assert abs(steps - cpu_steps) <= 1, \
                f"iterate: {steps} steps on the gpu, {cpu_steps} on the cpu"
            info['cpu_steps'] = cpu_steps
        info.update(steps=steps, rel=rel)
    return info


def main(argv):
    mode, device = argv[1], argv[2]
    ch.started_with(ENGINE_VARS, MODES[mode][0])
    if device == 'gpu':
        ch.open_gpu("the scale engine driver needs a GPU", set_device=False)
    return ch.run_jobs([(p, lambda p=p: run_mode(mode, device, p))
                        for p in PRECISIONS[device]],
                       {'mode': mode, 'device': device})


if __name__ == '__main__':
    sys.exit(main(sys.argv))
