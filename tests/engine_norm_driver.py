"""The tracked engine run shared by test_gpu_norm_engine.py, and its child
entry point: `python tests/engine_norm_driver.py <mode>` runs one entry of
MODES with and without an affine step, in float32, float64 and bfloat16
features, in a process whose environment selects the engine layout, and
prints one JSON line per (precision, affine). Built on
tests/engine_affine_driver.py and the job loop of tests/child_harness.py. This
is a plain module, not a test file.

Per step: the tracked engine's result equals an untracked engine's bit for
bit; the two accumulators are compared with the host's float64 sums over the
stripes as read back (the result, and the features before the step), to
spmm_cases_norm.norm_bound; last_step_norms() is the square roots of the
accumulators; and the backend's counters say which entry point measured.
"""
import math
import os
import sys
import tempfile

import numpy as np

if not __package__:         # started as a script: see tests/child_harness.py
    import child_harness  # noqa: F401
from tests import child_harness as ch  # noqa: E402

from tests import engine_affine_driver as ead  # noqa: E402
from tests import spmm_cases_norm as sn  # noqa: E402
from tests.gpu_children import ENGINE_VARS  # noqa: E402

PRECISIONS = ead.PRECISIONS
PREC_TAG = {'float32': 'f32', 'float64': 'f64', 'bfloat16': 'bf16'}
STEPS = 2
# mode -> (variables, run arguments, fused: the launch itself measures)
MODES = {
    'default': ({}, ead.L1, True),
    'fuse_all0': ({'ARROW_FUSE_ALL': '0'}, ead.L1, False),
    'fold0': ({'ARROW_FOLD': '0'}, ead.L2, False),
    'fold1': ({'ARROW_FOLD': '1'}, ead.L2, False),
    'fold2': ({'ARROW_FOLD': '2'}, ead.L2, False),
}


def _acc(arrow):
    acc = arrow._norm_acc if arrow.decomposition_length > 1 \
        else arrow.engines[0]._norm_acc
    return acc.cpu().tolist()


def run_tracked(precision, affine, **kwargs):
    """STEPS checked steps of a tracked engine next to an untracked one.
    Returns (tracked arrow, worst err / bound)."""
    import torch
    a, A, perm0, X, R = ead.build(precision=precision, **kwargs)
    b, *_ = ead.build(precision=precision, **kwargs)
    for arrow in (a, b):
        arrow.B.set_features(X[perm0].copy())
        if affine:
            arrow.set_affine_step(ead.ALPHA, ead.GAMMA, R[perm0].copy())
    a.track_step_norms()
    be = a.engines[0].backend
    worst = 0.0
    for step in range(STEPS):
        x64 = a.B.feature_tile().to(torch.float64).cpu().numpy()
        a.step()
        b.step()
        Ca, Cb = a.B.result_tile(), b.B.result_tile()
        assert torch.equal(Ca.view(torch.uint8), Cb.view(torch.uint8)), \
            f"step {step}: tracking changed the result"
        c64 = Ca.to(torch.float64).cpu().numpy()
        assert np.isfinite(c64).all() and np.abs(c64).max() > 0
        acc = _acc(a)
        s0, s1 = sn.host_sums(c64, x64)
        b0, b1 = sn.norm_bound(PREC_TAG[precision], c64.size, s0, s1)
        e0, e1 = abs(acc[0] - s0), abs(acc[1] - s1)
        print(f"# {precision} affine={affine} step {step}: acc {acc}, host "
              f"{[s0, s1]}, err {[e0, e1]}, bound {[b0, b1]}",
              file=sys.stderr)
        assert e0 <= b0 and e1 <= b1, \
            f"step {step}: acc {acc} host {[s0, s1]} bound {[b0, b1]}"
        assert a.last_step_norms() == (math.sqrt(acc[0]), math.sqrt(acc[1]))
        worst = max(worst, e0 / b0, e1 / b1)
        for arrow in (a, b):
            arrow.B.set_features(arrow.B.result_tile())
    return a, be.norm_launches, be.diffnorm_launches, worst


def check_counters(fused, norm_launches, diffnorm_launches):
    """The fused layout measures in its own launch and never runs the
    stand-alone pass; every other layout the reverse, once a step."""
    want = (STEPS, 0) if fused else (0, STEPS)
    assert (norm_launches, diffnorm_launches) == want, \
        f"(fused launches, stand-alone passes) = " \
        f"{(norm_launches, diffnorm_launches)}, expected {want}"


# ---------------------------------------------------------------------------
# iterate() on a contraction
# ---------------------------------------------------------------------------

DAMPING = 0.5
ITER_SHAPE = dict(n_blocks=[3], width=64, k=8, seed=0)
# float32 / float64: rel falls by about the damping per step from O(1), far
# below max_steps; bfloat16 features cannot resolve steps below their own
# spacing 2**-8, so its tolerance stays above it
ITER_TOL = {'float32': 1e-3, 'float64': 1e-3, 'bfloat16': 2.0 ** -5}
ITER_MAX = 40


def build_scaled(precision, device):
    """ead.build on a matrix scaled so that its maximum absolute row sum is
    <= 1 (damping 0.5 then makes the step a contraction), on `device`.
    Returns (arrow, perm0, X)."""
    from arrow_matrix_amd import graphio, synth
    from arrow_matrix_amd.arrow_dec import ArrowDecompositionMPI
    s = ITER_SHAPE
    dtype = ead.dtype_of(precision)
    decomp = synth.synth_arrow_decomposition(
        s['width'], s['n_blocks'], avg_deg=6, seed=s['seed'],
        dtype=np.float32)
    A = synth.recompose([(B.astype(np.float64), p) for B, p in decomp])
    scale = np.float32(1.0 / (1.001 * abs(A).sum(axis=1).max()))
    decomp = [((B * scale).astype(np.float32), p) for B, p in decomp]
    with tempfile.TemporaryDirectory() as td:
        prefix = os.path.join(td, 'g')
        graphio.save_decomposition_new(decomp, prefix, s['width'],
                                       block_diagonal=True)
        blocks, nb, tp, tn = ArrowDecompositionMPI.load_decomposition_new(
            None, prefix, s['width'], is_block_diagonal=True, datatype=dtype)
        arrow = ArrowDecompositionMPI.initialize(
            None, nb, tp, tn, s['width'], s['k'], device=device,
            block_diagonal=True, slim=True, dtype=dtype)
        arrow.load_data_from_blocks(blocks)
        arrow.zero_rhs(s['width'], s['k'], dtype=dtype)
    rng = np.random.default_rng(7)
    np_dt = np.float64 if precision == 'float64' else np.float32
    X = (2 * rng.random((s['n_blocks'][0] * s['width'], s['k'])) - 1) \
        .astype(np_dt)
    return arrow, decomp[0][1], X


def run_iterate(precision, device):
    arrow, perm0, X = build_scaled(precision, device)
    arrow.B.set_features(X[perm0].copy())
    arrow.set_affine_step(DAMPING, 1.0 - DAMPING, X[perm0].copy())
    return arrow.iterate(ITER_MAX, tol=ITER_TOL[precision])


def run_mode(mode, precision, affine):
    """One (precision, affine) of one entry of MODES; returns the line's
    figures."""
    _, kwargs, fused = MODES[mode]
    arrow, n_fused, n_alone, worst = run_tracked(precision, affine, **kwargs)
    eng0 = arrow.engines[0]
    # the path the environment asked for is the path that ran
    if mode == 'default':
        assert eng0._A_all is not None
    elif mode == 'fuse_all0':
        assert eng0._A_all is None and eng0._A_row0
    elif mode == 'fold0':
        assert arrow._folded is None
    elif mode == 'fold1':
        assert arrow._folded is not None and arrow._fold_cols
    elif mode == 'fold2':
        assert arrow._folded is not None and not arrow._fold_cols
    check_counters(fused, n_fused, n_alone)
    return dict(fused_launches=n_fused, stand_alone=n_alone,
                max_err_over_bound=worst)


def main(argv):
    mode = argv[1]
    ch.started_with(ENGINE_VARS, MODES[mode][0])
    ch.open_gpu("the norm engine driver needs a GPU", set_device=False)
    return ch.run_jobs(
        [(f'{p}_affine{int(a)}', lambda p=p, a=a: run_mode(mode, p, a))
         for p in PRECISIONS for a in (False, True)], {'mode': mode})


if __name__ == '__main__':
    sys.exit(main(sys.argv))
