"""The affine-step engine run shared by test_gpu_affine_engine.py, and its child
entry point: `python tests/engine_affine_driver.py <mode>` runs one entry of
MODES, in float32, float64 and bfloat16 features, in a process whose
environment selects the engine layout (ARROW_FUSE_ALL / ARROW_FOLD are read
when the structures are built), and prints one JSON line per precision
through the job loop of tests/child_harness.py. This is a plain module, not a
test file.

Step check. Three steps of X <- 0.85 A@X + 0.15 R; after each the golden is
the float64 evaluation on the recomposed matrix of the engine's OWN previous
output (read back exactly), so rounding does not compound. Per element

    |C - G| <= (s 2**-8 + (2 n_row + 2 L + 8) u) (|alpha| |A|@|X| + |gamma||R|)

with n_row the row's nonzero count in the recomposed matrix, L the number of
parts and u = 2**-24 (float64: 2**-53): one rounding per product and per add
of the chain, one add per part that is accumulated, the roundings of
alpha * sum, gamma * r and their add, all doubled so that it holds with fma
or without. s counts the roundings to bf16 storage and is 0 for float32 and
float64; for bfloat16 features s = L + 1: each part's launch rounds its
contribution (or the running sum it adds to) once, and the layouts that
finish with the tail kernel round once more. Derived, not measured.
"""
import os
import sys
import tempfile

import numpy as np

if not __package__:         # started as a script: see tests/child_harness.py
    import child_harness  # noqa: F401
from tests import child_harness as ch  # noqa: E402

from tests.gpu_children import ENGINE_VARS  # noqa: E402

ALPHA, GAMMA = 0.85, 0.15
L1 = dict(n_blocks=[3], width=64, k=32, seed=0)
L2 = dict(n_blocks=[4, 2], width=50, k=8, seed=1)
# two hub rows of 8000 draws over 2560 columns: about 2450 distinct nonzeros
# each, above the 2048 of one work item: split rows in the fused structure
HUB = dict(n_blocks=[5], width=512, k=8, seed=5, hub_rows=2, hub_deg=8000)
BANDED = dict(n_blocks=[4], width=32, k=16, seed=53, block_diagonal=False,
              slim=False)
# mode -> (variables, run arguments, the affine step rides in the launches)
MODES = {
    'fuse_all0': ({'ARROW_FUSE_ALL': '0'}, L1, False),   # two launches + tail
    'fold0': ({'ARROW_FOLD': '0'}, L2, False),           # sequential + tail
    'fold1': ({'ARROW_FOLD': '1'}, L2, True),            # full fold
    'fold2': ({'ARROW_FOLD': '2'}, L2, True),            # row fold
    'banded': ({'ARROW_FUSE_ALL': '0'}, BANDED, False),  # banded ArrowMPI
}
PRECISIONS = ('float32', 'float64', 'bfloat16')


def dtype_of(name):
    import torch
    return {'float32': np.float32, 'float64': np.float64,
            'bfloat16': torch.bfloat16}[name]


def step_bound(A, absA, X, R, L, precision):
    """(golden, bound) of one affine step from the float64 features X and
    residual R (original row order)."""
    n_row = np.diff(A.indptr).astype(np.float64)
    u = 2.0 ** -53 if precision == 'float64' else 2.0 ** -24
    s = L + 1 if precision == 'bfloat16' else 0
    factor = s * 2.0 ** -8 + (2.0 * n_row + 2.0 * L + 8.0) * u
    mag = ALPHA * np.asarray(absA @ np.abs(X)) + GAMMA * np.abs(R)
    return ALPHA * np.asarray(A @ X) + GAMMA * R, factor[:, None] * mag


def build(n_blocks, width, k, seed, precision, hub_rows=0, hub_deg=None,
          block_diagonal=True, slim=True):
    """save -> load_decomposition_new -> initialize -> zero_rhs on the GPU.
    Returns (arrow, A, perm0, X, R): the recomposed float64 matrix, part 0's
    permutation and fp32 features and residual in original row order (for
    bf16 the engine rounds them once)."""
    from arrow_matrix_amd import graphio, synth
    from arrow_matrix_amd.arrow_dec import ArrowDecompositionMPI
    dtype = dtype_of(precision)
    decomp = synth.synth_arrow_decomposition(
        width, n_blocks, avg_deg=6, seed=seed, hub_rows=hub_rows,
        hub_deg=hub_deg, block_diagonal=block_diagonal, dtype=np.float32)
    n = n_blocks[0] * width
    with tempfile.TemporaryDirectory() as td:
        prefix = os.path.join(td, 'g')
        graphio.save_decomposition_new(decomp, prefix, width,
                                       block_diagonal=block_diagonal)
        blocks, nb, tp, tn = ArrowDecompositionMPI.load_decomposition_new(
            None, prefix, width, is_block_diagonal=block_diagonal,
            datatype=dtype)
        arrow = ArrowDecompositionMPI.initialize(
            None, nb, tp, tn, width, k, device='gpu',
            block_diagonal=block_diagonal, slim=slim, dtype=dtype)
        arrow.load_data_from_blocks(blocks)
        arrow.zero_rhs(width, k, dtype=dtype)
    # recomposed in float64: where parts overlap the engine adds their
    # contributions in its own precision, it never forms an fp32 sum of A's
    A = synth.recompose([(B.astype(np.float64), p) for B, p in decomp]).tocsr()
    rng = np.random.default_rng(seed)
    np_dt = np.float64 if precision == 'float64' else np.float32
    X = (2 * rng.random((n, k)) - 1).astype(np_dt)
    R = (2 * rng.random((n, k)) - 1).astype(np_dt)
    return arrow, A, decomp[0][1], X, R


def held(tensor, perm0):
    """A device stripe in part-0 order, as float64 in original row order."""
    import torch
    out = np.empty(tuple(tensor.shape))
    out[perm0] = tensor.to(torch.float64).cpu().numpy()
    return out


def run_steps(arrow, A, perm0, precision, iters=3):
    """Iterate X := C with the affine step set; per step (max err / bound,
    max |G|). Raises AssertionError outside the bound."""
    L = arrow.decomposition_length
    absA = abs(A)
    R = held(arrow.engines[0]._R, perm0)     # as the engine holds it
    out = []
    for step in range(iters):
        Xin = held(arrow.B.feature_tile(), perm0)
        arrow.step()
        C = arrow.B.allgather_result().astype(np.float64)
        G, bound = step_bound(A, absA, Xin, R, L, precision)
        err = np.abs(C - G[perm0])
        worst = float((err / np.maximum(bound[perm0], 1e-300)).max())
        print(f"# {precision} step {step}: max err/bound {worst:.3f}, "
              f"max |G| {float(np.abs(G).max()):.3f}", file=sys.stderr)
        assert np.isfinite(C).all()
        assert (err <= bound[perm0]).all(), \
            f"{precision} step {step}: max err/bound {worst}"
        assert np.abs(G).max() > 0
        out.append((worst, float(np.abs(G).max())))
        arrow.B.set_features(arrow.B.result_tile())
    return out


class TailCounter:
    """Counts backend.axpby_rows calls of an engine (a wrapper, in place)."""

    def __init__(self, backend):
        self.calls = 0
        inner = backend.axpby_rows

        def counted(*args, **kwargs):
            self.calls += 1
            return inner(*args, **kwargs)
        backend.axpby_rows = counted


def run(precision, **kwargs):
    """Build, set the affine step, run three checked steps. Returns (arrow,
    tail-kernel calls, per-step figures)."""
    arrow, A, perm0, X, R = build(precision=precision, **kwargs)
    tails = TailCounter(arrow.engines[0].backend)
    arrow.B.set_features(X[perm0].copy())
    arrow.set_affine_step(ALPHA, GAMMA, R[perm0].copy())
    figures = run_steps(arrow, A, perm0, precision)
    return arrow, tails.calls, figures


def run_mode(mode, precision):
    """One precision of one entry of MODES; returns the line's figures."""
    _, kwargs, inside = MODES[mode]
    arrow, tails, figures = run(precision, **kwargs)
    eng0 = arrow.engines[0]
    # the path the environment asked for is the path that ran
    if mode in ('fuse_all0', 'banded'):
        assert eng0._A_all is None and eng0._A_row0 and eng0._A_rest
        assert eng0.banded == (mode == 'banded')
    elif mode == 'fold0':
        assert arrow._folded is None
    elif mode == 'fold1':
        assert arrow._folded is not None and arrow._fold_cols
    elif mode == 'fold2':
        assert arrow._folded is not None and not arrow._fold_cols
    # fused layouts never call the tail kernel; the others once a step
    assert tails == (0 if inside else 3), f"{tails} tail calls"
    return dict(tails=tails, max_err_over_bound=max(f[0] for f in figures))


def main(argv):
    mode = argv[1]
    ch.started_with(ENGINE_VARS, MODES[mode][0])
    ch.open_gpu("the affine engine driver needs a GPU", set_device=False)
    return ch.run_jobs([(p, lambda p=p: run_mode(mode, p))
                        for p in PRECISIONS], {'mode': mode})


if __name__ == '__main__':
    sys.exit(main(sys.argv))
