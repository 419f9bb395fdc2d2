"""The bfloat16-feature engine run shared by test_gpu_bf16_engine.py, and its
child entry point: `python tests/engine_bf16_driver.py <mode> <out.npy>` runs
one entry of MODES in a process whose environment selects the engine path
(ARROW_FUSE_ALL / ARROW_FOLD are read when the structures are built) and
saves, per step, the result, the golden and the bound. This is a plain
module, not a test file.

Step check. The engine's features are bf16, so after each step the golden is
recomputed from the engine's OWN previous output (read back exactly, bf16 ->
float64): rounding does not compound across steps. Per element

    |C - A@X| <= (L 2**-8 + (n_row + L + 2) 2**-24) (|A| @ |X|)

with A the recomposed matrix (fp32 values, as resident), n_row its row's
nonzero count and L the number of decomposition parts: one round-to-nearest
to bf16 (unit roundoff 2**-8) per part's contribution — each part's product
is rounded once by its launch, and the running sum once per part that is
added to it — plus the fp32 fma chain of n_row terms and the L + 2 fp32 adds
around it. Derived, not measured.
"""
import os
import sys
import tempfile

import numpy as np

if not __package__:         # started as a script: see tests/child_harness.py
    import child_harness  # noqa: F401
from tests import child_harness as ch  # noqa: E402

from tests.gpu_children import ENGINE_VARS  # noqa: E402

L1 = dict(n_blocks=[4], width=64, k=16, seed=31, iters=3)
L2 = dict(n_blocks=[4, 2], width=50, k=8, seed=41, iters=3)
# mode -> (variables, run_bf16 arguments)
MODES = {
    'fuse_all0': ({'ARROW_FUSE_ALL': '0'}, L1),     # the two-launch layout
    'fold0': ({'ARROW_FOLD': '0'}, L2),             # L = 2 sequential
    'fold1': ({'ARROW_FOLD': '1'}, L2),             # full fold
    'fold2': ({'ARROW_FOLD': '2'}, L2),             # row fold
}


def make_decomposition(n_blocks, width, seed, hub_rows=0, hub_deg=None,
                       avg_deg=6):
    from arrow_matrix_amd import synth
    return synth.synth_arrow_decomposition(
        width, n_blocks, avg_deg=avg_deg, seed=seed, hub_rows=hub_rows,
        hub_deg=hub_deg, dtype=np.float32)


def step_bound(A, absA, X, L):
    """(golden, bound) of one step from the float64 features X (original
    row order)."""
    n_row = np.diff(A.indptr).astype(np.float64)
    factor = L * 2.0 ** -8 + (n_row + L + 2.0) * 2.0 ** -24
    return np.asarray(A @ X), factor[:, None] * np.asarray(absA @ np.abs(X))


def run_engine(n_blocks, width, k, seed, dtype, iters=3, hub_rows=0,
               hub_deg=None, avg_deg=6):
    """save -> load_decomposition_new(datatype=dtype) -> initialize(dtype) ->
    zero_rhs(dtype) -> iterate X := C. Returns (results, goldens, bounds,
    arrow) per step in part-0 order; every golden is the float64 product of
    the recomposed matrix with the features the engine held BEFORE the
    step."""
    import torch
    from arrow_matrix_amd import graphio, synth
    from arrow_matrix_amd.arrow_dec import ArrowDecompositionMPI

    decomp = make_decomposition(n_blocks, width, seed, hub_rows, hub_deg,
                                avg_deg)
    n = n_blocks[0] * width
    L = len(n_blocks)
    rng = np.random.default_rng(seed)
    X = (2 * rng.random((n, k)) - 1).astype(np.float32)
    with tempfile.TemporaryDirectory() as td:
        prefix = os.path.join(td, 'g')
        graphio.save_decomposition_new(decomp, prefix, width,
                                       block_diagonal=True)
        blocks, nb, tp, tn = ArrowDecompositionMPI.load_decomposition_new(
            None, prefix, width, is_block_diagonal=True, datatype=dtype)
        np.testing.assert_array_equal(nb, n_blocks)
        arrow = ArrowDecompositionMPI.initialize(
            None, nb, tp, tn, width, k, device='gpu', dtype=dtype)
        arrow.load_data_from_blocks(blocks)
        arrow.zero_rhs(width, k, dtype=dtype)
    perm0 = decomp[0][1]
    A = synth.recompose(decomp).astype(np.float64).tocsr()
    absA = abs(A)
    arrow.B.set_features(X[perm0].copy())         # numpy float32
    results, goldens, bounds = [], [], []
    for _ in range(iters):
        held = arrow.B.feature_tile()
        assert isinstance(held, torch.Tensor)
        Xin = np.empty((n, k))
        Xin[perm0] = held.to(torch.float64).cpu().numpy()
        arrow.step()
        C = arrow.B.allgather_result()
        G, bound = step_bound(A, absA, Xin, L)
        results.append(C.copy())
        goldens.append(G[perm0])
        bounds.append(bound[perm0])
        arrow.B.set_features(arrow.B.result_tile())
    return results, goldens, bounds, arrow


def run_bf16(**kwargs):
    import torch
    results, goldens, bounds, arrow = run_engine(dtype=torch.bfloat16,
                                                 **kwargs)
    for C in results:
        assert C.dtype == np.float32          # the exact upcast of bf16
    return results, goldens, bounds, arrow


def main(argv):
    mode, out = argv[1], argv[2]
    variables, kwargs = MODES[mode]
    ch.started_with(ENGINE_VARS, variables)
    ch.open_gpu("the bfloat16 engine driver needs a GPU", set_device=False)
    results, goldens, bounds, arrow = run_bf16(**kwargs)
    eng0 = arrow.engines[0]
    # the path the environment asked for is the path that ran
    if mode == 'fuse_all0':
        assert eng0._A_all is None and eng0._A_row0 and eng0._A_rest
    elif mode == 'fold0':
        assert arrow._folded is None
    elif mode == 'fold1':
        assert arrow._folded is not None and arrow._fold_cols
    elif mode == 'fold2':
        assert arrow._folded is not None and not arrow._fold_cols
    np.save(out, np.stack([np.stack(results).astype(np.float64),
                           np.stack(goldens), np.stack(bounds)]))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
