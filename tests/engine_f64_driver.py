"""The float64 engine run shared by test_gpu_f64_engine.py, and its child
entry point: `python tests/engine_f64_driver.py <mode> <out.npy>` runs one
entry of MODES in a process whose environment selects the engine path
(ARROW_FUSE_ALL / ARROW_FOLD are read when the structures are built) and
saves the per-iteration results. This is a plain module, not a test file.
"""
import os
import sys
import tempfile

import numpy as np

if not __package__:         # started as a script: see tests/child_harness.py
    import child_harness  # noqa: F401
from tests import child_harness as ch  # noqa: E402

from tests.gpu_children import ENGINE_VARS  # noqa: E402

# mode -> (variables, run_f64 arguments). 'default' is what the parent
# computes in-process with none of ENGINE_VARS set.
L1 = dict(n_blocks=[4], width=64, k=16, seed=31, iters=3)
L2 = dict(n_blocks=[4, 2], width=50, k=8, seed=41, iters=3)
BANDED = dict(n_blocks=[4], width=32, k=16, seed=53, iters=3,
              block_diagonal=False, slim=False)
MODES = {
    'fuse_all0': ({'ARROW_FUSE_ALL': '0'}, L1),
    'allreduce_x0': ({'ARROW_FUSE_ALL': '0'}, dict(L1, allreduce_x0=True)),
    'fold0': ({'ARROW_FOLD': '0'}, L2),
    'fold1': ({'ARROW_FOLD': '1'}, L2),
    'fold2': ({'ARROW_FOLD': '2'}, L2),
    'banded': ({}, BANDED),
}
DEFAULT_OF = {'fuse_all0': L1, 'allreduce_x0': L1, 'fold0': L2, 'fold1': L2,
              'fold2': L2}


def make_decomposition(n_blocks, width, seed, block_diagonal=True,
                       hub_rows=0, hub_deg=None, avg_deg=6):
    """The float64 synthetic decomposition run_f64 multiplies with (a pure
    function of its arguments). hub_deg entries are drawn with replacement
    and merged, so a hub row holds fewer distinct nonzeros than hub_deg."""
    from arrow_matrix_amd import synth
    return synth.synth_arrow_decomposition(
        width, n_blocks, avg_deg=avg_deg, seed=seed,
        block_diagonal=block_diagonal, hub_rows=hub_rows, hub_deg=hub_deg,
        dtype=np.float64)


def run_f64(n_blocks, width, k, seed, iters=1, device='gpu',
            block_diagonal=True, slim=True, allreduce_x0=False,
            hub_rows=0, hub_deg=None, avg_deg=6):
    """save -> load_decomposition_new(datatype=float64) ->
    initialize(dtype=float64) -> zero_rhs(dtype=float64) -> iterate.
    Returns (results, goldens) per iteration in part-0 order; the golden is
    synth.recompose(decomp).astype(float64) @ X."""
    from arrow_matrix_amd import graphio, synth
    from arrow_matrix_amd.arrow_dec import ArrowDecompositionMPI

    decomp = make_decomposition(n_blocks, width, seed, block_diagonal,
                                hub_rows, hub_deg, avg_deg)
    n = n_blocks[0] * width
    rng = np.random.default_rng(seed)
    X = 2 * rng.random((n, k)) - 1          # float64
    with tempfile.TemporaryDirectory() as td:
        prefix = os.path.join(td, 'g')
        graphio.save_decomposition_new(decomp, prefix, width,
                                       block_diagonal=block_diagonal)
        blocks, nb, tp, tn = ArrowDecompositionMPI.load_decomposition_new(
            None, prefix, width, is_block_diagonal=block_diagonal,
            datatype=np.float64)
        np.testing.assert_array_equal(nb, n_blocks)
        arrow = ArrowDecompositionMPI.initialize(
            None, nb, tp, tn, width, k, device=device,
            block_diagonal=block_diagonal, slim=slim, dtype=np.float64)
        arrow.load_data_from_blocks(blocks)
        arrow.zero_rhs(width, k, dtype=np.float64)
        if allreduce_x0:
            for eng in arrow.engines:
                eng.allreduce_x0 = True
        perm0 = decomp[0][1]
        A = synth.recompose(decomp).astype(np.float64)
        arrow.B.set_features(X[perm0].copy())
        results, goldens = [], []
        gX = X
        for _ in range(iters):
            arrow.step()
            C = arrow.B.allgather_result()
            assert C.dtype == np.float64
            results.append(C.copy())
            gX = A @ gX
            goldens.append(gX[perm0])
            arrow.B.set_features(arrow.B.result_tile())
        return results, goldens, arrow


def main(argv):
    mode, out = argv[1], argv[2]
    variables, kwargs = MODES[mode]
    ch.started_with(ENGINE_VARS, variables)
    ch.open_gpu("the float64 engine driver needs a GPU", set_device=False)
    results, goldens, _ = run_f64(**kwargs)
    np.save(out, np.stack([np.stack(results), np.stack(goldens)]))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
