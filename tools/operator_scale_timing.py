"""Time the operator passes of ABI 1007 on the fused single-launch structure
of bench.py's synthetic matrix, beside one plain SpMM step on the same
structure, in one session (HIP events around each call, a warm-up first,
float32):

    sums    arrow_csr_sums, row and column sums (row_sum, col_sum0 ==
            col_sum1 == one vector, as the engine calls it)
    rowsum  arrow_csr_sums, row sums only (no per-nonzero atomics)
    scale   arrow_csr_scale with row and column factors (all 1.0, so the
            values stay what they are and every repetition does the same work)
    step    arrow.step(), the plain X <- A@X launch
    and the wall time of engine.operator_sums() and engine.scale_operator(),
    host side of the O(n) vectors included.

Expectation (not a threshold): one streaming pass, 8 B/nnz read, + 8 B/nnz
written for scale, + 12 B per item, + an 8-byte gather (scale) or float64
atomic (sums) per nonzero.

Prints one JSON line. Recorded, not gated.

Usage: python tools/operator_scale_timing.py [--rows 20000000] [--k 128]
                                             [--reps 10] [--json-out F]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools.affine_fused_vs_unfused import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=20_000_000)
    ap.add_argument('--n-blocks', type=int, default=8)
    ap.add_argument('--band', type=int, default=1024)
    ap.add_argument('--k', type=int, default=128)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--json-out', type=str, default=None)
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "needs a HIP GPU"
    torch.cuda.set_device(0)
    import bench
    from arrow_matrix_amd.arrow_dec import ArrowDecompositionMPI
    from arrow_matrix_amd.comm import Comm

    nb, k = args.n_blocks, args.k
    w = args.rows // nb
    grids, _, _ = bench.build_blocks_for_rank(0, 1, w, nb, 1, 'cuda', args.band)
    arrow = ArrowDecompositionMPI.initialize(
        Comm(), np.array([nb]), [None], [None], w, k, device='gpu')
    arrow.load_data_from_blocks(grids)
    arrow.zero_rhs(w, k)
    eng = arrow.engines[0]
    be = eng.backend
    h = eng._A_all
    assert h is not None, "expected the fused single-launch layout"
    n = nb * w
    g = torch.Generator(device='cuda')
    g.manual_seed(42)
    eng.set_features(torch.rand(eng.X_i.shape, generator=g, device='cuda',
                                dtype=torch.float32) * 2 - 1)

    row = be.scale_vector(np.zeros(n))
    col = be.scale_vector(np.zeros(n))
    ones = be.scale_vector(np.ones(n))
    res = {}
    res['step'] = timed(arrow.step, args.reps, args.warmup)
    res['sums'] = timed(lambda: be.block_sums(h, row, col, col, True),
                        args.reps, args.warmup)
    res['rowsum'] = timed(lambda: be.block_sums(h, row, None, None, True),
                          args.reps, args.warmup)
    res['scale'] = timed(lambda: be.block_scale(h, ones, ones, ones),
                         args.reps, args.warmup)
    res['step_after'] = timed(arrow.step, args.reps, args.warmup)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return round(1e3 * (time.perf_counter() - t0), 3)
    wall_ms = dict(
        operator_sums=wall(lambda: arrow.operator_sums(absolute=True)),
        scale_operator=wall(lambda: arrow.scale_operator(np.ones(n),
                                                         np.ones(n))))
    col_sums = arrow.operator_sums(absolute=True)[1]

    nnz, items = h.nnz, n
    nbytes = dict(sums=8 * nnz + 12 * items, rowsum=8 * nnz + 12 * items,
                  scale=16 * nnz + 12 * items)

    def summary(key):
        ms = res[key]
        med = statistics.median(ms)
        out = dict(ms_median=round(med, 4), ms_best=round(min(ms), 4),
                   ms_all=[round(t, 4) for t in ms])
        if key in nbytes:
            out.update(stream_bytes=nbytes[key],
                       stream_tbs_median=round(
                           nbytes[key] / (med * 1e-3) / 1e12, 3))
        return out
    out = dict(
        # the name string as the runtime reports it: a label, not an identity
        runtime_device_name=torch.cuda.get_device_name(0),
        dtype='float32', k=k, rows=n, nnz=nnz,
        **{key: summary(key) for key in res}, wall_ms=wall_ms,
        hottest_column_sum_over_mean=round(
            float(col_sums.max() / max(col_sums.mean(), 1e-300)), 2),
        not_run=["float64 structures", "the two-launch and folded layouts",
                 "the parent commit in the same session: its plain step is "
                 "the 'step' kernel here, which this change does not touch"])
    line = json.dumps(out)
    print(line)
    if args.json_out:
        with open(args.json_out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
