"""Time the fused single-launch structure in float64 at k=64 against float32
at k=128 on bench.py's synthetic matrix (HIP events around the launch).

The two cases move the same X and C bytes per row (64 x 8 = 128 x 4); A is
12 B/nnz (split int32 cols + double vals) against 8 B/nnz (packed pairs).
Algorithmic bytes per launch (DESIGN.md roofline):

    (A bytes/nnz) * nnz + 4 * (rows + 1) + 2 * itemsize * k * rows

Prints one JSON line: ms/launch (median and best of --reps), the algorithmic
byte ratio f64/f32, the time ratio, and the achieved algorithmic TB/s of
both. Recorded, not gated.

Usage: python tools/f64_vs_f32.py [--rows 20000000] [--reps 20] [--json-out F]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

A_BYTES = {np.dtype(np.float32): 8, np.dtype(np.float64): 12}


def time_case(grids, w, nb, k, dtype, reps, warmup):
    import torch
    from arrow_matrix_amd import hip
    from arrow_matrix_amd.arrow_dec import ArrowDecompositionMPI
    from arrow_matrix_amd.comm import Comm

    dtype = np.dtype(dtype)
    arrow = ArrowDecompositionMPI.initialize(
        Comm(), np.array([nb]), [None], [None], w, k, device='gpu',
        dtype=dtype)
    arrow.load_data_from_blocks(grids)
    arrow.zero_rhs(w, k, dtype=dtype)
    eng = arrow.engines[0]
    assert eng._A_all is not None, "expected the fused single-launch layout"
    g = torch.Generator(device='cuda')
    g.manual_seed(42)
    X = torch.rand(eng.X_i.shape, generator=g, device='cuda',
                   dtype=eng.backend.torch_dtype) * 2 - 1
    eng.set_features(X)
    for _ in range(warmup):
        arrow.step()
        eng.set_features(eng.result_tile())
    torch.cuda.synchronize()
    eng.kernel_events = []
    for _ in range(reps):
        arrow.step()
        eng.set_features(eng.result_tile())
    torch.cuda.synchronize()
    ms = [s.elapsed_time(e) for s, e, *_ in eng.kernel_events]
    eng.kernel_events = None
    assert len(ms) == reps
    nnz, rows = eng._A_all.nnz, nb * w
    plan = hip.spmm_plan(k, nnz, -1, dtype=dtype)
    nbytes = A_BYTES[dtype] * nnz + 4 * (rows + 1) + 2 * dtype.itemsize * k * rows
    med = statistics.median(ms)
    out = dict(dtype=dtype.name, k=k, rows=rows, nnz=nnz, plan=plan,
               ms_median=round(med, 4), ms_best=round(min(ms), 4),
               ms_all=[round(t, 4) for t in ms], algorithmic_bytes=nbytes,
               tbs_median=round(nbytes / (med * 1e-3) / 1e12, 3),
               gflops_median=round(2.0 * nnz * k / (med * 1e-3) / 1e9, 1))
    del arrow, eng, X
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=20_000_000)
    ap.add_argument('--n-blocks', type=int, default=8)
    ap.add_argument('--band', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--json-out', type=str, default=None)
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "needs a HIP GPU"
    torch.cuda.set_device(0)
    import bench

    nb = args.n_blocks
    w = args.rows // nb
    grids, _, _ = bench.build_blocks_for_rank(0, 1, w, nb, 1, 'cuda', args.band)
    f32 = time_case(grids, w, nb, 128, np.float32, args.reps, args.warmup)
    f64 = time_case(grids, w, nb, 64, np.float64, args.reps, args.warmup)
    # the name string as the runtime reports it, which can be a generic one
    # ("AMD Radeon Graphics") on an Instinct card: a label, not an identity
    out = dict(runtime_device_name=torch.cuda.get_device_name(0),
               f32_k128=f32, f64_k64=f64,
               algorithmic_byte_ratio=round(
                   f64['algorithmic_bytes'] / f32['algorithmic_bytes'], 4),
               time_ratio_median=round(f64['ms_median'] / f32['ms_median'], 4))
    line = json.dumps(out)
    print(line)
    if args.json_out:
        with open(args.json_out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
