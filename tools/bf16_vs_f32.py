"""Time the fused single-launch structure with bfloat16 features against
float32 at the same k on bench.py's synthetic matrix (HIP events around the
launch, a warm-up first, both in one session).

Only the storage of X and C differs: A is the same resident fp32 (col, val)
pairs, 8 B/nnz, in both cases. Algorithmic bytes per launch (DESIGN.md
roofline):

    8 * nnz + 4 * (rows + 1) + 2 * itemsize * k * rows

that is 8 nnz + 4 (rows + 1) + 8 k rows for float32 and + 4 k rows for
bfloat16. Prints one JSON line: ms/launch (median and best of --reps), the
algorithmic byte ratio bf16/f32, the time ratio, and the achieved
algorithmic TB/s of both. Recorded, not gated: the queue thresholds were
tuned for float32 rows and are not retuned here.

Usage: python tools/bf16_vs_f32.py [--rows 20000000] [--k 128] [--reps 20]
                                   [--json-out F]
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

A_BYTES = 8     # fp32 (col, val) pairs, for both feature dtypes


def time_case(grids, w, nb, k, dtype, reps, warmup):
    import torch
    from arrow_matrix_amd import hip
    from arrow_matrix_amd.arrow_dec import ArrowDecompositionMPI
    from arrow_matrix_amd.comm import Comm

    arrow = ArrowDecompositionMPI.initialize(
        Comm(), np.array([nb]), [None], [None], w, k, device='gpu',
        dtype=dtype)
    arrow.load_data_from_blocks(grids)
    arrow.zero_rhs(w, k, dtype=dtype)
    eng = arrow.engines[0]
    assert eng._A_all is not None, "expected the fused single-launch layout"
    itemsize = eng.backend.feat_itemsize
    name = 'bfloat16' if eng.backend.bf16 else eng.np_dtype.name
    g = torch.Generator(device='cuda')
    g.manual_seed(42)
    X = (torch.rand(eng.X_i.shape, generator=g, device='cuda',
                    dtype=torch.float32) * 2 - 1).to(eng.backend.torch_dtype)
    eng.set_features(X)
    # the warm-up also allocates the bf16 split-row scratch, outside timing
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
    plan = hip.spmm_plan(k, nnz, -1, dtype=eng.backend.feat_dtype)
    nbytes = A_BYTES * nnz + 4 * (rows + 1) + 2 * itemsize * k * rows
    med = statistics.median(ms)
    out = dict(dtype=name, k=k, rows=rows, nnz=nnz, plan=plan,
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
    ap.add_argument('--k', type=int, default=128)
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
    f32 = time_case(grids, w, nb, args.k, np.float32, args.reps, args.warmup)
    bf16 = time_case(grids, w, nb, args.k, torch.bfloat16, args.reps,
                     args.warmup)
    # the name string as the runtime reports it, which can be a generic one
    # ("AMD Radeon Graphics") on an Instinct card: a label, not an identity
    out = dict(runtime_device_name=torch.cuda.get_device_name(0),
               f32=f32, bf16=bf16,
               algorithmic_byte_ratio=round(
                   bf16['algorithmic_bytes'] / f32['algorithmic_bytes'], 4),
               time_ratio_median=round(bf16['ms_median'] / f32['ms_median'], 4),
               not_run=["world>1 (bfloat16 is refused there)",
                        "queue thresholds, chunk and grid sizes not retuned "
                        "for bfloat16 rows (fp32 values carried over by row "
                        "bytes)"])
    line = json.dumps(out)
    print(line)
    if args.json_out:
        with open(args.json_out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
