"""Time the step norms sum (C - X)^2, sum C^2 of the affine step on the fused
single-launch structure of bench.py's synthetic matrix, four ways in one
session (HIP events around each step, a warm-up first, float32):

    (a) the affine launch, C = alpha * A@X + gamma * R;
    (b) the affine-norm launch: (a) that also measures, in its write-back;
    (c) (a) followed by the stand-alone pass arrow_diffnorm_rows_f32;
    (d) (a) followed by torch: (C - X).square().sum() and C.square().sum().

Algorithmic bytes (DESIGN.md roofline):

    (a) 8 nnz + 4 (rows + 1) + 3 * 4 k rows
    (b) 8 nnz + 4 (rows + 1) + 4 * 4 k rows      one more read of X as D
    (c) 8 nnz + 4 (rows + 1) + 5 * 4 k rows      + read C, read X
    (d) 8 nnz + 4 (rows + 1) + 8 * 4 k rows      + read C, read X, write and
                                                   read the temporary, read C

Prints one JSON line: ms/step (median and best of --reps) of each and the
byte and time ratios against (a). Recorded, not gated.

Usage: python tools/norm_fused_vs_unfused.py [--rows 20000000] [--k 128]
                                             [--reps 20] [--json-out F]
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

from tools.affine_fused_vs_unfused import ALPHA, GAMMA, timed  # noqa: E402


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
    from arrow_matrix_amd import hip
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
    assert eng._A_all is not None, "expected the fused single-launch layout"
    g = torch.Generator(device='cuda')
    g.manual_seed(42)
    draw = lambda: torch.rand(eng.X_i.shape, generator=g, device='cuda',
                              dtype=torch.float32) * 2 - 1
    # the features stay put between steps: every step does the same work
    eng.set_features(draw())
    arrow.set_affine_step(ALPHA, GAMMA, draw())

    affine = timed(arrow.step, args.reps, args.warmup)

    arrow.track_step_norms()
    before = (be.norm_launches, be.diffnorm_launches)
    fused = timed(arrow.step, args.reps, args.warmup)
    n = args.reps + args.warmup
    assert (be.norm_launches - before[0], be.diffnorm_launches - before[1]) \
        == (n, 0), "the fused layout did not measure in its launch"
    fused_norms = arrow.last_step_norms()
    arrow.track_step_norms(False)

    acc = be.norm_acc()

    def stand_alone():
        arrow.step()
        acc.zero_()
        be.diffnorm_rows(eng.C_i, eng.X_i, acc)
    alone = timed(stand_alone, args.reps, args.warmup)
    alone_norms = tuple(float(v) for v in acc.sqrt().tolist())

    out_t = [None, None]

    def with_torch():
        arrow.step()
        out_t[0] = (eng.C_i - eng.X_i).square().sum()
        out_t[1] = eng.C_i.square().sum()
    torch_ms = timed(with_torch, args.reps, args.warmup)
    torch_norms = tuple(float(v.sqrt()) for v in out_t)

    nnz, rows = eng._A_all.nnz, nb * w
    base = 8 * nnz + 4 * (rows + 1)
    nbytes = {key: base + f * 4 * k * rows for key, f in
              (('affine', 3), ('fused', 4), ('stand_alone', 5), ('torch', 8))}

    def summary(ms, key):
        med = statistics.median(ms)
        return dict(ms_median=round(med, 4), ms_best=round(min(ms), 4),
                    ms_all=[round(t, 4) for t in ms],
                    algorithmic_bytes=nbytes[key],
                    tbs_median=round(nbytes[key] / (med * 1e-3) / 1e12, 3))
    res = dict(affine=summary(affine, 'affine'), fused=summary(fused, 'fused'),
               stand_alone=summary(alone, 'stand_alone'),
               torch=summary(torch_ms, 'torch'))
    a_ms = res['affine']['ms_median']
    out = dict(
        # the name string as the runtime reports it: a label, not an identity
        runtime_device_name=torch.cuda.get_device_name(0),
        dtype='float32', k=k, rows=rows, nnz=nnz, alpha=ALPHA, gamma=GAMMA,
        plan=hip.spmm_plan(k, nnz, -1), **res,
        norms=dict(fused=fused_norms, stand_alone=alone_norms,
                   torch_float32=torch_norms),
        byte_ratio_over_affine={key: round(nbytes[key] / nbytes['affine'], 4)
                                for key in nbytes},
        time_ratio_over_affine={key: round(res[key]['ms_median'] / a_ms, 4)
                                for key in res},
        not_run=["float64 and bfloat16 features (float32 only is timed)",
                 "world>1 (step norms are refused there)",
                 "the layouts that measure with the stand-alone pass inside "
                 "an engine step"])
    line = json.dumps(out)
    print(line)
    if args.json_out:
        with open(args.json_out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
