"""Time the affine step X <- alpha * A@X + gamma * R on the fused single-launch
structure of bench.py's synthetic matrix, three ways in one session (HIP
events around each step, a warm-up first, float32):

    (a) the plain launch, C = A@X;
    (b) the fused affine launch, C = alpha * A@X + gamma * R in the
        write-back;
    (c) the plain launch followed by the tail kernel C = alpha * C + gamma * R.

Algorithmic bytes (DESIGN.md roofline):

    (a) 8 nnz + 4 (rows + 1) + 2 * 4 k rows
    (b) 8 nnz + 4 (rows + 1) + 3 * 4 k rows      one more read of R
    (c) 8 nnz + 4 (rows + 1) + 5 * 4 k rows      + read C, read R, write C

Prints one JSON line: ms/step (median and best of --reps) of each, the byte
and time ratios (b)/(a) and (c)/(a). Recorded, not gated.

Usage: python tools/affine_fused_vs_unfused.py [--rows 20000000] [--k 128]
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

ALPHA, GAMMA = 0.85, 0.15


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    events = []
    for _ in range(reps):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        events.append((s, e))
    torch.cuda.synchronize()
    return [s.elapsed_time(e) for s, e in events]


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
    assert eng._A_all is not None, "expected the fused single-launch layout"
    g = torch.Generator(device='cuda')
    g.manual_seed(42)
    draw = lambda: torch.rand(eng.X_i.shape, generator=g, device='cuda',
                              dtype=torch.float32) * 2 - 1
    # the features stay put between steps: every step does the same work
    eng.set_features(draw())
    R = draw()

    plain = timed(arrow.step, args.reps, args.warmup)

    arrow.set_affine_step(ALPHA, GAMMA, R)
    calls = [0]
    inner = eng.backend.axpby_rows

    def counted(*a, **kw):
        calls[0] += 1
        return inner(*a, **kw)
    eng.backend.axpby_rows = counted
    fused = timed(arrow.step, args.reps, args.warmup)
    assert calls[0] == 0, "the fused layout called the tail kernel"
    eng.backend.axpby_rows = inner
    Rbuf = eng._R
    arrow.clear_affine_step()   # plain launches; Rbuf keeps R resident

    def unfused():
        arrow.step()
        eng.backend.axpby_rows(eng.C_i, Rbuf, ALPHA, GAMMA)
    tail = timed(unfused, args.reps, args.warmup)

    nnz, rows = eng._A_all.nnz, nb * w
    base = 8 * nnz + 4 * (rows + 1)
    nbytes = dict(plain=base + 2 * 4 * k * rows, fused=base + 3 * 4 * k * rows,
                  unfused=base + 5 * 4 * k * rows)

    def summary(ms, key):
        med = statistics.median(ms)
        return dict(ms_median=round(med, 4), ms_best=round(min(ms), 4),
                    ms_all=[round(t, 4) for t in ms],
                    algorithmic_bytes=nbytes[key],
                    tbs_median=round(nbytes[key] / (med * 1e-3) / 1e12, 3))
    a, b, c = (summary(plain, 'plain'), summary(fused, 'fused'),
               summary(tail, 'unfused'))
    out = dict(
        # the name string as the runtime reports it: a label, not an identity
        runtime_device_name=torch.cuda.get_device_name(0),
        dtype='float32', k=k, rows=rows, nnz=nnz, alpha=ALPHA, gamma=GAMMA,
        plan=hip.spmm_plan(k, nnz, -1),
        plain=a, fused=b, unfused=c,
        byte_ratio_fused_over_plain=round(nbytes['fused'] / nbytes['plain'], 4),
        byte_ratio_unfused_over_plain=round(
            nbytes['unfused'] / nbytes['plain'], 4),
        time_ratio_fused_over_plain=round(b['ms_median'] / a['ms_median'], 4),
        time_ratio_unfused_over_plain=round(c['ms_median'] / a['ms_median'], 4),
        not_run=["float64 and bfloat16 features (float32 only is timed)",
                 "world>1 (the affine step is refused there)",
                 "the folds and the layouts that finish with the tail kernel "
                 "inside an engine step"])
    line = json.dumps(out)
    print(line)
    if args.json_out:
        with open(args.json_out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
