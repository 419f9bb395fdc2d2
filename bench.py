#!/usr/bin/env python3
"""Flagship benchmark: arrow-decomposition iterated SpMM on MI355X.

Measures BASELINE.json's metric (iterated-SpMM GFLOP/s + achieved HBM GB/s)
on the named configuration: at N=1 the workload is the configuration the
metric is quoted on — the 100M-row synthetic planar-like graph, width 12.5M
(8 block-rows), features k=128 (BASELINE.json configs[3]) — it fits one
MI355X (~125 GB of 288 GB HBM3E). `--gpus N` shards the SAME matrix's
block-rows over N ranks (strong scaling), launched by the driver as
torchrun with one rank per GPU over RCCL.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--rows R] [--features k]
                  [--dump-outputs DIR] [--full]

Timing: W untimed warmup steps, then exactly K steps bracketed by
barrier + torch.cuda.synchronize on both sides; MAX over ranks; rank 0
prints ONE JSON line. Inputs are resident in HBM before the timed region
and seeded, so the same arguments give the same inputs on every run.
On a single GPU the timed loop replays a captured two-step hipGraph; an odd
K ends on one uncaptured step, so `ms_per_step` then averages K-1 replayed
steps and one plainly launched one (the launch cost is microseconds against
~50 ms of kernel time).

A plain run does only that: set up, warm up, time the K steps, write the
last step's result stripe if `--dump-outputs DIR` is given, print the line
(`roofline` and `cpu_baseline` are null). `--full` adds the secondary
measurements described below, each in a pass of its own outside the timed
region: the streaming HBM peak, the HIP-event roofline pass, the rocprofv3
traffic probe and the CPU baseline.

The `roofline` object reports the dominant kernel (spmm_kernel): the
§8d algorithmic bytes PER ITERATION — `8*nnz (A pairs, read once) +
4*(rows+1) (work items) + 4*k*rows (X stripe read ONCE per iteration,
regardless of how many launches touch it) + 4*k*rows (C written once)` —
divided by the HIP-event-measured total kernel time of the instrumented
iterations on the launch stream. The per-launch accounting (each launch's
own X operand counted separately; the round-1 headline) is kept as the
secondary field `achieved_per_launch`. `traffic` is the rocprofv3
PMC-measured fabric traffic per launch (tools/measure_traffic.py, run
by --full at N=1 when rocprofv3 is present; ARROW_TRAFFIC_PROBE=0
skips, ARROW_TRAFFIC_JSON points at a pre-measured file).
`cpu_baseline` times the reference's own CPU arithmetic (scipy CSR @,
arrow_slim_mpi.py:109-144 — restated via oracle semantics) on a bounded
sample of the same workload on ALL host cores (multiprocessing fork; core
count reported).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def build_parser():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument('--gpus', type=int, default=1)
    p.add_argument('--steps', type=int, default=5)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--rows', type=int, default=100_000_000,
                   help='total rows n (width = n / n-blocks)')
    p.add_argument('--features', type=int, default=128)
    p.add_argument('--n-blocks', type=int, default=8)
    p.add_argument('--parts', type=int, default=1,
                   help='decomposition length L (L>1 exercises the '
                        'inter-part alltoallv exchange)')
    p.add_argument('--device', type=str, default='gpu', choices=['gpu', 'cpu'])
    p.add_argument('--band', type=int, default=1024,
                   help='diagonal-block band half-width (planar-like locality)')
    p.add_argument('--full', action='store_true',
                   help='also run the secondary measurements (streaming HBM '
                        'peak, HIP-event roofline pass, rocprofv3 traffic '
                        'probe, CPU baseline); a plain run only sets up, '
                        'warms up, times the steps and prints the result')
    p.add_argument('--no-cpu-baseline', action='store_true',
                   help='with --full: skip the CPU baseline leg')
    p.add_argument('--cpu-baseline-seconds', type=float, default=8.0,
                   help='with --full: how long each core runs the CPU '
                        'baseline sample')
    p.add_argument('--dump-outputs', type=str, default=None, metavar='DIR',
                   help='after the timed steps write the result stripe of '
                        'the last timed step to DIR/C.npy (float32; '
                        'DIR/C_rank<r>.npy per rank at world>1); at most '
                        '32 MiB over all ranks: a stripe over its 1/world '
                        'share is cut to a fixed seeded row sample')
    p.add_argument('--json-out', type=str, default=None)
    p.add_argument('--check', action='store_true',
                   help='parity mode (L=1): run 3 iterations of the exact '
                        'bench pipeline (incl. the allreduce_x0 deferred '
                        'collective at world>1) and compare against a '
                        'scipy golden rebuilt from the deterministic '
                        'generators; prints a check line and exits')
    p.add_argument('--graph', choices=['auto', 'on', 'off'], default='auto',
                   help='hipGraph-capture the steady-state iteration '
                        '(BASELINE cfg5); auto = on for single-GPU runs. '
                        'world>1 stays capture-less by default: capturing '
                        'RCCL collectives could not be validated on a '
                        '1-GPU rig (RCCL 2.26 refuses two ranks per '
                        'device, profiles/r02_ab3_summary.log) and the '
                        'chunk-pipelined C_0 allreduce already overlaps '
                        'the collective with compute')
    return p


# --- synthetic planar-like arrow blocks (deterministic per block id) --------

DIAG_DEG = 6
COL_DEG = 2
ROW0_DEG = 2
HUB_ROWS = 16
HUB_NNZ = 50_000
# Values are positive and every row of the assembled matrix sums to 1 (each
# block carries a fixed share of its rows' sum, see ROW_SHARE): the
# iteration X := A X then neither grows nor dies out, so the result stays
# finite and non-trivial after any number of steps. A signed, unnormalised
# A grows ~5x per step through the hub rows (measured at the default size:
# max|C| = 2.2e6 nine steps after |X| <= 1), i.e. overflows f32 near step
# 55. Only the values differ; the sparsity pattern is the workload.
ROW_SHARE = {'diag': 0.75, 'col': 0.25, 'row0': 1.0}


def _gen_cols(role, w, deg, band, gen, device):
    import torch
    if role == 'diag':
        base = torch.arange(w, device=device, dtype=torch.int64).unsqueeze(1)
        delta = torch.randint(-band, band + 1, (w, deg), generator=gen, device=device)
        cols = (base + delta) % w
    else:
        # zipf-like skew toward low (hub) indices (col ~ w·u^4: the top 4%
        # of rows take ~45% of draws): arrow decompositions place the
        # highest-degree vertices first in the head, so the first-block-
        # column/row accesses concentrate on hot hub rows
        u = torch.rand((w, deg), generator=gen, device=device)
        cols = (u * u * u * u * w).long().clamp_(max=w - 1)
    return torch.sort(cols, dim=1).values


def generate_block(role, w, seed, device, band, share=1.0):
    """Returns (indptr int64, indices int32, data f32) host numpy arrays for
    one w x w block. Each row's values are positive and sum to `share`."""
    import torch
    deg = {'diag': DIAG_DEG, 'col': COL_DEG, 'row0': ROW0_DEG}[role]
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    cols = _gen_cols(role, w, deg, band, gen, device)
    if role == 'row0' and w > 4 * HUB_NNZ:
        # hub rows: the first rows of the arrow head are dense-ish
        hub = torch.sort(
            (torch.rand((HUB_ROWS, HUB_NNZ), generator=gen, device=device) * w)
            .long().clamp_(max=w - 1), dim=1).values
        counts = torch.full((w,), deg, dtype=torch.int64, device=device)
        counts[:HUB_ROWS] += HUB_NNZ
        indptr = torch.zeros(w + 1, dtype=torch.int64, device=device)
        torch.cumsum(counts, 0, out=indptr[1:])
        head = torch.cat([hub, cols[:HUB_ROWS]], dim=1)
        head = torch.sort(head, dim=1).values
        indices = torch.cat([head.flatten(), cols[HUB_ROWS:].flatten()])
    else:
        indices = cols.flatten()
        indptr = torch.arange(0, indices.numel() + 1, deg, dtype=torch.int64,
                              device=device)
    nnz = indices.numel()
    data = torch.rand(nnz, generator=gen, device=device) + 0.5
    # rows are uniform-length runs: the hub head (if any), then the rest
    hub_rows = HUB_ROWS if nnz > cols.numel() else 0
    n_head = hub_rows * (HUB_NNZ + deg)
    runs = [data[n_head:].view(-1, deg)]
    if hub_rows:
        runs.append(data[:n_head].view(hub_rows, HUB_NNZ + deg))
    for rows in runs:
        rows *= (share / rows.sum(dim=1, keepdim=True,
                                  dtype=torch.float64)).float()
    return (indptr.cpu().numpy(),
            indices.to(torch.int32).cpu().numpy(),
            data.float().cpu().numpy())


def block_csr(role, w, seed, device, band, share=1.0):
    from scipy import sparse
    indptr, indices, data = generate_block(role, w, seed, device, band, share)
    return sparse.csr_matrix((data, indices, indptr), shape=(w, w))


def expected_nnz(w, nb):
    per_part = nb * (ROW0_DEG * w) + (nb - 1) * (DIAG_DEG + COL_DEG) * w
    if w > 4 * HUB_NNZ:
        per_part += nb * HUB_ROWS * HUB_NNZ
    return per_part


def build_blocks_for_rank(rank, world, w, nb, parts, gen_device, band):
    """Block grids (only this rank's blocks materialised) for each part."""
    grids = []
    bpr = -(-nb // world)
    first = min(rank * bpr, nb)
    last = min(first + bpr, nb)
    # the parts' products add up, and block-row 0 is spread over nb blocks
    sh = {'row0': ROW_SHARE['row0'] / (nb * parts),
          'diag': ROW_SHARE['diag'] / parts, 'col': ROW_SHARE['col'] / parts}
    for p in range(parts):
        grid = [[None] * nb for _ in range(nb)]
        for c in range(first, last):
            grid[0][c] = block_csr('row0', w, 10_000 * p + 10 * c + 1,
                                   gen_device, band, sh['row0'])
        for r in range(max(first, 1), last):
            grid[r][r] = block_csr('diag', w, 10_000 * p + 10 * r + 2,
                                   gen_device, band, sh['diag'])
            grid[r][0] = block_csr('col', w, 10_000 * p + 10 * r + 3,
                                   gen_device, band, sh['col'])
        grids.append(grid)
    return grids, first, last


def _kernel_name(k, nnz_dominant):
    """Mirror the launcher's scheduler policy (csrc/arrow_spmm.hip): queue
    scheduler when GROUP >= 8 and the structure is big enough, unless
    ARROW_QUEUE forces it. nnz_dominant: nnz of the dominant structure."""
    env = os.environ.get('ARROW_QUEUE', '')
    if env == '0':
        return "spmm_kernel"
    if env.startswith('1'):
        return "spmm_kernel_q"
    vec = 4 if k % 4 == 0 else (2 if k % 2 == 0 else 1)
    lanes = (k + vec - 1) // vec
    group = 1
    while group < lanes and group < 64:
        group <<= 1
    big = nnz_dominant >= (32 << 20)
    if group >= 8 and big:
        return "spmm_kernel_q"
    if group >= 4 and big:
        return "spmm_kernel_qw"  # per-wave grabs at small GROUP (k=16)
    return "spmm_kernel"


def _cpu_worker(args):
    """One worker: alternate diag/row0 scipy CSRMMs for ~seconds s.
    (Top-level so multiprocessing can pickle it under any start method.)"""
    seconds, k, seed = args
    import time as _t
    A_diag, A_row0 = _CPU_BLOCKS  # inherited via fork (read-only, COW)
    cap_w = A_diag.shape[0]
    rng = np.random.default_rng(seed)
    X = (2 * rng.random((cap_w, k)) - 1).astype(np.float32)
    flops = 0.0
    t0 = _t.perf_counter()
    while True:
        C = A_diag @ X
        flops += 2.0 * A_diag.nnz * k
        C = A_row0 @ X
        flops += 2.0 * A_row0.nnz * k
        t = _t.perf_counter() - t0
        if t >= seconds:
            break
    del C
    return flops, t


_CPU_BLOCKS = None


def cpu_baseline_sample(w, band, k, threads=None, seconds=8.0):
    """Time the reference CPU arithmetic (scipy CSR @ dense,
    arrow_slim_mpi.py:109-144) on ALL host cores: every core runs the same
    bounded sample (one diagonal block + one hub row-0 block of this
    workload's shape) for ~8 s; value = total FLOPs / wall (the node's
    aggregate reference-CPU rate). Reported baseline, not the target."""
    global _CPU_BLOCKS
    import multiprocessing as mp
    if threads is None:
        threads = os.cpu_count() or 1
    cap_w = min(w, 250_000)
    A_diag = block_csr('diag', cap_w, 2, 'cpu', band)
    A_row0 = block_csr('row0', cap_w, 1, 'cpu', band)
    _CPU_BLOCKS = (A_diag, A_row0)
    jobs = [(seconds, k, 100 + i) for i in range(threads)]
    t0 = time.perf_counter()
    if threads == 1:
        results = [_cpu_worker(jobs[0])]
    else:
        ctx = mp.get_context('fork')
        with ctx.Pool(threads) as pool:
            results = pool.map(_cpu_worker, jobs)
    wall = time.perf_counter() - t0
    total_flops = sum(f for f, _ in results)
    gflops = total_flops / wall / 1e9
    hub = " incl. 16x50k-nnz hub rows" if cap_w > 4 * HUB_NNZ else ""
    return {
        "value": round(gflops, 3), "unit": "GFLOP/s", "cores": threads,
        "kind": "port",
        "sample": f"{threads} procs x (one {cap_w}-row diagonal block "
                  f"({A_diag.nnz} nnz) + one row-0 block ({A_row0.nnz} nnz"
                  f"{hub})) x k={k}, scipy CSR @ dense (the reference's cpu "
                  f"kernel), ~{seconds:.0f}s each, wall {wall:.1f}s",
    }


def traffic_probe(args):
    """Run tools/measure_traffic.py (rocprofv3 PMC passes) on this exact
    workload in a subprocess and return the per-launch fabric traffic, or
    None. Guarded so the probe's own bench child never recurses."""
    import shutil
    import subprocess
    if (os.environ.get('ARROW_TRAFFIC_PROBE', '1') == '0'
            or os.environ.get('ARROW_TRAFFIC_CHILD') == '1'
            or shutil.which('rocprofv3') is None):
        return None
    out = os.path.join(REPO, 'gpurun_out', 'traffic_auto.json')
    cmd = [sys.executable, os.path.join(REPO, 'tools', 'measure_traffic.py'),
           '--rows', str(args.rows), '--features', str(args.features),
           '--band', str(args.band), '--steps', '2', '--warmup', '1',
           '--out', out]
    try:
        log = os.path.join(REPO, 'gpurun_out', 'traffic_auto.err')
        os.makedirs(os.path.dirname(log), exist_ok=True)
        with open(log, 'w') as lf:
            subprocess.run(cmd, check=True, timeout=420,
                           stdout=lf, stderr=lf)
        with open(out) as f:
            t = json.load(f)
        if t.get('workload', {}).get('rows') == args.rows:
            return round(t['avg_read_bytes'] + t['avg_write_bytes_raw'])
    except Exception as e:
        print(f"# traffic probe skipped: {e}", file=sys.stderr)
    return None


def parity_check(arrow, comm, w, nb, k, band, use_gpu, world):
    """3 iterations of the bench pipeline vs a scipy golden rebuilt from
    the same deterministic block generators (L=1 only). Every rank's
    feature stripe is seeded by rank with a numpy rng so rank 0 can
    reproduce the full X."""
    import torch
    from scipy import sparse
    eng0 = arrow.engines[0]
    first, last = eng0.first_block, eng0.last_block
    stripe_np = (2 * np.random.default_rng(100 + comm.rank)
                 .random(((last - first) * w, k)) - 1).astype(np.float32)
    if stripe_np.shape[0] == 0:
        stripe_np = np.zeros((w, k), np.float32)
    X0 = torch.from_numpy(stripe_np.copy())
    eng0.set_features(X0.cuda() if use_gpu else X0)
    for _ in range(3):
        arrow.step()
        eng0.set_features(eng0.result_tile())
    # the deferred C_0 collective of the LAST step is waited only at the
    # next step's consumer — run one more step so every rank's stripe
    # (incl. the head refresh) reflects iteration 3... simpler: compare
    # against FOUR golden iterations after a fourth step.
    arrow.step()
    eng0.set_features(eng0.result_tile())
    iters = 4
    # rank-LOCAL comparison (no collective in the check itself: gloo has
    # no CUDA all_gather); every rank rebuilds the full A and X from the
    # deterministic generators and checks its own stripe.
    eng0._flush_x0_pipeline()  # drain the deferred collective + head copy
    C_local = eng0.feature_tile().cpu().numpy()
    first, last = eng0.first_block, eng0.last_block
    gen_device = 'cuda' if use_gpu else 'cpu'
    bpr = -(-nb // world)
    stripes = []
    for r in range(world):
        f, l = min(r * bpr, nb), min(min(r * bpr, nb) + bpr, nb)
        if l > f:
            stripes.append((2 * np.random.default_rng(100 + r)
                            .random(((l - f) * w, k)) - 1)
                           .astype(np.float32))
    X_full = np.concatenate(stripes)
    rows_l, cols_l, data_l = [], [], []
    for c in range(nb):
        ip, ix, dv = generate_block('row0', w, 10 * c + 1, gen_device, band,
                                    ROW_SHARE['row0'] / nb)
        rows_l.append(np.repeat(np.arange(w), np.diff(ip)))
        cols_l.append(ix.astype(np.int64) + c * w)
        data_l.append(dv)
    for r in range(1, nb):
        for role, seed, coff in (('diag', 10 * r + 2, r * w),
                                 ('col', 10 * r + 3, 0)):
            ip, ix, dv = generate_block(role, w, seed, gen_device, band,
                                        ROW_SHARE[role])
            rows_l.append(np.repeat(np.arange(w), np.diff(ip)) + r * w)
            cols_l.append(ix.astype(np.int64) + coff)
            data_l.append(dv)
    A = sparse.csr_matrix(
        (np.concatenate(data_l),
         (np.concatenate(rows_l), np.concatenate(cols_l))),
        shape=(nb * w, nb * w))
    G = X_full
    for _ in range(iters):
        G = A @ G
    G_local = G[first * w:last * w]
    n_cmp = min(C_local.shape[0], G_local.shape[0])
    err = float(np.abs(C_local[:n_cmp] - G_local[:n_cmp]).max()) \
        if n_cmp else 0.0
    scale = max(1.0, float(np.abs(G).max()))
    ok = err <= 1e-4 * scale
    flag = torch.tensor([0.0 if ok else 1.0])
    comm.allreduce_max_(flag)
    status = {"check": "ok" if flag.item() == 0 else "FAIL",
              "rank_max_abs_err": err, "scale": scale,
              "rel_err": err / scale, "world": world, "rows": nb * w,
              "k": k, "iters": iters}
    if comm.rank == 0:
        print(json.dumps(status))
    else:
        print(f"# rank {comm.rank} check err={err:.3e}", file=sys.stderr)
    return status


def measure_hbm_peak(reps=10, gib=2.0):
    """Streaming HBM peak on THIS box (the roofline
    denominator is the measured per-GPU peak, spec stated alongside).
    Best of copy/scale/triad over fp32 buffers, HIP-event timed."""
    import torch
    n = int(gib * (1 << 30) / 4)
    x = torch.rand(n, device='cuda')
    z = torch.rand(n, device='cuda')
    y = torch.empty(n, device='cuda')
    for _ in range(3):
        y.copy_(x)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)

    def best(fn, bpe):
        t = float('inf')
        for _ in range(reps):
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            t = min(t, s.elapsed_time(e))
        return bpe * n / (t * 1e-3) / 1e9

    peak = max(best(lambda: y.copy_(x), 8),
               best(lambda: torch.mul(x, 1.0001, out=y), 8),
               best(lambda: torch.add(x, z, alpha=1.0001, out=y), 12))
    del x, z, y
    torch.cuda.empty_cache()
    return round(peak, 1)


DUMP_MAX_BYTES = 32 << 20  # all ranks' files together; each gets 1/world


def dump_outputs(out_dir, eng0, rank, world):
    """Write what the timed path handed back in its last step — this rank's
    result stripe C (== the next iteration's X) — as float32 .npy. A stripe
    over this rank's share of DUMP_MAX_BYTES (1/world of it, so the files of
    one run never exceed it together) is cut to a fixed, seeded sample of
    distinct rows (same rows every run, so two builds compare row for
    row)."""
    import torch
    eng0._flush_x0_pipeline()  # drain a deferred C_0 collective + head copy
    C = eng0.feature_tile()
    n, k = C.shape
    m = max(1, DUMP_MAX_BYTES // max(world, 1) // (4 * k))
    if n > m:
        rows = np.sort(np.random.default_rng(2024).choice(n, m, replace=False))
        C = C[torch.from_numpy(rows).to(C.device)]
    os.makedirs(out_dir, exist_ok=True)
    name = 'C' if world <= 1 else f'C_rank{rank}'
    np.save(os.path.join(out_dir, name + '.npy'),
            C.detach().cpu().numpy().astype(np.float32, copy=False))


def main():
    args = build_parser().parse_args()
    import torch

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', str(rank)))
    n_gpus = max(args.gpus, world)

    use_gpu = args.device == 'gpu'
    if use_gpu and not torch.cuda.is_available():
        raise RuntimeError("bench.py --device gpu needs a HIP GPU "
                           "(no silent CPU fallback); use --device cpu explicitly")

    import torch.distributed as dist
    from arrow_matrix_amd.arrow_dec import ArrowDecompositionMPI
    from arrow_matrix_amd.comm import TorchDistComm, Comm

    if world > 1:
        backend = os.environ.get('ARROW_BENCH_BACKEND',
                                 'nccl' if use_gpu else 'gloo')
        if use_gpu:
            # modulo lets oversubscribed validation runs share one device
            torch.cuda.set_device(local_rank % torch.cuda.device_count())
        dist.init_process_group(backend=backend)
        comm = TorchDistComm()
    else:
        if use_gpu:
            torch.cuda.set_device(local_rank)
        comm = Comm()

    nb = args.n_blocks
    w = args.rows // nb
    k = args.features
    L = args.parts
    gen_device = 'cuda' if use_gpu else 'cpu'

    hbm_peak_meas = None
    if args.full and use_gpu and rank == 0 and world <= 1 and not args.check:
        hbm_peak_meas = measure_hbm_peak()
        print(f"# measured streaming HBM peak: {hbm_peak_meas} GB/s "
              f"(spec 8000)", file=sys.stderr)

    t0 = time.perf_counter()
    grids, first, last = build_blocks_for_rank(comm.rank, comm.size, w, nb, L,
                                               gen_device, args.band)
    if rank == 0:
        print(f"# generated blocks in {time.perf_counter()-t0:.1f}s "
              f"(rank owns block-rows [{first},{last}))", file=sys.stderr)

    n_blocks = np.full(L, nb, dtype=np.int64)
    if L > 1:
        # a REAL random permutation between parts (deterministic) so the
        # forward/backward exchange routes rows across all ranks
        # (the alltoallv machinery is exercised at L >= 2)
        rng_p = np.random.default_rng(1234)
        perm = rng_p.permutation(nb * w).astype(np.int64)
        inv = np.argsort(perm)
        to_prev = [None] + [inv[first * w:last * w]] * (L - 1)
        to_next = [perm[first * w:last * w]] * (L - 1) + [None]
    else:
        to_prev, to_next = [None], [None]

    arrow = ArrowDecompositionMPI.initialize(comm, n_blocks, to_prev, to_next,
                                             w, k, device=args.device)
    t0 = time.perf_counter()
    arrow.load_data_from_blocks(grids)
    del grids
    arrow.zero_rhs(w, k)
    if rank == 0:
        print(f"# uploaded blocks in {time.perf_counter()-t0:.1f}s", file=sys.stderr)

    # features resident on device before the timed region
    eng0 = arrow.engines[0]
    for eng in arrow.engines:
        # iterated GNN-propagation loop (X := C): fuse C_0 reduce with the
        # next X_0 broadcast into one allreduce. Only
        # valid at L == 1: with multiple parts the inter-part exchange
        # rewrites C after the spmm, so next X_0 != this C_0.
        eng.allreduce_x0 = (args.device == 'gpu' and L == 1)
    if args.check:
        assert L == 1, "--check supports L=1 (the headline config)"
        parity_check(arrow, comm, w, nb, k, args.band, use_gpu, comm.size)
        if world > 1:
            dist.destroy_process_group()
        return

    if use_gpu:
        g = torch.Generator(device='cuda')
        g.manual_seed(42 + comm.rank)
        X = torch.rand(eng0.X_i.shape, generator=g, device='cuda') * 2 - 1
    else:
        g = torch.Generator()
        g.manual_seed(42 + comm.rank)
        X = torch.rand(eng0.X_i.shape, generator=g) * 2 - 1
    eng0.set_features(X)

    def sync():
        comm.barrier()
        if use_gpu:
            torch.cuda.synchronize()

    def one_step():
        arrow.step()
        eng0.set_features(eng0.result_tile())

    use_graph = use_gpu and (args.graph == 'on'
                             or (args.graph == 'auto' and world <= 1))
    steps = args.steps

    for _ in range(args.warmup):
        one_step()
    sync()

    # roofline instrumentation pass (--full; HIP events on the launch
    # stream; kept OUTSIDE the timed region so the timed loop is
    # uninstrumented)
    events = []
    if args.full:
        for eng in arrow.engines:
            eng.kernel_events = events
        for _ in range(2):
            one_step()
        sync()
        for eng in arrow.engines:
            eng.kernel_events = None

    graph = None
    if use_graph and steps >= 2:
        # hipGraph-captured steady-state iteration (BASELINE cfg5). One
        # capture spans TWO steps: the X<->C ping-pong returns to its
        # original buffer assignment after a pair, so a replay is exactly
        # 2 iterations.
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            one_step()
            one_step()
        graph.replay()
        sync()

    sync()
    t_start = time.perf_counter()
    if graph is not None:
        for _ in range(steps // 2):
            graph.replay()
        if steps % 2:
            # a replay leaves the ping-pong where the capture started, so
            # an odd --steps ends on one plain step: exactly `steps` timed
            one_step()
    else:
        for _ in range(steps):
            one_step()
    sync()
    elapsed = time.perf_counter() - t_start

    # MAX over ranks
    t_t = torch.tensor([elapsed], dtype=torch.float64,
                       device='cuda' if (world > 1 and use_gpu) else 'cpu')
    comm.allreduce_max_(t_t)
    elapsed = float(t_t.item())

    used_graph = graph is not None
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, eng0, comm.rank, comm.size)

    nnz_total = expected_nnz(w, nb) * L
    flops = 2.0 * nnz_total * k * steps
    gflops = flops / elapsed / 1e9

    # roofline from the kernel events (this rank; rank 0 reports)
    roofline = None
    if use_gpu and events:
        total_ms = 0.0
        per_launch_bytes = 0.0   # round-1 accounting: X counted per launch
        a_meta_bytes = 0.0       # A pairs + work-item metadata (per launch)
        if os.environ.get('ARROW_BENCH_LAUNCH_DETAIL') == '1':
            for i, (s, e, nnz, c_rows, x_rows) in enumerate(events):
                print(f"launch[{i}]: {s.elapsed_time(e):.3f} ms nnz={nnz} "
                      f"c_rows={c_rows} x_rows={x_rows}", file=sys.stderr)
        for s, e, nnz, c_rows, x_rows in events:
            total_ms += s.elapsed_time(e)
            a_meta_bytes += 8.0 * nnz + 4.0 * (c_rows + 1)
            per_launch_bytes += (8.0 * nnz + 4.0 * (c_rows + 1)
                                 + 4.0 * k * (x_rows + c_rows))
        # §8d X-ONCE accounting (the headline): per iteration each engine's
        # X stripe is charged ONCE (rows_touched), however many launches
        # read it, and C is charged once per row written. The instrumented
        # pass covers `instr_steps` iterations.
        instr_steps = 2
        stripe_rows = sum(eng.n_owned for eng in arrow.engines) * w
        xc_bytes = instr_steps * 4.0 * k * (2 * stripe_rows)  # X once + C once
        total_bytes = a_meta_bytes + xc_bytes
        achieved = total_bytes / (total_ms / 1e3) / 1e9  # GB/s
        achieved_pl = per_launch_bytes / (total_ms / 1e3) / 1e9
        peak = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
        # measured per-launch fabric traffic: pre-measured file
        # (ARROW_TRAFFIC_JSON) or the automatic rocprofv3 probe below
        traffic = None
        tj = os.environ.get('ARROW_TRAFFIC_JSON')
        if tj and os.path.exists(tj):
            with open(tj) as f:
                t = json.load(f)
            if t.get('workload', {}).get('rows') == args.rows:
                traffic = round(t['avg_read_bytes'] + t['avg_write_bytes_raw'])
        roofline = {
            "bound": "hbm",
            "achieved": round(achieved, 1),
            "peak": peak,
            "unit": "GB/s",
            "frac": round(achieved / peak, 4),
            "traffic": traffic,
            "achieved_per_launch": round(achieved_pl, 1),
            "kernel": _kernel_name(k, max(n for _, _, n, _, _ in events)),
            "launches": len(events),
            "avg_launch_ms": round(total_ms / len(events), 4),
        }
        if hbm_peak_meas:
            # §8d's denominator: the box's own measured streaming peak
            roofline["peak_measured"] = hbm_peak_meas
            roofline["frac_measured"] = round(achieved / hbm_peak_meas, 4)

    cpu_base = None
    if args.full and rank == 0 and world <= 1 and not args.no_cpu_baseline:
        cpu_base = cpu_baseline_sample(w, args.band, k,
                                       seconds=args.cpu_baseline_seconds)

    if (roofline is not None and roofline.get('traffic') is None
            and rank == 0 and world <= 1):
        # free the resident workload FIRST: the probe re-runs this bench as
        # a child under rocprofv3 and needs the HBM this process holds
        import gc
        graph = None
        X = None
        eng = None   # loop variable from the allreduce_x0 setup still
        eng0 = None  # pins an engine (structures + 51 GB stripes)
        arrow = None
        one_step = None  # the closure holds arrow/eng0
        events.clear()
        gc.collect()
        torch.cuda.empty_cache()
        free, total = torch.cuda.mem_get_info()
        print(f"# traffic probe: freed workload, {free/2**30:.0f} GiB free",
              file=sys.stderr)
        roofline['traffic'] = traffic_probe(args)

    if rank == 0:
        result = {
            "metric": "iterated_spmm_gflops",
            "value": round(gflops, 2),
            "unit": "GFLOP/s",
            "n_gpus": n_gpus,
            "steps": steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": f"cfg4_synth_{args.rows//1_000_000}M_k{k}",
                "rows": args.rows, "width": w, "n_blocks": nb, "parts": L,
                "features": k, "nnz": nnz_total, "band": args.band,
                "parallelism": f"block-rows over {n_gpus} GPU(s), RCCL/xGMI",
                "hipgraph": used_graph,
            },
            "roofline": roofline,
            "cpu_baseline": cpu_base,
        }
        line = json.dumps(result)
        print(line)
        if args.json_out:
            with open(args.json_out, 'w') as f:
                f.write(line + "\n")

    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
