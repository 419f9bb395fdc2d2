"""The multi-rank engine on one device, and the child entry point of
test_gpu_rank_engine.py. Two roles in one file:

    python tests/engine_ranks_driver.py launch <child> [cpu]
    python tests/engine_ranks_driver.py rank <child> [cpu]

`launch` never opens the GPU. It picks a free local port, starts the W ranks
of the child (tests/engine_cases_ranks.py) as fresh processes, each with its
own time limit, and waits. If a rank ends non-zero, with a signal or at its
limit, it ends the others, starts nothing more and exits with that rank's
status (a signal as 128 + its number; a time limit as 124), so that
tests/gpu_children.py sees what it latches on. Otherwise it merges the
ranks' JSON lines per job and prints one line each: ok only if every rank
said ok, max_err_over_bound the largest of any rank, rank 0's digests.

`rank` is one rank: gloo process group (the only backend that lets ranks
share a device; CUDA tensors are staged through the host by the backend or
by comm.py), engines built through save -> load_decomposition_new(comm) ->
initialize(comm, device=...), and the child's jobs through the job loop of
tests/child_harness.py. A job runs the exact class bit for bit and the real
class to engine_cases_ranks.step_bound. EVERY rank checks its own stripe
C_i[:n_owned * w] against the golden's rows for its blocks, and the gathered
result as well.

Ranks stay in step whatever they find: a failed comparison is recorded, the
job issues every collective it would have issued, and at its end the ranks
exchange their verdicts, so that all of them fail the job together and exit
1 without anyone waiting for a peer that has left. Only an error (a library
error, a collective that timed out) ends one rank alone; the launcher then
ends the others.

Readout in the allreduce_x0 jobs. result_tile() does not flush the deferred
C_0 allreduce: between steps the head rows of rank 0's stripe are stale by
design (the engine refreshes them at the top of the next step). The path that
flushes is allgather_result(); a rank reads its own stripe after it. These
jobs read out only every second step, so that the other steps leave the
collective pending across the step boundary; such a step's result is checked
all the same, as the features the next step consumed (gathered from
feature_tile() AFTER that step, when rank 0 has refreshed its head from the
reduced X_0). This is a plain module, not a test file.
"""
import hashlib
import json
import os
import socket
import subprocess
import sys
import tempfile
import time
import traceback

import numpy as np

if not __package__:         # started as a script: see tests/child_harness.py
    import child_harness  # noqa: F401
from tests import child_harness as ch  # noqa: E402

from tests import engine_affine_driver as ead  # noqa: E402
from tests import engine_cases_queue as ecq  # noqa: E402
from tests import engine_cases_ranks as ecr  # noqa: E402
from tests.gpu_children import ENGINE_VARS, FATAL_STATUS  # noqa: E402
from tests.spmm_cases import KERNEL_VARS  # noqa: E402

DRIVER = os.path.abspath(__file__)
START_VARS = KERNEL_VARS + ENGINE_VARS + ('ARROW_X0_DEFER',)
EXIT_TIMEOUT = 124
assert EXIT_TIMEOUT in FATAL_STATUS


# ---------------------------------------------------------------------------
# launch: W fresh processes, one verdict
# ---------------------------------------------------------------------------

def free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def exit_status(returncode):
    """A rank's status as the launcher's own: a signal becomes 128 + its
    number where gpu_children latches on that, else EXIT_ERRORED."""
    if returncode >= 0:
        return returncode
    status = 128 - returncode
    return status if status in FATAL_STATUS else ch.EXIT_ERRORED


def _end(procs):
    for p in procs:
        if p.poll() is None:
            p.terminate()
    for p in procs:
        try:
            p.wait(timeout=5)
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()


def run_ranks(commands, limit_s, env=None, poll_s=0.05):
    """Starts one process per command, all at once, rank r with RANK=r,
    WORLD_SIZE, MASTER_ADDR and a free MASTER_PORT, and waits for all of
    them. Returns (status, [stdout of each rank]): 0 when every rank exited
    0; else the status of the first rank seen to end non-zero or with a
    signal, or 124 when one reached limit_s; the others are ended then and
    nothing more is started."""
    env = dict(os.environ if env is None else env)
    env.update(WORLD_SIZE=str(len(commands)), MASTER_ADDR='127.0.0.1',
               MASTER_PORT=str(free_port()))
    with tempfile.TemporaryDirectory() as td:
        outs = [open(os.path.join(td, f'rank{r}.out'), 'w+')
                for r in range(len(commands))]
        procs = []
        status = 0
        try:
            for r, argv in enumerate(commands):
                procs.append(subprocess.Popen(
                    argv, env=dict(env, RANK=str(r)), cwd=ch.REPO,
                    stdin=subprocess.DEVNULL, stdout=outs[r]))
            deadline = time.monotonic() + limit_s
            while status == 0 and any(p.poll() is None for p in procs):
                for r, p in enumerate(procs):
                    if p.poll() not in (None, 0):
                        status = exit_status(p.returncode)
                        print(f"# rank {r} ended with status {p.returncode}",
                              file=sys.stderr)
                        break
                else:
                    if time.monotonic() > deadline:
                        status = EXIT_TIMEOUT
                        print(f"# a rank reached its {limit_s}s limit",
                              file=sys.stderr)
                    else:
                        time.sleep(poll_s)
            if status == 0:
                bad = [p.returncode for p in procs if p.returncode != 0]
                status = exit_status(bad[0]) if bad else 0
        finally:
            _end(procs)
        texts = []
        for f in outs:
            f.seek(0)
            texts.append(f.read())
            f.close()
    return status, texts


def merge(names, rank_lines):
    """One line per job name that any rank printed, in `names`' order.
    rank_lines: per rank {case: line}."""
    merged = []
    for name in names:
        lines = [rl.get(name) for rl in rank_lines]
        if not any(lines):
            continue
        line = dict(next(ln for ln in lines if ln))
        line['ranks'] = len(lines)
        line['ok'] = all(ln is not None and ln['ok'] for ln in lines)
        bad = [(r, ln) for r, ln in enumerate(lines)
               if ln is None or not ln['ok']]
        line.pop('error', None)
        line.pop('errored', None)
        if bad:
            line['error'] = '; '.join(
                f"rank {r}: {ln['error'] if ln else 'no line'}"
                for r, ln in bad)[:2000]
            if any(ln is not None and ln.get('errored') for _, ln in bad):
                line['errored'] = True
        for key in ('max_err_over_bound', 'exact_mismatch', 'ms'):
            values = [ln[key] for ln in lines if ln and key in ln]
            if values:
                line[key] = max(values)
        plans = set()
        for ln in lines:
            plans |= set((ln or {}).get('plans', ()))
        if any('plans' in (ln or {}) for ln in lines):
            line['plans'] = sorted(plans)
        if lines[0] and 'digests' in lines[0]:
            line['digests'] = lines[0]['digests']
        line.pop('rank', None)
        merged.append(line)
    return merged


def launch(child, device):
    from tests.gpu_children import json_lines
    world = ecr.world_of(child)
    argv = [sys.executable, DRIVER, 'rank', child, device]
    status, texts = run_ranks([argv] * world, ecr.rank_limit(child))
    for line in merge(ecr.job_names(child), [json_lines(t) for t in texts]):
        print(json.dumps(line), flush=True)
    return status


# ---------------------------------------------------------------------------
# rank: the engine of one case
# ---------------------------------------------------------------------------

def np_dtype(precision):
    return np.float64 if precision == 'float64' else np.float32


def build(comm, decomp, shape, precision, k, device):
    """save -> load_decomposition_new(comm) -> initialize(comm) -> zero_rhs,
    as engine_affine_driver.build does at world 1; every rank writes and
    reads files of its own."""
    from arrow_matrix_amd import graphio
    from arrow_matrix_amd.arrow_dec import ArrowDecompositionMPI
    args = ecr.build_args(shape, k)
    width = args['width']
    block_diagonal = args.get('block_diagonal', True)
    dtype = np_dtype(precision)
    with tempfile.TemporaryDirectory() as td:
        prefix = os.path.join(td, 'g')
        graphio.save_decomposition_new(decomp, prefix, width,
                                       block_diagonal=block_diagonal)
        blocks, nb, tp, tn = ArrowDecompositionMPI.load_decomposition_new(
            comm, prefix, width, is_block_diagonal=block_diagonal,
            datatype=dtype)
        arrow = ArrowDecompositionMPI.initialize(
            comm, nb, tp, tn, width, k, device=device,
            block_diagonal=block_diagonal, slim=args.get('slim', True),
            dtype=dtype)
        arrow.load_data_from_blocks(blocks)
        arrow.zero_rhs(width, k, dtype=dtype)
    assert [int(b) for b in nb] == list(args['n_blocks'])
    return arrow


def set_options(arrow, options):
    for i, eng in enumerate(arrow.engines):
        eng.allreduce_x0 = options == 'x0all' or (options == 'x0' and i == 0)


def check_structure(arrow, case, device):
    """The engines are the ones the case means: the spans, the two-launch
    layout, the chunk count of the C_0 reduce, the banded engine."""
    shape = ecr.SHAPES[case.shape]
    w = shape['width']
    for eng, nb in zip(arrow.engines, shape['n_blocks']):
        assert eng.comm.size == case.world
        assert (eng.first_block, eng.last_block) == \
            ecr.owned_blocks(nb, case.world, eng.comm.rank)
        assert eng.banded == (not shape.get('slim', True))
        want = int(case.variables.get('ARROW_ROW0_CHUNKS',
                                      4 if w >= 64 else 1))
        assert eng._row0_chunks(w) == min(want, w)
        if device == 'gpu':
            assert eng._A_all is None
            if eng.n_owned:
                assert len(eng._A_row0) == eng._row0_chunks(w)
            else:
                assert not eng._A_row0 and not eng._A_rest
    assert arrow._folded is None


def plans_of(arrow, precision, k):
    """The scheduler names of every resident structure of this rank."""
    from arrow_matrix_amd import hip
    from tests import engine_queue_driver as eqd
    blocks = eqd.resident_structures(arrow)
    for eng in arrow.engines:
        blocks += [bd[0] for bd in (eng._A_bd_lo, eng._A_bd_hi) if bd]
    return sorted({ecq.SCHED_NAME[hip.spmm_plan(
        k, blk.nnz, -1, ead.dtype_of(precision))['scheduler']]
        for blk in blocks})


def stripe(eng, full, dtype):
    """This rank's rows of `full` (part 0's order) as the engine takes its
    features; a rank that owns nothing holds one tile of zeros."""
    w = eng.width
    rows = full[eng.first_block * w:eng.last_block * w]
    if not rows.shape[0]:
        rows = np.zeros((w, full.shape[1]))
    return np.ascontiguousarray(rows.astype(dtype))


def gather_stripes(eng, tensor):
    """The ranks' stripes of `tensor` (features or result of `eng`) side by
    side as numpy, like allgather_result but with no flush of the deferred
    allreduce."""
    w, k = eng.width, tensor.shape[1]
    pad = eng.backend.zeros((eng.blocks_per_rank * w, k))
    if eng.n_owned:
        pad[:eng.n_owned * w].copy_(tensor[:eng.n_owned * w])
    return eng.comm.allgather_cat(pad)[:eng.tiles_per_side * w].cpu().numpy()


def own_result(eng):
    """C_i[:n_owned * w] on the host. Call after allgather_result(), the
    readout that flushes the deferred allreduce."""
    return eng.result_tile()[:eng.n_owned * eng.width].cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def reads_out(case, step):
    """allreduce_x0 jobs read out every second step, the others every one."""
    return case.options != 'x0' or step % 2 == 1


def run_exact(comm, case, device, errors):
    """Steps from new integer features each; a readout step equals the
    float64 reference bit for bit, gathered and on this rank's stripe. In
    the allreduce_x0 jobs the new features of a step that follows one with
    no readout arrive while that step's collective is pending: the drain at
    the top of _spmm_step. Returns (mismatching elements, plans)."""
    decomp = ecr.exact_decomposition(case.shape)
    arrow = build(comm, decomp, case.shape, case.precision, case.k, device)
    set_options(arrow, case.options)
    check_structure(arrow, case, device)
    plans = plans_of(arrow, case.precision, case.k) if device == 'gpu' else []
    eng0, perm0, dt = arrow.engines[0], decomp[0][1], np_dtype(case.precision)
    w = eng0.width
    mismatch = 0
    for step in range(ecr.EXACT_STEPS):
        X = ecr.exact_features(case.shape, case.k, step)
        eng0.set_features(stripe(eng0, X[perm0], dt))
        arrow.step()
        if not reads_out(case, step):
            if device == 'gpu' and not eng0._pending_x0_works \
                    and 'ARROW_X0_DEFER' not in case.variables:
                errors.append(f"exact step {step}: nothing was deferred")
            continue
        C = arrow.B.allgather_result()
        G = ecr.exact_reference(case.shape, case.k, step)
        ref = G.astype(dt)
        assert (ref.astype(np.float64) == G).all() and np.abs(G).max() > 0
        assert C.dtype == dt and C.shape == ref.shape
        own_ref = ref[eng0.first_block * w:eng0.last_block * w]
        for what, got, want in (('gathered', C, ref),
                                ('own stripe', own_result(eng0), own_ref)):
            bad = bits(got) != bits(want)
            if bad.any():
                mismatch += int(bad.sum())
                errors.append(
                    f"exact step {step}, {what}: {int(bad.sum())} of "
                    f"{bad.size} elements differ in rows "
                    f"{np.flatnonzero(bad.any(axis=1))[:8].tolist()}, max "
                    f"|diff| {float(np.abs(got - want).max())}")
    return mismatch, plans


def run_real(comm, case, device, errors):
    """REAL_STEPS steps with X := C. Returns (worst err / bound, digests of
    the gathered result per step, plans)."""
    decomp = ecr.decomposition(case.shape)
    arrow = build(comm, decomp, case.shape, case.precision, case.k, device)
    set_options(arrow, case.options)
    check_structure(arrow, case, device)
    plans = plans_of(arrow, case.precision, case.k) if device == 'gpu' else []
    eng0, perm0, dt = arrow.engines[0], decomp[0][1], np_dtype(case.precision)
    w, L = eng0.width, arrow.decomposition_length
    A = ecr.real_matrix(case.shape)
    absA = abs(A)
    head = ecr.head_rows(decomp, w)
    deferred = case.options == 'x0'   # the input is read after the step
    worst = [0.0]
    digests = [None] * ecr.REAL_STEPS

    def original(full):
        out = np.empty(full.shape)
        out[perm0] = full
        return out

    def compare(step, what, got, G, bound, rows=slice(None)):
        got = got.astype(np.float64)
        err = np.abs(got - G[perm0][rows])
        b = bound[perm0][rows]
        ratio = float((err / np.maximum(b, 1e-300)).max()) if err.size else 0.0
        print(f"# {case_label(case)} rank {comm.rank} step {step} {what}: "
              f"max err/bound {ratio:.3f}", file=sys.stderr)
        worst[0] = max(worst[0], ratio)
        if not (np.isfinite(got).all() and (err <= b).all()):
            errors.append(f"real step {step}, {what}: max err/bound {ratio}, "
                          f"rows {np.flatnonzero((err > b).any(axis=1))[:8].tolist()}")

    X0 = ecr.real_features(case.shape, case.k, case.precision)
    eng0.set_features(stripe(eng0, X0[perm0], dt))
    Xin = X0.astype(np.float64)
    unread = None                 # (step, golden, bound) of a step not read
    own = slice(eng0.first_block * w, eng0.last_block * w)
    for step in range(ecr.REAL_STEPS):
        arrow.step()
        if deferred:
            # what this step consumed: the previous step's result, with rank
            # 0's head as the engine refreshed it
            held = gather_stripes(eng0, eng0.feature_tile())
            if step == 0 and not (bits(held) == bits(X0[perm0])).all():
                errors.append("step 0 did not consume the features set")
            if unread is not None:
                compare(unread[0], 'as consumed by the next step', held,
                        unread[1], unread[2])
                digests[unread[0]] = digest(held)
                unread = None
            Xin = original(held.astype(np.float64))
        G, bound = ecr.step_bound(A, absA, Xin, L, case.precision,
                                  case.world, head)
        assert np.abs(G).max() > 0
        if reads_out(case, step):
            C = arrow.B.allgather_result()
            compare(step, 'gathered', C, G, bound)
            compare(step, 'own stripe', own_result(eng0), G, bound, own)
            digests[step] = digest(C)
            Xin = original(C.astype(np.float64))
        else:
            unread = (step, G, bound)
        eng0.set_features(eng0.result_tile())
    assert unread is None and all(digests)
    return worst[0], digests, plans


def case_label(case):
    return ecr.case_name(case)


def agree(comm, errors):
    """Every rank learns whether any rank failed; all of them raise."""
    flags = comm.allgather_int(1 if errors else 0)
    if any(flags):
        failed = [r for r, f in enumerate(flags) if f]
        raise ch.Mismatch('; '.join(errors) if errors
                          else f"failed on ranks {failed}")


def run_case(comm, case, device):
    errors = []
    mismatch, plans = run_exact(comm, case, device, errors)
    worst, digests, plans_real = run_real(comm, case, device, errors)
    agree(comm, errors)
    line = dict(rank=comm.rank, exact_mismatch=mismatch,
                max_err_over_bound=worst,
                plans=sorted(set(plans) | set(plans_real)))
    if case.options == 'x0':
        line['digests'] = digests
    return line


class CollectiveCounter:
    """Counts the calls of every collective of a comm (wrappers, in place)."""
    NAMES = ('barrier', 'bcast_', 'reduce_sum_', 'allreduce_max_',
             'allreduce_sum_', 'alltoallv', 'alltoallv_async',
             'allgather_cat', 'allgather_int', 'alltoall_ints')

    def __init__(self, comm):
        self.calls = 0
        for name in self.NAMES:
            setattr(comm, name, self._counted(getattr(comm, name)))

    def _counted(self, inner):
        def counted(*args, **kwargs):
            self.calls += 1
            return inner(*args, **kwargs)
        return counted


def run_refusal(comm, child):
    """zero_rhs(dtype=torch.bfloat16) on a float32 GPU engine at world 2 is
    refused with the engine's message before any collective is issued; the
    ranks are still in step: one exact step follows."""
    import torch
    from arrow_matrix_amd.comm import TorchDistComm
    case = ecr.cases(child)[0]._replace(precision='float32', options='plain')
    decomp = ecr.exact_decomposition(case.shape)
    counted = TorchDistComm()
    arrow = build(counted, decomp, case.shape, 'float32', case.k, 'gpu')
    counter = CollectiveCounter(counted)
    w = ecr.SHAPES[case.shape]['width']
    errors = []
    for target in (arrow, arrow.engines[0]):
        try:
            target.zero_rhs(w, case.k, dtype=torch.bfloat16)
            errors.append(f"{type(target).__name__}.zero_rhs accepted "
                          f"bfloat16 on a float32 engine")
        except TypeError as e:
            for words in ('zero_rhs(dtype=torch.bfloat16)', 'float32',
                          'fixed when it is constructed'):
                if words not in str(e):
                    errors.append(f"message does not name {words!r}: {e}")
    if counter.calls:
        errors.append(f"{counter.calls} collectives were issued by a refused "
                      f"zero_rhs")
    eng0, perm0 = arrow.engines[0], decomp[0][1]
    X = ecr.exact_features(case.shape, case.k, 0)
    eng0.set_features(stripe(eng0, X[perm0], np.float32))
    arrow.step()
    C = arrow.B.allgather_result()
    ref = ecr.exact_reference(case.shape, case.k, 0).astype(np.float32)
    if not (bits(C) == bits(ref)).all():
        errors.append("the step after the refusal differs from the reference")
    agree(comm, errors)
    return dict(rank=comm.rank, refused=2)


def rank_main(child, device):
    import datetime
    import torch
    import torch.distributed as dist
    variables = ecr.child_variables(child)
    ch.started_with(START_VARS, variables)
    assert set(variables) <= set(START_VARS)
    world = ecr.world_of(child)
    assert int(os.environ['WORLD_SIZE']) == world
    if device == 'gpu':
        ch.open_gpu("the rank engine driver needs a GPU", set_device=False)
        torch.cuda.set_device(0)      # the ranks share one device
    dist.init_process_group('gloo', timeout=datetime.timedelta(
        seconds=ecr.collective_timeout(child)))
    try:
        from arrow_matrix_amd.comm import TorchDistComm
        comm = TorchDistComm()
        assert (comm.rank, comm.size) == (int(os.environ['RANK']), world)
        jobs = [(ecr.case_name(c), lambda c=c: run_case(comm, c, device))
                for c in ecr.cases(child)]
        if ecr.REFUSAL in ecr.job_names(child):
            jobs.append((ecr.REFUSAL, lambda: run_refusal(comm, child)))
        if device != 'gpu':
            jobs = [job for job in jobs if job[0] not in ecr.GPU_ONLY]
        assert [job[0] for job in jobs] == \
            [n for n in ecr.job_names(child)
             if device == 'gpu' or n not in ecr.GPU_ONLY]
        return ch.run_jobs(jobs, {'child': child, 'world': world,
                                  'device': device})
    finally:
        dist.destroy_process_group()


def guarded(fn):
    """fn()'s status; anything it raises is an error of this process, not a
    failed case."""
    try:
        return fn()
    except Exception:
        traceback.print_exc()
        return ch.EXIT_ERRORED


def main(argv):
    role, child = argv[1], argv[2]
    device = argv[3] if len(argv) > 3 else 'gpu'
    assert role in ('launch', 'rank') and device in ('gpu', 'cpu')
    assert child in ecr.CHILDREN, child
    if role == 'launch':
        return launch(child, device)
    return rank_main(child, device)


if __name__ == '__main__':
    sys.exit(guarded(lambda: main(sys.argv)))
