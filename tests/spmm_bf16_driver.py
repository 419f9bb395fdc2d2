"""Runs one entry of spmm_cases_bf16.env_table() on the GPU, in a process of
its own: `python tests/spmm_bf16_driver.py <case-set>`.

The bfloat16-feature twin of spmm_f64_driver.py: the ARROW_* kernel variables
are read once per process, so a variant can only be selected by the
environment this process STARTS with (test_gpu_bf16_kernels.py starts one
child per entry). For every case the launch plan is asserted first, from
arrow_spmm_plan_bf16, and then the result; the sentinels around C are checked
after every launch; one JSON line is printed per case and the process exits
non-zero on the first mismatch. This is a plain module, not a test file.
"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import spmm_cases as sc  # noqa: E402
from tests import spmm_cases_bf16 as s16  # noqa: E402

PAD = 64                 # guard int16 words (128 B) around every view
X_GUARD = 0x7fc1         # a bf16 NaN: a read outside X poisons the result
C_GUARD = 0x4b1d         # must be unchanged after every launch
C_FILL = 0x7fd2          # bf16 NaN pre-fill of C at beta=0


class Mismatch(AssertionError):
    pass


def guarded(torch, bits, guard):
    """A device copy of the raw bf16 `bits` (uint16) as a torch.bfloat16
    view into a larger int16 buffer with PAD sentinel words on either side;
    the view, and so every row (k % 8 == 0), stays 16-byte aligned."""
    assert bits.dtype == np.uint16
    n = bits.size
    buf = torch.full((n + 2 * PAD,), guard, dtype=torch.int16, device='cuda')
    view = buf[PAD:PAD + n].view(bits.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)))
    assert view.data_ptr() % 16 == 0
    return buf, view


def guards_intact(buf, guard):
    return bool((buf[:PAD] == guard).all().item()
                and (buf[-PAD:] == guard).all().item())


def host_bits(view):
    return view.cpu().numpy().view(np.uint16)


def check_plan(hip, case, nnz):
    got = hip.spmm_plan(case['k'], nnz,
                        -1 if case['queue'] is None else case['queue'],
                        dtype='bfloat16')
    if got != case['plan']:
        raise Mismatch(f"plan {got} != expected {case['plan']}")
    return got


_ref_cache = {}


def reference(case, X0, X1, C0):
    key = (case['matrix'], case['kind'], case['k'], case['beta'],
           bool(case.get('row_ids')))
    if key not in _ref_cache:
        _ref_cache.clear()       # consecutive cases share it; keep one
        _ref_cache[key] = s16.reference(case, X0, X1, C0)
    return _ref_cache[key]


def launch(hip, torch, case, m, X0v, X1v, C0, remap):
    """One upload + launch; returns (C bits as numpy, guards intact)."""
    k, beta = case['k'], case['beta']
    cbuf, cv = guarded(torch, s16.bf16_bits(C0), C_GUARD)
    if not beta:
        cv.fill_(C_FILL)
    blk = hip.CsrBlockGPU(
        arrays=((m['rows'], m['n0']), m['indptr'], m['cols'], m['vals']),
        row_ids=sc.row_ids(case), col_items=case.get('col_items', 0))
    # one resident fp32 copy of A serves bf16 features
    assert hip._load().arrow_csr_dtype(blk._handle) == 32
    if case['queue'] is not None:
        blk.set_queue(case['queue'])
    blk.set_xcd_remap(remap)
    stream = torch.cuda.current_stream().cuda_stream
    outs = []
    for _ in range(2 if case.get('repeat') else 1):
        if outs:
            cv.copy_(torch.from_numpy(s16.bf16_bits(C0).view(np.int16)))
        if m['n1']:
            blk.spmm_dual(X0v.data_ptr(), X1v.data_ptr(), cv.data_ptr(), k,
                          beta, stream, feat_dtype='bfloat16')
        else:
            blk.spmm(X0v.data_ptr(), cv.data_ptr(), k, beta, stream,
                     feat_dtype=torch.bfloat16)
        torch.cuda.synchronize()
        outs.append(host_bits(cv))
    if len(outs) == 2 and not (outs[0] == outs[1]).all():
        raise Mismatch("two launches of the same inputs differ")
    return outs[-1], guards_intact(cbuf, C_GUARD)


def run_spmm_case(hip, torch, case):
    m = sc.matrix(case['matrix'])
    nnz = int(m['cols'].size)
    plan = check_plan(hip, case, nnz)
    k, beta = case['k'], case['beta']
    items = sc.n_items(m)
    groups_per_block = 256 // plan['group']
    info = {}
    if 'capped_groups_per_block' in case:
        assert groups_per_block == case['capped_groups_per_block']
        if not -(-items // groups_per_block) > plan['grid_cap']:
            raise Mismatch(f"{items} items do not exceed the grid cap")
    if case['matrix'] in ('std', 'std_dual', 'zero_rows'):
        assert (np.diff(m['indptr']) > sc.SEG_NNZ).any()   # split rows

    X0, X1, C0 = s16.operands(case)
    _, X0v = guarded(torch, s16.bf16_bits(X0), X_GUARD)
    _, X1v = guarded(torch, s16.bf16_bits(X1), X_GUARD)
    rows, G = reference(case, X0, X1, C0)
    untouched = np.setdiff1d(np.arange(C0.shape[0]), rows)

    remaps = (False, True) if case.get('remap') == 'both' else (False,)
    outs = []
    for remap in remaps:
        got, intact = launch(hip, torch, case, m, X0v, X1v, C0, remap)
        if not intact:
            raise Mismatch("sentinels around C were overwritten")
        if untouched.size:
            want = s16.bf16_bits(C0[untouched]) if beta else C_FILL
            if not (got[untouched] == want).all():
                raise Mismatch("rows outside row_ids were written")
        got = got[rows]
        if case['kind'] == 'exact':
            want = s16.bf16_bits(G)          # the float64 result, cast once
            bad = int((got != want).sum())
            info['differing'] = bad
            if bad:
                lens = np.diff(m['indptr'])
                worst = np.flatnonzero((got != want).any(axis=1))
                raise Mismatch(
                    f"{bad} elements differ from bf16_RNE of the float64 "
                    f"reference (bit for bit); row lengths of the first: "
                    f"{lens[worst[:8]].tolist()}")
        else:
            bound = s16.real_bound(case, X0, X1, C0, G)
            err = np.abs(s16.bf16_to_f64(got) - G)
            info['max_err_over_bound'] = float(
                (err / np.maximum(bound, 1e-300)).max())
            if not (err <= bound).all():    # NaN fails too
                raise Mismatch("outside the derived bound: max err/bound "
                               f"{info['max_err_over_bound']}")
        outs.append(got)
    if len(outs) == 2 and not (outs[0] == outs[1]).all():
        raise Mismatch("xcd_remap on and off differ")
    info.update(plan=plan, sentinels='intact', items=items, nnz=nnz)
    return info


def run_route_case(hip, torch, op, n, k):
    rc = s16.route_case(op, n, k)
    stream = torch.cuda.current_stream().cuda_stream
    _, src = guarded(torch, rc['src'], X_GUARD)
    dbuf, dst = guarded(torch, rc['dst0'], C_GUARD)
    idx = {key: torch.from_numpy(rc[key]).cuda()
           for key in ('src_idx', 'dst_idx') if rc[key] is not None}
    bf = dict(dtype=torch.bfloat16)
    if op == 'gather':
        hip.gather_rows(src.data_ptr(), dst.data_ptr(),
                        idx['src_idx'].data_ptr(), n, k, stream, **bf)
    elif op in ('scatter', 'scatter_add'):
        fn = hip.scatter_rows if op == 'scatter' else hip.scatter_add_rows
        fn(dst.data_ptr(), src.data_ptr(), idx['dst_idx'].data_ptr(), n, k,
           stream, **bf)
    else:
        fn = hip.permute_rows if op == 'permute' else hip.permute_add_rows
        fn(dst.data_ptr(), src.data_ptr(), idx['dst_idx'].data_ptr(),
           idx['src_idx'].data_ptr(), n, k, stream, **bf)
    torch.cuda.synchronize()
    if not guards_intact(dbuf, C_GUARD):
        raise Mismatch("sentinels around dst were overwritten")
    # bit for bit; rows outside the index set keep dst0's bits
    if not (host_bits(dst) == rc['ref']).all():
        raise Mismatch("differs from the reference, bit for bit")
    return dict(sentinels='intact')


def run_misuse(hip, torch):
    """A float64 handle at arrow_spmm_bf16 / arrow_spmm_dual_bf16, and
    k = 12 on a float32 handle, through ctypes: a negative code, a message
    naming the reason, and C keeps its bits (nothing is launched)."""
    lib = hip._load()
    m = sc.matrix('std')
    arrays = ((m['rows'], m['n0']), m['indptr'], m['cols'], m['vals'])
    h32 = hip.CsrBlockGPU(arrays=arrays)
    h64 = hip.CsrBlockGPU(arrays=arrays, dtype=np.float64)
    rng = np.random.default_rng(16)
    stream = torch.cuda.current_stream().cuda_stream
    for handle, k, words in ((h64, 8, ('float64', 'bfloat16')),
                             (h32, 12, ('k % 8', '12'))):
        X = s16.bf16_bits(rng.integers(-8, 9, (m['n0'], k)).astype(np.float32))
        C0 = s16.bf16_bits(rng.integers(-8, 9, (m['rows'], k)).astype(np.float32))
        _, Xv = guarded(torch, X, X_GUARD)
        for fn, dual in ((lib.arrow_spmm_bf16, False),
                         (lib.arrow_spmm_dual_bf16, True)):
            for beta in (0, 1):
                cbuf, cv = guarded(torch, C0, C_GUARD)
                xs = (Xv.data_ptr(),) * (2 if dual else 1)
                rc = fn(handle._handle, *xs, cv.data_ptr(), k, beta, stream)
                msg = lib.arrow_last_error().decode()
                torch.cuda.synchronize()
                if not rc < 0:
                    raise Mismatch(f"misuse accepted (rc {rc}, k {k})")
                if not all(w in msg for w in words):
                    raise Mismatch(f"message does not name {words}: {msg!r}")
                if not (guards_intact(cbuf, C_GUARD)
                        and (host_bits(cv) == C0).all()):
                    raise Mismatch("C was written by a refused call")
    return dict(sentinels='intact')


def route_case_names():
    return [f'route_{op}_n{n}_k{k}' for op in sc.ROUTE_OPS
            for n, k in s16.ROUTE_SHAPES]


def main(argv):
    name = argv[1]
    variables, cases = s16.env_table()[name]
    for var in sc.KERNEL_VARS:      # started with exactly this entry's set
        assert os.environ.get(var) == variables.get(var), var

    import torch
    from arrow_matrix_amd import hip
    assert torch.cuda.is_available(), "the bfloat16 driver needs a HIP GPU"
    hip.set_device(torch.cuda.current_device())

    jobs = [(c['name'], c, lambda c=c: run_spmm_case(hip, torch, c))
            for c in cases]
    if name == 'default':
        jobs += [(f'route_{op}_n{n}_k{k}', dict(op=op, n=n, k=k),
                  lambda op=op, n=n, k=k: run_route_case(hip, torch, op, n, k))
                 for op in sc.ROUTE_OPS for n, k in s16.ROUTE_SHAPES]
        jobs.append(('misuse', {}, lambda: run_misuse(hip, torch)))
    for cname, spec, job in jobs:
        line = {'case': cname, 'env': name}
        line.update({key: spec[key] for key in
                     ('matrix', 'kind', 'k', 'beta', 'queue', 'op', 'n')
                     if key in spec})
        t0 = time.perf_counter()
        try:
            line.update(job())
            line['ok'] = True
        except AssertionError as e:
            line.update(ok=False, error=str(e)[:2000])
        line['ms'] = round(1e3 * (time.perf_counter() - t0), 1)
        print(json.dumps(line), flush=True)
        if not line['ok']:
            return 1
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
