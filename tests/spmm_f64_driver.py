"""Runs one entry of spmm_cases_f64.env_table() on the GPU, in a process of
its own: `python tests/spmm_f64_driver.py <case-set>`.

The float64 twin of spmm_variant_driver.py: the ARROW_* kernel variables are
read once per process, so a variant can only be selected by the environment
this process STARTS with (test_gpu_f64_kernels.py starts one child per
entry). For every case the launch plan is asserted first, from
arrow_spmm_plan_f64, and then the result; one JSON line is printed per case
and the process exits non-zero on the first mismatch. This is a plain
module, not a test file.
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import spmm_cases as sc  # noqa: E402
from tests import spmm_cases_f64 as s64  # noqa: E402

PAD = 64                      # guard int32 words (256 B) around every view
X_GUARD = 0x7ff8dead          # both words: a float64 NaN — a read outside
                              # X poisons the result
C_GUARD = 0x4b1d4b1d          # must be unchanged after every launch
C_FILL = 0x7ff81234           # float64 NaN pre-fill of C at beta=0


class Mismatch(AssertionError):
    pass


def guarded(torch, arr, guard_bits):
    """A device copy of the float64 `arr` as a view into a larger int32
    buffer with PAD sentinel words on either side; the view, and so every
    row of an even-k operand, stays 16-byte aligned."""
    assert arr.dtype == np.float64
    n = 2 * arr.size
    buf = torch.full((n + 2 * PAD,), guard_bits, dtype=torch.int32,
                     device='cuda')
    view = buf[PAD:PAD + n].view(torch.float64).view(arr.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    assert view.data_ptr() % 16 == 0
    if arr.ndim == 2 and arr.shape[1] % 2 == 0:
        assert (arr.shape[1] * 8) % 16 == 0     # every row 16-byte aligned
    return buf, view


def guards_intact(buf, guard_bits):
    return bool((buf[:PAD] == guard_bits).all().item()
                and (buf[-PAD:] == guard_bits).all().item())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def fill_bits(word):
    return np.array([word, word], dtype=np.int32).view(np.int64)[0]


def check_plan(hip, case, nnz):
    got = hip.spmm_plan(case['k'], nnz,
                        -1 if case['queue'] is None else case['queue'],
                        dtype=np.float64)
    if got != case['plan']:
        raise Mismatch(f"plan {got} != expected {case['plan']}")
    return got


_ref_cache = {}


def reference(case, X0, X1, C0):
    key = (case['matrix'], case['kind'], case['k'], case['beta'],
           bool(case.get('row_ids')))
    if key not in _ref_cache:
        _ref_cache.clear()       # consecutive cases share it; keep one
        fn = (s64.reference_longdouble if case['kind'] == 'real'
              else s64.reference)
        _ref_cache[key] = fn(case, X0, X1, C0)
    return _ref_cache[key]


def launch(hip, torch, case, m, X0v, X1v, C0, remap):
    """One upload + launch; returns (C as numpy, guards intact)."""
    k, beta = case['k'], case['beta']
    if beta:
        cbuf, cv = guarded(torch, C0, C_GUARD)
    else:
        cbuf, cv = guarded(torch, np.zeros_like(C0), C_GUARD)
        cv.view(torch.int32).fill_(C_FILL)
    blk = hip.CsrBlockGPU(
        arrays=((m['rows'], m['n0']), m['indptr'], m['cols'],
                s64.values(case['matrix'], case['kind'])),
        row_ids=sc.row_ids(case), col_items=case.get('col_items', 0),
        dtype=np.float64)
    assert blk.dtype == np.float64
    if case['queue'] is not None:
        blk.set_queue(case['queue'])
    if case.get('qblocks'):
        blk.set_qblocks(case['qblocks'])
    blk.set_xcd_remap(remap)
    stream = torch.cuda.current_stream().cuda_stream
    if m['n1']:
        blk.spmm_dual(X0v.data_ptr(), X1v.data_ptr(), cv.data_ptr(), k, beta,
                      stream)
    else:
        blk.spmm(X0v.data_ptr(), cv.data_ptr(), k, beta, stream)
    torch.cuda.synchronize()
    return cv.cpu().numpy(), guards_intact(cbuf, C_GUARD)


def run_spmm_case(hip, torch, case):
    m = sc.matrix(case['matrix'])
    nnz = int(m['cols'].size)
    plan = check_plan(hip, case, nnz)
    k, beta = case['k'], case['beta']
    items = sc.n_items(m)
    groups_per_block = 256 // plan['group']
    info = {}
    if 'capped_groups_per_block' in case:
        # the grid really is capped: the grid-stride loop body iterates
        assert groups_per_block == case['capped_groups_per_block']
        if not -(-items // groups_per_block) > plan['grid_cap']:
            raise Mismatch(f"{items} items do not exceed the grid cap")
        info['blocks_wanted'] = -(-items // groups_per_block)
    if 'grid_mod8' in case:
        blocks = -(-items // groups_per_block)
        assert blocks <= plan['grid_cap']
        if blocks % 8 != case['grid_mod8']:
            raise Mismatch(f"gridDim.x {blocks} % 8 != {case['grid_mod8']}")
        info['grid'] = blocks
    if case.get('zero_rows_capped'):
        assert (np.diff(m['indptr']) > sc.SEG_NNZ).sum() * k > 4096 * 256

    X0, X1, C0 = s64.operands(case)
    _, X0v = guarded(torch, X0, X_GUARD)
    _, X1v = guarded(torch, X1, X_GUARD)
    rows, ref = reference(case, X0, X1, C0)
    untouched = np.setdiff1d(np.arange(C0.shape[0]), rows)

    remaps = (False, True) if case.get('remap') == 'both' else (False,)
    outs = []
    for remap in remaps:
        got, intact = launch(hip, torch, case, m, X0v, X1v, C0, remap)
        assert got.dtype == np.float64
        if not intact:
            raise Mismatch("sentinels around C were overwritten")
        if untouched.size:
            want = bits(C0[untouched]) if beta else fill_bits(C_FILL)
            if not (bits(got[untouched]) == want).all():
                raise Mismatch("rows outside row_ids were written")
        got = got[rows]
        if case['kind'] == 'exact':
            if not (bits(got) == bits(ref)).all():    # NaN fails too
                bad = int((bits(got) != bits(ref)).sum())
                raise Mismatch(f"{bad} elements differ from the float64 "
                               f"reference (bit for bit)")
        else:
            bound = s64.real_bound(case, X0, X1, C0)
            err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
            info['max_err_over_bound'] = float(
                (err / np.maximum(bound, 1e-300)).max()) if bound.any() else 0.0
            if not (err <= bound).all():    # NaN fails too
                raise Mismatch("outside the derived summation bound: "
                               f"max err/bound {info['max_err_over_bound']}")
        outs.append(got)
    if len(outs) == 2 and not (bits(outs[0]) == bits(outs[1])).all():
        raise Mismatch("xcd_remap on and off differ")
    info.update(plan=plan, sentinels='intact', items=items, nnz=nnz)
    return info


def run_route_case(hip, torch, op, n, k):
    rc = s64.route_case(op, n, k)
    stream = torch.cuda.current_stream().cuda_stream
    _, src = guarded(torch, rc['src'], X_GUARD)
    dbuf, dst = guarded(torch, rc['dst0'], C_GUARD)
    idx = {key: torch.from_numpy(rc[key]).cuda()
           for key in ('src_idx', 'dst_idx') if rc[key] is not None}
    f64 = dict(dtype=np.float64)
    if op == 'gather':
        hip.gather_rows(src.data_ptr(), dst.data_ptr(),
                        idx['src_idx'].data_ptr(), n, k, stream, **f64)
    elif op in ('scatter', 'scatter_add'):
        fn = hip.scatter_rows if op == 'scatter' else hip.scatter_add_rows
        fn(dst.data_ptr(), src.data_ptr(), idx['dst_idx'].data_ptr(), n, k,
           stream, **f64)
    else:
        fn = hip.permute_rows if op == 'permute' else hip.permute_add_rows
        fn(dst.data_ptr(), src.data_ptr(), idx['dst_idx'].data_ptr(),
           idx['src_idx'].data_ptr(), n, k, stream, **f64)
    torch.cuda.synchronize()
    if not guards_intact(dbuf, C_GUARD):
        raise Mismatch("sentinels around dst were overwritten")
    # bit for bit; rows outside the index set keep dst0's bits
    if not (bits(dst.cpu().numpy()) == bits(rc['ref'])).all():
        raise Mismatch("differs from the numpy fancy-indexing reference")
    return dict(sentinels='intact')


def run_handle_misuse(hip, torch):
    """Each precision's handle passed to the other precision's SpMM entry
    point, through ctypes: a negative code, a message naming both
    precisions, and C keeps its bits (nothing is launched)."""
    lib = hip._load()
    m = sc.matrix('std')
    arrays = ((m['rows'], m['n0']), m['indptr'], m['cols'], m['vals'])
    h32 = hip.CsrBlockGPU(arrays=arrays)
    h64 = hip.CsrBlockGPU(arrays=arrays, dtype=np.float64)
    if (lib.arrow_csr_dtype(h32._handle), lib.arrow_csr_dtype(h64._handle)) \
            != (32, 64):
        raise Mismatch("arrow_csr_dtype does not report 32 and 64")
    k = 8
    rng = np.random.default_rng(8)
    X = s64.exact_values(rng, (m['n0'], k))
    C0 = s64.exact_values(rng, (m['rows'], k))
    _, Xv = guarded(torch, X, X_GUARD)
    stream = torch.cuda.current_stream().cuda_stream
    for fn, dual, handle in ((lib.arrow_spmm_f64, False, h32),
                             (lib.arrow_spmm_dual_f64, True, h32),
                             (lib.arrow_spmm, False, h64),
                             (lib.arrow_spmm_dual, True, h64)):
        for beta in (0, 1):
            cbuf, cv = guarded(torch, C0, C_GUARD)
            xs = (Xv.data_ptr(), Xv.data_ptr()) if dual else (Xv.data_ptr(),)
            rc = fn(handle._handle, *xs, cv.data_ptr(), k, beta, stream)
            msg = lib.arrow_last_error().decode()
            torch.cuda.synchronize()
            if not rc < 0:
                raise Mismatch(f"wrong-precision handle accepted (rc {rc})")
            if 'float32' not in msg or 'float64' not in msg:
                raise Mismatch(f"message does not name both: {msg!r}")
            if not (guards_intact(cbuf, C_GUARD)
                    and (bits(cv.cpu().numpy()) == bits(C0)).all()):
                raise Mismatch("C was written by a refused call")
    return dict(sentinels='intact')


def route_case_names():
    return [f'route_{op}_n{n}_k{k}' for op in sc.ROUTE_OPS
            for n, k in sc.ROUTE_SHAPES]


def main(argv):
    name = argv[1]
    variables, cases = s64.env_table()[name]
    for var in sc.KERNEL_VARS:      # started with exactly this entry's set
        assert os.environ.get(var) == variables.get(var), var

    import torch
    from arrow_matrix_amd import hip
    assert torch.cuda.is_available(), "the float64 driver needs a HIP GPU"
    hip.set_device(torch.cuda.current_device())

    jobs = [(c['name'], c, lambda c=c: run_spmm_case(hip, torch, c))
            for c in cases]
    if name == 'default':
        jobs += [(f'route_{op}_n{n}_k{k}', dict(op=op, n=n, k=k),
                  lambda op=op, n=n, k=k: run_route_case(hip, torch, op, n, k))
                 for op in sc.ROUTE_OPS for n, k in sc.ROUTE_SHAPES]
        jobs.append(('handle_misuse', {},
                     lambda: run_handle_misuse(hip, torch)))
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
