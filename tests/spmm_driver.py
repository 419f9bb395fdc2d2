"""Runs one entry of a precision's env_table() on the GPU, in a process of its
own: `python tests/spmm_driver.py <precision> <case-set>`, with precision
f32, f64 or bf16.

The ARROW_* kernel variables are read once per process, so a variant can only
be selected by the environment this process STARTS with (the test_gpu_*
kernel modules start one child per entry, through tests/gpu_children.py).
For every case the launch plan is asserted first, from the precision's
arrow_spmm_plan, and then the result; the sentinels around C are checked
after every launch; one JSON line is printed per case and the process exits
non-zero on the first mismatch.

Everything is written once. What differs between the precisions is the data
of a Precision record, as Prec<T> holds it for the kernels; the job loop, the
refusal check, the guarded buffers and the upload are tests/child_harness.py's,
shared with every other driver. This is a plain module, not a test file.
"""
import dataclasses
import sys
from typing import Any, Callable

import numpy as np
import torch

if not __package__:         # started as a script: see tests/child_harness.py
    import child_harness  # noqa: F401
from tests import child_harness as ch  # noqa: E402

from arrow_matrix_amd import hip  # noqa: E402
from tests import spmm_cases as sc  # noqa: E402
from tests import spmm_cases_bf16 as s16  # noqa: E402
from tests import spmm_cases_f64 as s64  # noqa: E402
# the guarded buffers and Mismatch are the harness's, used through this module
from tests.child_harness import (  # noqa: E402,F401
    PAD, Mismatch, _words, fill_bits, guarded, guards_intact, host_bits)


# ---------------------------------------------------------------------------
# what differs between the precisions
# ---------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class Precision:
    name: str
    cases: Any               # the case module: env_table, operands, route_case
    plan_dtype: Any          # passed to hip.spmm_plan
    feat_dtype: Any          # passed to spmm / spmm_dual (None: A's own)
    route_dtype: Any         # passed to the route calls
    struct_dtype: Any        # of the resident A
    check_block: Callable    # asserted on every new CsrBlockGPU
    word: str                # guard-buffer word type (torch and numpy name)
    x_guard: int             # NaN: a read outside X poisons the result
    c_guard: int             # must be unchanged after every launch
    c_fill: int              # NaN pre-fill of C at beta=0
    bits: Callable           # host array -> its raw bits, one int per element
    bits_dtype: str          # the numpy type of those ints
    a_values: Callable       # (case, matrix dict) -> A's values
    reference: Callable      # (case, X0, X1, C0) -> (touched rows, ref)
    bound: Callable          # (case, X0, X1, C0, ref) -> per-element bound
    exact: Callable          # (got bits, ref, row lengths); raises Mismatch
    real: Callable           # (got bits, ref, bound) -> max err/bound; raises
    route_shapes: Any
    split_row_matrices: tuple = ()     # asserted to hold split rows
    extra_jobs: tuple = ()             # (name, function) of the default set

    @property
    def words_per_element(self):
        return np.dtype(self.bits_dtype).itemsize // np.dtype(self.word).itemsize


# ---------------------------------------------------------------------------
# one case
# ---------------------------------------------------------------------------

def check_plan(prec, case, nnz):
    got = hip.spmm_plan(case['k'], nnz,
                        -1 if case['queue'] is None else case['queue'],
                        dtype=prec.plan_dtype)
    if got != case['plan']:
        raise Mismatch(f"plan {got} != expected {case['plan']}")
    return got


_ref_cache = {}


def reference(prec, case, X0, X1, C0):
    key = (prec.name, case['matrix'], case['kind'], case['k'], case['beta'],
           bool(case.get('row_ids')), str(case.get('legacy')))
    if key not in _ref_cache:
        _ref_cache.clear()       # consecutive cases share it; keep one
        _ref_cache[key] = prec.reference(case, X0, X1, C0)
    return _ref_cache[key]


def launch(prec, case, m, X0v, X1v, C0_bits, remap):
    """One upload + launch (two with 'repeat'); returns (C's bits as numpy,
    guards intact)."""
    k, beta = case['k'], case['beta']
    cbuf, cv = guarded(prec, C0_bits, prec.c_guard, 'cuda')
    blk = ch.upload(prec, case, m)
    blk.set_xcd_remap(remap)
    stream = ch.stream()
    outs = []
    for _ in range(2 if case.get('repeat') else 1):
        if not beta:
            cv.fill_(prec.c_fill)
        elif outs:
            cv.copy_(torch.from_numpy(_words(prec, C0_bits)))
        if m['n1']:
            blk.spmm_dual(X0v.data_ptr(), X1v.data_ptr(), cv.data_ptr(), k,
                          beta, stream, feat_dtype=prec.feat_dtype)
        else:
            blk.spmm(X0v.data_ptr(), cv.data_ptr(), k, beta, stream,
                     feat_dtype=prec.feat_dtype)
        torch.cuda.synchronize()
        outs.append(host_bits(prec, cv, C0_bits.shape))
    if len(outs) == 2 and not (outs[0] == outs[1]).all():
        raise Mismatch("two launches of the same inputs differ")
    return outs[-1], guards_intact(cbuf, prec.c_guard)


def run_spmm_case(prec, case):
    m = sc.matrix(case['matrix'])
    nnz = int(m['cols'].size)
    plan = check_plan(prec, case, nnz)
    k, beta = case['k'], case['beta']
    items = sc.n_items(m)
    lens = np.diff(m['indptr'])
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
        assert (lens > sc.SEG_NNZ).sum() * k > 4096 * 256
    if case['matrix'] in prec.split_row_matrices:
        assert (lens > sc.SEG_NNZ).any()

    X0, X1, C0 = prec.cases.operands(case)
    _, X0v = guarded(prec, prec.bits(X0), prec.x_guard, 'cuda')
    _, X1v = guarded(prec, prec.bits(X1), prec.x_guard, 'cuda')
    C0_bits = prec.bits(C0)
    rows, ref = reference(prec, case, X0, X1, C0)
    untouched = np.setdiff1d(np.arange(C0.shape[0]), rows)

    remaps = (False, True) if case.get('remap') == 'both' else (False,)
    outs = []
    for remap in remaps:
        got, intact = launch(prec, case, m, X0v, X1v, C0_bits, remap)
        if not intact:
            raise Mismatch("sentinels around C were overwritten")
        if untouched.size:
            want = C0_bits[untouched] if beta else fill_bits(prec)
            if not (got[untouched] == want).all():
                raise Mismatch("rows outside row_ids were written")
        got = got[rows]
        if case['kind'] == 'exact':
            info.update(prec.exact(got, ref, lens))
        else:
            bound = prec.bound(case, X0, X1, C0, ref)
            info['max_err_over_bound'] = prec.real(got, ref, bound)
            if case['kind'] == 'legacy':    # the original test's own check
                _, ref32 = prec.cases.reference(case, X0, X1, C0,
                                                dtype=np.float32)
                tol = case['legacy']['tol']
                scale = max(1.0, float(np.abs(ref32).max()))
                np.testing.assert_allclose(got.view(np.float32), ref32,
                                           rtol=tol, atol=tol * scale)
        outs.append(got)
    if len(outs) == 2 and not (outs[0] == outs[1]).all():
        raise Mismatch("xcd_remap on and off differ")
    info.update(plan=plan, sentinels='intact', items=items, nnz=nnz)
    return info


def run_route_case(prec, op, n, k):
    rc = prec.cases.route_case(op, n, k)
    stream = ch.stream()
    _, src = guarded(prec, prec.bits(rc['src']), prec.x_guard, 'cuda')
    dbuf, dst = guarded(prec, prec.bits(rc['dst0']), prec.c_guard, 'cuda')
    idx = {key: torch.from_numpy(rc[key]).cuda()
           for key in ('src_idx', 'dst_idx') if rc[key] is not None}
    dt = dict(dtype=prec.route_dtype)
    if op == 'gather':
        hip.gather_rows(src.data_ptr(), dst.data_ptr(),
                        idx['src_idx'].data_ptr(), n, k, stream, **dt)
    elif op in ('scatter', 'scatter_add'):
        fn = hip.scatter_rows if op == 'scatter' else hip.scatter_add_rows
        fn(dst.data_ptr(), src.data_ptr(), idx['dst_idx'].data_ptr(), n, k,
           stream, **dt)
    else:
        fn = hip.permute_rows if op == 'permute' else hip.permute_add_rows
        fn(dst.data_ptr(), src.data_ptr(), idx['dst_idx'].data_ptr(),
           idx['src_idx'].data_ptr(), n, k, stream, **dt)
    torch.cuda.synchronize()
    if not guards_intact(dbuf, prec.c_guard):
        raise Mismatch("sentinels around dst were overwritten")
    # bit for bit; rows outside the index set keep dst0's bits
    want = prec.bits(rc['ref'])
    if not (host_bits(prec, dst, want.shape) == want).all():
        raise Mismatch("differs from the reference, bit for bit")
    return dict(sentinels='intact')


def route_case_names(prec):
    return [f'route_{op}_n{n}_k{k}' for op in sc.ROUTE_OPS
            for n, k in prec.route_shapes]


# ---------------------------------------------------------------------------
# the two misuse jobs
# ---------------------------------------------------------------------------

def plain_call_refused(prec, fn, handle, dual, Xv, C0_bits, k, words):
    """fn, a plain entry point through ctypes, is refused (ch.refused) for
    beta 0 and 1, and C keeps its bits."""
    lib = hip._load()
    xs = (Xv.data_ptr(),) * (2 if dual else 1)
    for beta in (0, 1):
        cbuf, cv = guarded(prec, C0_bits, prec.c_guard, 'cuda')
        ch.refused(lambda: (fn(handle._handle, *xs, cv.data_ptr(), k, beta,
                               ch.stream()),
                            lib.arrow_last_error().decode()),
                   words, {'C': (cbuf, cv, prec.c_guard, C0_bits)})


def run_handle_misuse(prec):
    """Each precision's handle passed to the other precision's SpMM entry
    point: refused, with a message naming both precisions."""
    lib = hip._load()
    m, h64, h32 = ch.own_and_other(prec)         # a job of f64 alone
    if (lib.arrow_csr_dtype(h32._handle), lib.arrow_csr_dtype(h64._handle)) \
            != (32, 64):
        raise Mismatch("arrow_csr_dtype does not report 32 and 64")
    k = 8
    rng = np.random.default_rng(8)
    X = s64.exact_values(rng, (m['n0'], k))
    C0 = prec.bits(s64.exact_values(rng, (m['rows'], k)))
    _, Xv = guarded(prec, prec.bits(X), prec.x_guard, 'cuda')
    for fn, dual, handle in ((lib.arrow_spmm_f64, False, h32),
                             (lib.arrow_spmm_dual_f64, True, h32),
                             (lib.arrow_spmm, False, h64),
                             (lib.arrow_spmm_dual, True, h64)):
        plain_call_refused(prec, fn, handle, dual, Xv, C0, k,
                           ('float32', 'float64'))
    return dict(sentinels='intact')


def run_bf16_misuse(prec):
    """A float64 handle at arrow_spmm_bf16 / arrow_spmm_dual_bf16, and
    k = 12 on a float32 handle: refused, with a message naming the reason."""
    lib = hip._load()
    m, h32, h64 = ch.own_and_other(prec)         # a job of bf16 alone
    rng = np.random.default_rng(16)
    for handle, k, words in ((h64, 8, ('float64', 'bfloat16')),
                             (h32, 12, ('k % 8', '12'))):
        X = prec.bits(rng.integers(-8, 9, (m['n0'], k)).astype(np.float32))
        C0 = prec.bits(rng.integers(-8, 9, (m['rows'], k)).astype(np.float32))
        _, Xv = guarded(prec, X, prec.x_guard, 'cuda')
        for fn, dual in ((lib.arrow_spmm_bf16, False),
                         (lib.arrow_spmm_dual_bf16, True)):
            plain_call_refused(prec, fn, handle, dual, Xv, C0, k, words)
    return dict(sentinels='intact')


# ---------------------------------------------------------------------------
# comparators: pure numpy, on the raw bits that came back from the device
# ---------------------------------------------------------------------------

def _within(got, ref, bound):
    """The real check, on values widened to the reference's type. Returns
    max err/bound."""
    err = np.abs(got - ref).astype(np.float64)
    worst = float((err / np.maximum(bound, 1e-300)).max()) \
        if bound.any() else 0.0
    if not (err <= bound).all():    # NaN fails too
        raise Mismatch("outside the derived summation bound: "
                       f"max err/bound {worst}")
    return worst


def _exact_f32(got, ref, lens):
    want = ref.astype(np.float32)
    bad = int((got.view(np.float32) != want).sum())     # NaN fails too
    if bad:
        raise Mismatch(f"{bad} elements differ from the float64 reference")
    return {}


def _exact_f64(got, ref, lens):
    bad = int((got != _f64_bits(ref)).sum())    # a NaN's bits differ too
    if bad:
        raise Mismatch(f"{bad} elements differ from the float64 reference "
                       f"(bit for bit)")
    return {}


def _exact_bf16(got, ref, lens):
    want = s16.bf16_bits(ref)            # the float64 result, cast once
    if (got != want).any():
        worst = np.flatnonzero((got != want).any(axis=1))
        raise Mismatch(
            f"{int((got != want).sum())} elements differ from bf16_RNE of "
            f"the float64 reference (bit for bit); row lengths of the "
            f"first: {lens[worst[:8]].tolist()}")
    return dict(differing=0)


def _bf16_bits(a):
    """The cases hold bf16 operands as float32 values, the routes as raw
    bits already."""
    return a if a.dtype == np.uint16 else s16.bf16_bits(a)


def _f64_bits(a):
    assert a.dtype == np.float64
    return np.ascontiguousarray(a).view(np.int64)


def _no_check(blk):
    pass


def _is_f64(blk):
    assert blk.dtype == np.float64


def _serves_bf16(blk):
    # one resident fp32 copy of A serves bf16 features
    assert hip._load().arrow_csr_dtype(blk._handle) == 32


# ---------------------------------------------------------------------------
# the three records
# ---------------------------------------------------------------------------

PRECISIONS = {p.name: p for p in (
    Precision(
        name='f32', cases=sc, plan_dtype=np.float32, feat_dtype=None,
        route_dtype=np.float32, struct_dtype=np.float32,
        check_block=_no_check,
        word='int32', x_guard=0x7fc0dead, c_guard=0x4b1d4b1d,
        c_fill=0x7fc12345,
        bits=lambda a: np.ascontiguousarray(a, dtype=np.float32)
        .view(np.int32), bits_dtype='int32',
        a_values=lambda case, m: (m['real_vals'] if case['kind'] == 'legacy'
                                  else m['vals']),
        reference=sc.reference,
        bound=lambda case, X0, X1, C0, ref: sc.real_bound(case, X0, X1, C0),
        exact=_exact_f32,
        real=lambda got, ref, bound: _within(
            got.view(np.float32).astype(np.float64), ref, bound),
        route_shapes=sc.ROUTE_SHAPES),
    Precision(
        # both int32 words of a guard element hold the guard: 0x7ff8dead
        # twice is a float64 NaN
        name='f64', cases=s64, plan_dtype=np.float64, feat_dtype=None,
        route_dtype=np.float64, struct_dtype=np.float64,
        check_block=_is_f64,
        word='int32', x_guard=0x7ff8dead, c_guard=0x4b1d4b1d,
        c_fill=0x7ff81234,
        bits=_f64_bits, bits_dtype='int64',
        a_values=lambda case, m: s64.values(case['matrix'], case['kind']),
        reference=lambda case, *ops: (
            s64.reference_longdouble if case['kind'] == 'real'
            else s64.reference)(case, *ops),
        bound=lambda case, X0, X1, C0, ref: s64.real_bound(case, X0, X1, C0),
        exact=_exact_f64,
        real=lambda got, ref, bound: _within(
            got.view(np.float64).astype(np.longdouble), ref, bound),
        route_shapes=sc.ROUTE_SHAPES,
        extra_jobs=(('handle_misuse', run_handle_misuse),)),
    Precision(
        name='bf16', cases=s16, plan_dtype='bfloat16', feat_dtype='bfloat16',
        route_dtype=torch.bfloat16, struct_dtype=np.float32,
        check_block=_serves_bf16,
        word='int16', x_guard=0x7fc1, c_guard=0x4b1d, c_fill=0x7fd2,
        bits=_bf16_bits, bits_dtype='uint16',
        a_values=lambda case, m: m['vals'],
        reference=s16.reference,
        bound=s16.real_bound,
        exact=_exact_bf16,
        real=lambda got, ref, bound: _within(s16.bf16_to_f64(got), ref, bound),
        route_shapes=s16.ROUTE_SHAPES,
        split_row_matrices=('std', 'std_dual', 'zero_rows'),
        extra_jobs=(('misuse', run_bf16_misuse),)),
)}


def main(argv):
    prec, name = PRECISIONS[argv[1]], argv[2]
    variables, cases = prec.cases.env_table()[name]
    ch.started_with(sc.KERNEL_VARS, variables)
    ch.open_gpu("the SpMM driver needs a HIP GPU")

    jobs = [(c['name'], lambda c=c: run_spmm_case(prec, c), c) for c in cases]
    if name == 'default':
        jobs += [(f'route_{op}_n{n}_k{k}',
                  lambda op=op, n=n, k=k: run_route_case(prec, op, n, k),
                  dict(op=op, n=n, k=k))
                 for op in sc.ROUTE_OPS for n, k in prec.route_shapes]
        jobs += [(jname, lambda fn=fn: fn(prec))
                 for jname, fn in prec.extra_jobs]
    return ch.run_jobs(jobs, {'env': name})


if __name__ == '__main__':
    sys.exit(main(sys.argv))
