"""Runs the operator-scaling kernel cases of one precision on the GPU, in a
process of its own: `python tests/scale_driver.py <precision>` with precision
f32 or f64 (default environment). Cases, references and bounds come from
tests/spmm_cases_scale.py; the job loop, the refusal check and the guarded
float64 vectors are tests/child_harness.py's. Prints one JSON line per case.
This is a plain module, not a test file.

Every float64 vector handed to the library sits between sentinels, checked
after each call. Exact class: sums equal the host sums exactly (absolute 0
and 1), a second call doubles them, NULL outputs are skipped, the aliased
col_sum1 == col_sum0 form adds both signs of column into one vector; after
arrow_csr_scale the dual SpMM at k in {1, 4, 16, 128} equals the float64
reference on the host-scaled matrix bit for bit (fp32 handle: bf16 features
too, at k = 16), with NULL factors, and an all-NULL scale changes nothing.
Real class (no split rows, so the launch is deterministic): the SpMM on the
device-scaled handle equals, bit for bit, the SpMM on a second handle
uploaded with the host-rounded values, and the sums are within the bound.
"""
import sys

import numpy as np
import torch

if not __package__:         # started as a script: see tests/child_harness.py
    import child_harness  # noqa: F401
from tests import child_harness as ch  # noqa: E402

from arrow_matrix_amd import hip  # noqa: E402
from tests import spmm_cases as sc  # noqa: E402
from tests import spmm_cases_scale as ss  # noqa: E402
from tests.child_harness import Mismatch  # noqa: E402
from tests.child_harness import f64_guards_intact as intact  # noqa: E402

PAD = 16
TORCH = {'f32': torch.float32, 'f64': torch.float64}


def guarded(values):
    """(buffer, view): a float64 device vector between PAD sentinels."""
    return ch.guarded_f64(values, PAD)


def block(c, prec, vals=None):
    m = ss.matrix(c['matrix'])
    v = ss.values(c, prec) if vals is None else vals
    return hip.CsrBlockGPU(arrays=((m['rows'], m['n0']), m['indptr'],
                                   m['cols'], v),
                           row_ids=ss.row_ids(c), dtype=ss.NP_DTYPE[prec])


def shapes(c):
    return ss.out_rows(c), ss.matrix(c['matrix'])['n0'], ss.n1(c)


def sums_call(blk, views, absolute):
    blk.sums(*(v.data_ptr() if v is not None else 0 for v in views),
             absolute=absolute, stream=ch.stream())
    torch.cuda.synchronize()


def check_sums(c, prec, vals=None):
    """vals: the values the handle is known to hold (default: the case's)."""
    blk = block(c, prec, vals)
    exact = c['kind'] == 'exact'
    bound = ss.sum_bound(c, prec, vals)
    worst = 0.0

    def compare(got, want, b, calls, what):
        nonlocal worst
        err = np.abs(got - calls * want)
        # calls * n terms of total magnitude calls * sum|v|
        b = calls * calls * b
        ok = (err == 0).all() if exact else (err <= b).all()
        if not ok:
            raise Mismatch(f"{c['name']} {what}: max err {err.max()}")
        if not exact:
            worst = max(worst, float((err / np.maximum(b, 1e-300)).max()))

    for absolute in (False, True):
        want = ss.host_sums(c, prec, absolute, vals)
        bufs, views = zip(*(guarded(np.zeros(n)) for n in shapes(c)))
        for calls in (1, 2):            # the second call adds
            sums_call(blk, views, absolute)
            if not intact(*bufs):
                raise Mismatch(f"{c['name']}: sentinels overwritten by sums")
            for j, what in enumerate(('row_sum', 'col_sum0', 'col_sum1')):
                compare(views[j].cpu().numpy(), want[j], bound[j], calls,
                        f"{what} absolute={absolute} calls={calls}")
        # NULL outputs are skipped: each output alone
        for j in range(3):
            bufs, views = zip(*(guarded(np.full(n, 3.0)) for n in shapes(c)))
            sums_call(blk, [v if i == j else None
                            for i, v in enumerate(views)], absolute)
            if not intact(*bufs):
                raise Mismatch(f"{c['name']}: sentinels overwritten by sums")
            for i, v in enumerate(views):
                w = want[i] if i == j else 0.0
                compare(v.cpu().numpy() - 3.0, w, bound[i] + 3.0 * 2.0 ** -52,
                        1, f"output {j} alone, vector {i}")
        # the aliased form: one vector takes both signs of column
        n0, n1 = shapes(c)[1:]
        if n1 <= n0:
            buf, view = guarded(np.zeros(n0))
            sums_call(blk, (None, view, view), absolute)
            both = want[1].copy()
            both[:n1] += want[2]
            b = bound[1].copy()
            b[:n1] += bound[2] + 2.0 ** -53 * np.abs(both[:n1])
            if not intact(buf):
                raise Mismatch(f"{c['name']}: sentinels overwritten (alias)")
            compare(view.cpu().numpy(), both, b, 1, "col_sum1 == col_sum0")
    return dict(max_err_over_bound=worst)


def _feat(prec, feat, X):
    t = torch.from_numpy(X.astype(np.float64)).to('cuda')
    return t.to(torch.bfloat16 if feat == 'bf16' else TORCH[prec]).contiguous()


def spmm(blk, c, prec, feat, X0, X1, k):
    """arrow_spmm_dual into a NaN-filled C; the structure rows as float64."""
    x0, x1 = _feat(prec, feat, X0), _feat(prec, feat, X1)
    C = torch.full((ss.out_rows(c), k), float('nan'), dtype=x0.dtype,
                   device='cuda')
    blk.spmm_dual(x0.data_ptr(), x1.data_ptr(), C.data_ptr(), k, 0,
                  ch.stream(),
                  feat_dtype='bfloat16' if feat == 'bf16' else None)
    torch.cuda.synchronize()
    return C


def check_scale(c, prec):
    m = ss.matrix(c['matrix'])
    r, c0, c1 = ss.factors(c)
    combos = [('all', (r, c0, c1)), ('row_only', (r, None, None)),
              ('cols_only', (None, c0, c1)), ('col0_only', (None, c0, None))]
    info = {}
    for tag, fac in combos:
        blk = block(c, prec)
        bufs, views = zip(*((None, None) if f is None else guarded(f)
                            for f in fac))
        X0, X1 = ss.operands(c, 16)
        before = spmm(blk, c, prec, None, X0, X1, 16)
        blk.scale(0, 0, 0, ch.stream())          # all NULL: nothing changes
        torch.cuda.synchronize()
        again = spmm(blk, c, prec, None, X0, X1, 16)
        if not torch.equal(before.view(torch.uint8), again.view(torch.uint8)):
            raise Mismatch(f"{c['name']}: an all-NULL scale changed the result")
        blk.scale(*(v.data_ptr() if v is not None else 0 for v in views),
                  stream=ch.stream())
        torch.cuda.synchronize()
        if not intact(*(b for b in bufs if b is not None)):
            raise Mismatch(f"{c['name']} {tag}: sentinels overwritten by scale")
        for f, v in zip(fac, views):
            if f is not None and not (v.cpu().numpy() == f).all():
                raise Mismatch(f"{c['name']} {tag}: a factor vector was written")
        want_vals = ss.scaled_values(c, prec, *fac)
        if c['kind'] == 'exact':
            feats = [(None, k) for k in ss.KS]
            if prec == 'f32':
                feats.append(('bf16', 16))
            for feat, k in feats:
                X0, X1 = ss.operands(c, k)
                rows, ref = ss.product(c, want_vals, X0, X1)
                C = spmm(blk, c, prec, feat, X0, X1, k)
                got = C.to(torch.float64).cpu().numpy()
                if feat == 'bf16':      # the one rounding of the result
                    ref = torch.from_numpy(ref).to(torch.bfloat16) \
                        .to(torch.float64).numpy()
                if not (got[rows] == ref).all():
                    raise Mismatch(f"{c['name']} {tag} k={k} feat={feat}: "
                                   f"SpMM on the scaled handle differs from "
                                   f"the reference")
                rest = np.setdiff1d(np.arange(got.shape[0]), rows)
                if not np.isnan(got[rest]).all():
                    raise Mismatch(f"{c['name']}: rows outside row_ids written")
        else:
            other = block(c, prec, want_vals)   # host-rounded values
            for k in (4, 16):
                X0, X1 = ss.operands(c, k)
                a = spmm(blk, c, prec, None, X0, X1, k)
                b = spmm(other, c, prec, None, X0, X1, k)
                if not torch.equal(a.view(torch.uint8), b.view(torch.uint8)):
                    raise Mismatch(f"{c['name']} {tag} k={k}: device-scaled "
                                   f"and host-rounded handles differ")
        info[tag] = 'ok'
    return info


def check_empty(c, prec):
    blk = block(c, prec)
    bufs, views = zip(*(guarded(np.full(n, 3.0)) for n in shapes(c)))
    sums_call(blk, views, False)
    blk.scale(*(v.data_ptr() for v in views), stream=ch.stream())
    torch.cuda.synchronize()
    if not intact(*bufs) or not all((v.cpu().numpy() == 3.0).all()
                                    for v in views):
        raise Mismatch("nnz == 0 is not a no-op")
    return {}


def run_misuse(prec):
    lib = hip._load()
    blk = block(ss.CASES[0], prec)

    def call(fn, *args):
        return lambda: (fn(*args, ch.stream()),
                        lib.arrow_last_error().decode())
    ch.refused(call(lib.arrow_csr_sums, blk._handle, None, None, None, 0),
               ('all NULL',), {})
    buf, view = guarded(np.full(8, 3.0))
    ptrs = (view.data_ptr(),) * 3
    for fn, args in ((lib.arrow_csr_sums, ptrs + (0,)),
                     (lib.arrow_csr_scale, ptrs)):
        ch.refused(call(fn, 1 << 40, *args), ('bad handle',),
                   {'the vector': (buf, view, ch.F64_GUARD, np.full(8, 3.0))})
    return {}


def jobs(prec):
    out = []
    for c in ss.CASES:
        if c['matrix'] == 'empty':
            out.append(('empty', lambda c=c: check_empty(c, prec)))
            continue
        out.append((f"sums_{c['name']}", lambda c=c: check_sums(c, prec)))
        out.append((f"scale_{c['name']}", lambda c=c: check_scale(c, prec)))
    out.append(('misuse', lambda: run_misuse(prec)))
    return out


def job_names(prec):
    return [name for name, _ in jobs(prec)]


def main(argv):
    prec = argv[1]
    ch.started_with(sc.KERNEL_VARS, {})     # the default environment
    ch.open_gpu("the scale driver needs a HIP GPU")
    return ch.run_jobs(jobs(prec), {'prec': prec})


if __name__ == '__main__':
    sys.exit(main(sys.argv))
