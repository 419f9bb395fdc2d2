"""Runs the affine-step kernel cases of one (precision, environment) on the
GPU, in a process of its own: `python tests/affine_driver.py <precision>
<environment>`, with precision f32, f64 or bf16 and an environment of
spmm_cases_affine.ENVS.

Built on tests/child_harness.py (the job loop, the refusal check, the guarded
buffers, the upload) and the Precision records of tests/spmm_driver.py. The
ARROW_* kernel variables are read once per process, so the child STARTS with
its environment; the scheduler and store form the launch plan reports are
asserted before every launch; one JSON line is printed per case and the
process exits non-zero on the first mismatch.

Per launch: the sentinels around C and around R are intact, R keeps its bits,
X is surrounded by NaN, rows outside row_ids keep their fill, and the result
equals the float64 reference bit for bit (exact class) or to the derived
bound (real class). This is a plain module, not a test file.
"""
import sys

import numpy as np
import torch

if not __package__:         # started as a script: see tests/child_harness.py
    import child_harness  # noqa: F401
from tests import child_harness as ch  # noqa: E402

from arrow_matrix_amd import hip  # noqa: E402
from tests import spmm_cases as sc  # noqa: E402
from tests import spmm_cases_affine as sa  # noqa: E402
from tests import spmm_driver as sd  # noqa: E402
from tests.child_harness import Mismatch  # noqa: E402

R_GUARD = {'f32': 0x5eed5eed, 'f64': 0x5eed5eed, 'bf16': 0x5eed}


def tier_call(prec, tier, blk, xs, C, R, D, acc, k, alpha, gamma, beta):
    """The entry point of the precision and tier ('_affine', '_affine_norm')
    itself, through ctypes, on device addresses or None (the binding's spmm /
    spmm_dual route (1, 0, NULL) to the plain entry point). Returns (rc,
    message)."""
    lib = hip._load()
    fn = getattr(lib, hip._spmm_symbol(len(xs) == 2, tier,
                                       hip._SPMM_SUFFIX[prec.name]))
    rc = fn(*hip._spmm_args(tier, blk._handle, xs, C, R, D, acc, k, alpha,
                            gamma, beta, ch.stream()))
    return rc, lib.arrow_last_error().decode()


def ptr(view):
    return view.data_ptr() if view is not None else None


def affine_call(prec, blk, dual, X0v, X1v, cv, Rv, k, alpha, gamma, beta):
    xs = (ptr(X0v), ptr(X1v)) if dual else (ptr(X0v),)
    return tier_call(prec, '_affine', blk, xs, ptr(cv), ptr(Rv), None, None,
                     k, alpha, gamma, beta)


_blocks = {}
_shared = {}


def block(prec, case):
    key = (case['matrix'], case['kind'], bool(case.get('row_ids')),
           case.get('col_items', 0), case['queue'], case.get('qblocks', 0))
    if key not in _blocks:
        assert case['queue'] is not None    # every case here sets it
        _blocks[key] = ch.upload(prec, case)
    return _blocks[key]


def shared(prec, case):
    """Operands, the plain product and |A| @ |X| of one (matrix, kind, k,
    beta, row_ids): computed once, shared by the (alpha, gamma) pairs and
    both schedulers, and left unchanged."""
    # the capped initialise cases share one product between beta 0 and 1
    op_case = dict(case, beta=0) if case.get('init_capped') else case
    key = (case['matrix'], case['kind'], case['k'], op_case['beta'],
           bool(case.get('row_ids')))
    if key not in _shared:
        if len(_shared) > 2:
            _shared.clear()
        X0, X1, C0, R = sa.operands(prec.name, op_case)
        P = sa.plain_product(prec.name, op_case, X0, X1)
        absP = sa.abs_product(prec.name, op_case, X0, X1) \
            if case['kind'] == 'real' else None
        _, X0v = sd.guarded(prec, prec.bits(X0), prec.x_guard, 'cuda')
        _, X1v = sd.guarded(prec, prec.bits(X1), prec.x_guard, 'cuda')
        for a in (X0, X1, P):
            a.setflags(write=False)
        _shared[key] = (X0, X1, C0, R, P, absP, X0v, X1v)
    return _shared[key]


def checked_plan(prec, env, case):
    """Before a launch: the plan reports the scheduler and store form the
    environment selects, and the matrix has the rows the case is about.
    Returns (matrix, plan, row lengths)."""
    m = sc.matrix(case['matrix'])
    k = case['k']
    plan = hip.spmm_plan(k, int(m['cols'].size), case['queue'],
                         dtype=prec.plan_dtype)
    want = sa.expected_scheduler(env, case['queue'], plan['group'])
    if plan['scheduler'] != want or plan['nt_mode'] != (env != 'nt0'):
        raise Mismatch(f"plan {plan}: expected scheduler {want}")
    lens = np.diff(m['indptr'])
    if case['matrix'] in ('std', 'std_dual', 'zero_rows'):
        assert (lens > sc.SEG_NNZ).any()
    if case.get('init_capped'):
        assert (lens > sc.SEG_NNZ).sum() * k > 4096 * 256
    return m, plan, lens


def run_case(prec, env, case):
    m, plan, lens = checked_plan(prec, env, case)
    k, beta = case['k'], case['beta']
    X0, X1, C0, R, P, absP, X0v, X1v = shared(prec, case)
    rows, ref = sa.reference(prec.name, case, X0, X1, C0, R, product=P)
    untouched = np.setdiff1d(np.arange(C0.shape[0]), rows)
    C0_bits, R_bits = prec.bits(C0), prec.bits(R)
    cbuf, cv = sd.guarded(prec, C0_bits, prec.c_guard, 'cuda')
    rbuf, Rv = sd.guarded(prec, R_bits, R_GUARD[prec.name], 'cuda')
    if not beta:
        cv.fill_(prec.c_fill)
    blk = block(prec, case)
    rc, msg = affine_call(prec, blk, bool(m['n1']), X0v, X1v, cv,
                          Rv if case['has_R'] else None, k, case['alpha'],
                          case['gamma'], beta)
    torch.cuda.synchronize()
    if rc != 0:
        raise Mismatch(f"affine call failed ({rc}): {msg}")
    got = sd.host_bits(prec, cv, C0_bits.shape)
    if not sd.guards_intact(cbuf, prec.c_guard):
        raise Mismatch("sentinels around C were overwritten")
    if not (sd.guards_intact(rbuf, R_GUARD[prec.name])
            and (sd.host_bits(prec, Rv, R_bits.shape) == R_bits).all()):
        raise Mismatch("R or the sentinels around it were written")
    if untouched.size:
        keep = C0_bits[untouched] if beta else sd.fill_bits(prec)
        if not (got[untouched] == keep).all():
            raise Mismatch("rows outside row_ids were written")
    info = {}
    if case['kind'] == 'exact':
        info.update(prec.exact(got[rows], ref, lens))
        if not case['has_R']:
            # (1, 0, NULL): the plain entry point's bits
            if beta:
                cv.copy_(torch.from_numpy(sd._words(prec, C0_bits)))
            else:
                cv.fill_(prec.c_fill)
            fn = blk.spmm_dual if m['n1'] else blk.spmm
            xs = (X0v.data_ptr(), X1v.data_ptr()) if m['n1'] \
                else (X0v.data_ptr(),)
            fn(*xs, cv.data_ptr(), k, beta, ch.stream(),
               feat_dtype=prec.feat_dtype)
            torch.cuda.synchronize()
            if not (sd.host_bits(prec, cv, C0_bits.shape) == got).all():
                raise Mismatch("(1, 0, NULL) differs from the plain entry "
                               "point")
    else:
        bound = sa.real_bound(prec.name, case, X0, X1, C0, R, ref,
                              abs_prod=absP)
        info['max_err_over_bound'] = prec.real(got[rows], ref, bound)
    info.update(scheduler=plan['scheduler'], sentinels='intact')
    return info


# ---------------------------------------------------------------------------
# misuse
# ---------------------------------------------------------------------------

def draw_bits(prec, rng, rows, k):
    """The raw bits of a rows x k operand of small integers."""
    return prec.bits(rng.integers(-8, 9, (rows, k)).astype(
        np.float64 if prec.name == 'f64' else np.float32))


def run_misuse(prec, env):
    """Each broken rule: a negative code, a message naming it, C unchanged
    (nothing is launched)."""
    m, own, other = ch.own_and_other(prec)
    rng = np.random.default_rng(1005)
    # (handle, k, beta, R, words), at alpha 0.5 and gamma 2.0
    rules = [(blk, 8, beta, R, words) for beta in (0, 1)
             for blk, R, words in (
                 (own, 'null', ('R is NULL', 'gamma')),
                 (own, 'c', ('R must not be C',)),
                 (other, 'ok', ('float32', 'float64')))]
    rules.append((own, 8, 2, 'ok', ('beta', '2')))
    if prec.name == 'bf16':
        rules.append((own, 12, 0, 'ok', ('k % 8', '12')))
    for blk, k, beta, R, words in rules:
        C0 = draw_bits(prec, rng, m['rows'], k)
        _, Xv = sd.guarded(prec, draw_bits(prec, rng, m['n0'], k),
                           prec.x_guard, 'cuda')
        cbuf, cv = sd.guarded(prec, C0, prec.c_guard, 'cuda')
        _, Rv = sd.guarded(prec, draw_bits(prec, rng, m['rows'], k),
                           R_GUARD[prec.name], 'cuda')
        Rarg = {'null': None, 'c': cv, 'ok': Rv}[R]
        for dual in (False, True):
            ch.refused(lambda: affine_call(prec, blk, dual, Xv, Xv, cv, Rarg,
                                           k, 0.5, 2.0, beta),
                       words, {'C': (cbuf, cv, prec.c_guard, C0)})
    return dict(sentinels='intact')


# ---------------------------------------------------------------------------
# the tail kernel
# ---------------------------------------------------------------------------

def run_axpby(prec, n, k, pair):
    alpha, gamma, has_R = pair
    C0, R, ref = sa.axpby_case(prec.name, n, k, pair)
    C0_bits, R_bits = prec.bits(C0), prec.bits(R)
    cbuf, cv = sd.guarded(prec, C0_bits, prec.c_guard, 'cuda')
    rbuf, Rv = sd.guarded(prec, R_bits, R_GUARD[prec.name], 'cuda')
    hip.axpby_rows(cv.data_ptr(), Rv.data_ptr() if has_R else 0, n, k, alpha,
                   gamma, ch.stream(), dtype=prec.route_dtype)
    torch.cuda.synchronize()
    if not sd.guards_intact(cbuf, prec.c_guard):
        raise Mismatch("sentinels around C were overwritten")
    if not (sd.guards_intact(rbuf, R_GUARD[prec.name])
            and (sd.host_bits(prec, Rv, R_bits.shape) == R_bits).all()):
        raise Mismatch("R or the sentinels around it were written")
    if n:
        prec.exact(sd.host_bits(prec, cv, C0_bits.shape), ref, np.zeros(n))
    return dict(sentinels='intact')


def axpby_jobs(prec):
    shapes = sa.AXPBY_SHAPES[prec.name]
    jobs = [(n, k, pair) for n, k in shapes[:-1] for pair in sa.EXACT_PAIRS]
    jobs.append((*shapes[-1], sa.EXACT_PAIRS[0]))
    return [(f'axpby_n{n}_k{k}_{sa._pair_tag(pair)}', n, k, pair)
            for n, k, pair in jobs]


def job_names(prec_name, env):
    """Every JSON line the child of (precision, environment) prints."""
    names = [c['name'] for c in sa.gpu_cases(prec_name, env)]
    if env == 'default':
        names += [j[0] for j in axpby_jobs(sd.PRECISIONS[prec_name])]
        names.append('misuse')
    return names


def main(argv):
    prec, env = sd.PRECISIONS[argv[1]], argv[2]
    ch.started_with(sc.KERNEL_VARS, sa.ENVS[env])
    ch.open_gpu("the affine driver needs a HIP GPU")

    jobs = [(c['name'], lambda c=c: run_case(prec, env, c))
            for c in sa.gpu_cases(prec.name, env)]
    if env == 'default':
        jobs += [(name, lambda n=n, k=k, pair=pair: run_axpby(prec, n, k, pair))
                 for name, n, k, pair in axpby_jobs(prec)]
        jobs.append(('misuse', lambda: run_misuse(prec, env)))
    return ch.run_jobs(jobs, {'env': env})


if __name__ == '__main__':
    sys.exit(main(sys.argv))
