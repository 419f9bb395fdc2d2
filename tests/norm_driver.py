"""Runs the step-norm kernel cases of one (precision, environment) on the GPU,
in a process of its own: `python tests/norm_driver.py <precision>
<environment>`, with precision f32, f64 or bf16 and an environment of
spmm_cases_norm.ENVS. Built on tests/child_harness.py (the job loop, the
refusal check, the guarded buffers) and tests/affine_driver.py (blocks,
shared operands, the plan check, the entry-point call).

Per launch: the plan reports the scheduler the environment selects; C from
the measuring entry point equals C from the affine entry point bit for bit
(exact class: and the float64 reference); the sentinels around C, D and the
accumulator pair are intact and D keeps its bits; rows outside row_ids keep
their NaN fill; and the two accumulators equal the host's float64 sums over
the device's OWN C and D as read back: bit for bit in the fp32 / bf16 exact
class, to spmm_cases_norm.norm_bound otherwise. This is a plain module, not a
test file.
"""
import sys

import numpy as np
import torch

if not __package__:         # started as a script: see tests/child_harness.py
    import child_harness  # noqa: F401
from tests import child_harness as ch  # noqa: E402

from arrow_matrix_amd import hip  # noqa: E402
from tests import affine_driver as ad  # noqa: E402
from tests import spmm_cases as sc  # noqa: E402
from tests import spmm_cases_norm as sn  # noqa: E402
from tests import spmm_driver as sd  # noqa: E402
from tests.child_harness import Mismatch  # noqa: E402

D_GUARD = {'f32': 0x0d0d0d0d, 'f64': 0x0d0d0d0d, 'bf16': 0x0d0d}
ACC_PAD = 8          # sentinels either side of the two doubles


def values(prec, bits):
    """Raw bits (spmm_driver's) as float64 values."""
    if prec.name == 'f64':
        return bits.view(np.float64)
    if prec.name == 'f32':
        return bits.view(np.float32).astype(np.float64)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def acc_buffer(init=(0.0, 0.0)):
    """(buffer, view): two doubles between ACC_PAD sentinels each side."""
    return ch.guarded_f64(init, ACC_PAD)


def norm_call(prec, blk, dual, X0v, X1v, cv, Rv, Dv, accv, k, alpha, gamma,
              beta):
    """The measuring entry point of the precision, through ctypes. Returns
    (rc, message)."""
    xs = (ad.ptr(X0v), ad.ptr(X1v)) if dual else (ad.ptr(X0v),)
    return ad.tier_call(prec, '_affine_norm', blk, xs, ad.ptr(cv), ad.ptr(Rv),
                        ad.ptr(Dv), ad.ptr(accv), k, alpha, gamma, beta)


def check_acc(prec, case, got_acc, c, d, calls=1):
    """got_acc against the host sums over c and d (float64 values of the
    read-back C rows and D rows); returns the figures."""
    if case['kind'] == 'exact' and prec.name != 'f64':
        want = tuple(calls * s for s in sn.exact_sums(c, d))
        if tuple(got_acc) != want:
            raise Mismatch(f"accumulators {tuple(got_acc)} != exact {want}")
        return dict(acc=list(want))
    s0, s1 = sn.host_sums(c, d)
    b0, b1 = sn.norm_bound(prec.name, c.size, s0, s1)
    e0, e1 = abs(got_acc[0] - calls * s0), abs(got_acc[1] - calls * s1)
    info = dict(acc=list(map(float, got_acc)), host=[s0, s1],
                err=[e0, e1], bound=[calls * b0, calls * b1])
    if not (e0 <= calls * b0 and e1 <= calls * b1):
        raise Mismatch(f"accumulators outside the bound: {info}")
    return info


def run_case(prec, env, case):
    m, plan, lens = ad.checked_plan(prec, env, case)
    k = case['k']
    X0, X1, C0, R, P, absP, X0v, X1v = ad.shared(prec, case)
    rows, ref = ad.sa.reference(prec.name, case, X0, X1, C0, R, product=P)
    untouched = np.setdiff1d(np.arange(C0.shape[0]), rows)
    C0_bits, R_bits = prec.bits(C0), prec.bits(R)
    cbuf, cv = sd.guarded(prec, C0_bits, prec.c_guard, 'cuda')
    _, Rv = sd.guarded(prec, R_bits, ad.R_GUARD[prec.name], 'cuda')
    Rarg = Rv if case['has_R'] else None
    dual = bool(m['n1'])
    blk = ad.block(prec, case)

    # D: its own buffer, NULL, or an operand the call already reads
    alias = None
    if case.get('D') == 'null':
        D_bits, dbuf, Dv = None, None, None
    elif case.get('D') == 'alias':
        if m['rows'] == m['n0'] and X0.shape == C0.shape:
            alias, D_bits, Dv = 'X0', prec.bits(X0), X0v
        else:
            alias, D_bits, Dv = 'R', R_bits, Rv
        dbuf = None
    else:
        D_bits = prec.bits(sn.operand_D(prec.name, case))
        dbuf, Dv = sd.guarded(prec, D_bits, D_GUARD[prec.name], 'cuda')

    # the affine entry point's C, for the bit-for-bit identity
    cv.fill_(prec.c_fill)
    rc, msg = ad.affine_call(prec, blk, dual, X0v, X1v, cv, Rarg, k,
                             case['alpha'], case['gamma'], 0)
    torch.cuda.synchronize()
    if rc != 0:
        raise Mismatch(f"affine call failed ({rc}): {msg}")
    affine_bits = sd.host_bits(prec, cv, C0_bits.shape).copy()

    abuf, accv = acc_buffer()
    calls = 2 if case.get('twice') else 1
    for _ in range(calls):      # the second call adds: no re-zeroing
        cv.fill_(prec.c_fill)
        rc, msg = norm_call(prec, blk, dual, X0v, X1v, cv, Rarg, Dv, accv, k,
                            case['alpha'], case['gamma'], 0)
        torch.cuda.synchronize()
        if rc != 0:
            raise Mismatch(f"norm call failed ({rc}): {msg}")
    got = sd.host_bits(prec, cv, C0_bits.shape)
    got_acc = accv.cpu().numpy()
    if not sd.guards_intact(cbuf, prec.c_guard):
        raise Mismatch("sentinels around C were overwritten")
    if not ch.f64_guards_intact(abuf):
        raise Mismatch("sentinels around the accumulators were overwritten")
    if dbuf is not None and not (
            sd.guards_intact(dbuf, D_GUARD[prec.name])
            and (sd.host_bits(prec, Dv, D_bits.shape) == D_bits).all()):
        raise Mismatch("D or the sentinels around it were written")
    if untouched.size and not (got[untouched] == sd.fill_bits(prec)).all():
        raise Mismatch("rows outside row_ids were written")
    if not (got == affine_bits).all():
        raise Mismatch("C differs from the affine entry point's")
    info = {}
    if case['kind'] == 'exact':
        info.update(prec.exact(got[rows], ref, lens))
    c = values(prec, got[rows])
    d = None if D_bits is None else values(prec, D_bits[rows])
    info.update(check_acc(prec, case, got_acc, c, d, calls))
    if D_bits is None:
        # equal: bit for bit where the sums are exact (fp32 / bf16). float64
        # squares are inexact and each accumulator's atomics land in an order
        # of their own, so there the two agree as two sums of the same terms
        # do, each within its derived bound of the one host sum (measured on
        # an MI355X: 21164106.31275159 against 21164106.312751587, one ulp)
        slack = sum(info['bound']) if 'bound' in info else 0.0
        if abs(got_acc[0] - got_acc[1]) > slack:
            raise Mismatch(f"D = NULL: acc[0] {got_acc[0]} != acc[1] "
                           f"{got_acc[1]} (allowed {slack})")
    if alias:
        info['alias'] = alias
    info.update(scheduler=plan['scheduler'], sentinels='intact')
    return info


# ---------------------------------------------------------------------------
# misuse
# ---------------------------------------------------------------------------

def run_misuse(prec, env):
    """Each broken rule: a negative code, a message naming it, C and the
    accumulators unchanged (nothing is launched)."""
    m, own, other = ch.own_and_other(prec)
    rng = np.random.default_rng(1006)
    # (handle, k, beta, R, D, acc given, words), at alpha 0.5 and gamma 2.0
    rules = [(own, 8, 0, 'ok', 'ok', False, ('acc is NULL',)),
             (own, 8, 0, 'ok', 'c', True, ('D must not be C',)),
             (own, 8, 1, 'ok', 'ok', True, ('beta must be 0', '1')),
             (own, 8, 2, 'ok', 'ok', True, ('beta must be 0', '2')),
             (own, 8, 0, 'null', 'ok', True, ('R is NULL', 'gamma')),
             (own, 8, 0, 'c', 'ok', True, ('R must not be C',)),
             (other, 8, 0, 'ok', 'ok', True, ('float32', 'float64'))]
    if prec.name == 'bf16':
        rules.append((own, 12, 0, 'ok', 'ok', True, ('k % 8', '12')))
    for blk, k, beta, R, D, acc, words in rules:
        C0 = ad.draw_bits(prec, rng, m['rows'], k)
        _, Xv = sd.guarded(prec, ad.draw_bits(prec, rng, m['n0'], k),
                           prec.x_guard, 'cuda')
        cbuf, cv = sd.guarded(prec, C0, prec.c_guard, 'cuda')
        _, Rv = sd.guarded(prec, ad.draw_bits(prec, rng, m['rows'], k),
                           ad.R_GUARD[prec.name], 'cuda')
        _, Dv = sd.guarded(prec, ad.draw_bits(prec, rng, m['rows'], k),
                           D_GUARD[prec.name], 'cuda')
        abuf, accv = acc_buffer((3.5, -2.25))
        Rarg = {'null': None, 'c': cv, 'ok': Rv}[R]
        Darg = {'c': cv, 'ok': Dv}[D]
        for dual in (False, True):
            ch.refused(lambda: norm_call(prec, blk, dual, Xv, Xv, cv, Rarg,
                                         Darg, accv if acc else None, k, 0.5,
                                         2.0, beta),
                       words, {'C': (cbuf, cv, prec.c_guard, C0),
                               'acc': (abuf, accv, ch.F64_GUARD,
                                       [3.5, -2.25])})
    return dict(sentinels='intact')


# ---------------------------------------------------------------------------
# the stand-alone pass
# ---------------------------------------------------------------------------

def run_diffnorm(prec, n, k, with_D):
    C, D = sn.diffnorm_case(prec.name, n, k)
    C_bits, D_bits = prec.bits(C), prec.bits(D)
    cbuf, cv = sd.guarded(prec, C_bits, prec.c_guard, 'cuda')
    dbuf, Dv = sd.guarded(prec, D_bits, D_GUARD[prec.name], 'cuda')
    abuf, accv = acc_buffer()
    hip.diffnorm_rows(cv.data_ptr(), Dv.data_ptr() if with_D else 0, n, k,
                      accv.data_ptr(), ch.stream(), dtype=prec.route_dtype)
    torch.cuda.synchronize()
    for buf, view, bits, guard in ((cbuf, cv, C_bits, prec.c_guard),
                                   (dbuf, Dv, D_bits, D_GUARD[prec.name])):
        if not (sd.guards_intact(buf, guard)
                and (sd.host_bits(prec, view, bits.shape) == bits).all()):
            raise Mismatch("an input or the sentinels around it were written")
    if not ch.f64_guards_intact(abuf):
        raise Mismatch("sentinels around the accumulators were overwritten")
    got = tuple(accv.cpu().tolist())
    # integers: exact in every precision, float64 included
    want = sn.exact_sums(C, D if with_D else None) if n else (0.0, 0.0)
    if got != want:
        raise Mismatch(f"accumulators {got} != exact {want}")
    return dict(acc=list(want), sentinels='intact')


def diffnorm_jobs(prec):
    shapes = sn.DIFFNORM_SHAPES[prec.name]
    jobs = [(n, k, with_D) for n, k in shapes[:-1] for with_D in (True, False)]
    jobs.append((*shapes[-1], True))
    return [(f'diffnorm_n{n}_k{k}_d{int(with_D)}', n, k, with_D)
            for n, k, with_D in jobs]


def job_names(prec_name, env):
    """Every JSON line the child of (precision, environment) prints."""
    names = [c['name'] for c in sn.gpu_cases(prec_name, env)]
    if env == 'default':
        names += [j[0] for j in diffnorm_jobs(sd.PRECISIONS[prec_name])]
        names.append('misuse')
    return names


def main(argv):
    prec, env = sd.PRECISIONS[argv[1]], argv[2]
    ch.started_with(sc.KERNEL_VARS, sn.ENVS[env])
    ch.open_gpu("the norm driver needs a HIP GPU")

    jobs = [(c['name'], lambda c=c: run_case(prec, env, c))
            for c in sn.gpu_cases(prec.name, env)]
    if env == 'default':
        jobs += [(name, lambda n=n, k=k, w=w: run_diffnorm(prec, n, k, w))
                 for name, n, k, w in diffnorm_jobs(prec)]
        jobs.append(('misuse', lambda: run_misuse(prec, env)))
    return ch.run_jobs(jobs, {'env': env})


if __name__ == '__main__':
    sys.exit(main(sys.argv))
