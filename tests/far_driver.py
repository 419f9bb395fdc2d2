"""Runs the far-offset cases of one precision on the GPU, in a process of its
own: `python tests/far_driver.py <precision>`, with precision f32, f64 or
bf16 and no ARROW_* kernel variable set. The geometry, the case lists and the
peak-memory figures are tests/spmm_cases_far.py's; the job loop, the guarded
buffers and the upload are tests/child_harness.py's, the Precision records,
plan check and exact comparators tests/spmm_driver.py's, the entry-point call
tests/affine_driver.py's, the accumulators tests/norm_driver.py's.

Per case: the launch plan is asserted; the touched rows equal the compact
reference bit for bit; the sentinels around every buffer are intact; a tall
read buffer holds NaN outside its windows, so a stray read poisons the
result; a tall written buffer is pre-filled, and after the launch EVERY word
outside the rows the case writes still holds the fill: checked on the device
in slices, no tall buffer is ever copied to the host. One JSON line is
printed per case, with torch.cuda.max_memory_allocated() of that case, and
the process exits non-zero on the first mismatch. A failed allocation is a
failed case. This is a plain module, not a test file.
"""
import ctypes
import json
import sys
import time

import numpy as np
import torch

if not __package__:         # started as a script: see tests/child_harness.py
    import child_harness  # noqa: F401
from tests import child_harness as ch  # noqa: E402

from arrow_matrix_amd import hip  # noqa: E402
from tests import affine_driver as ad  # noqa: E402
from tests import norm_driver as nd  # noqa: E402
from tests import spmm_cases as sc  # noqa: E402
from tests import spmm_cases_far as far  # noqa: E402
from tests import spmm_driver as sd  # noqa: E402
from tests.child_harness import Mismatch  # noqa: E402

assert far.PAD == sd.PAD

SLICE_BYTES = 1 << 29          # of a tall buffer per device compare
FORMULA_SLICE = 1 << 22        # elements per int64 formula slice (32 MiB)
TORCH_DTYPE = {'f32': torch.float32, 'f64': torch.float64,
               'bf16': torch.bfloat16}
BITS_DTYPE = {'f32': torch.int32, 'f64': torch.int64, 'bf16': torch.int16}


# ---------------------------------------------------------------------------
# tall buffers: never on the host
# ---------------------------------------------------------------------------

class Tall:
    """The tall buffers of the current case group, at most two; a new group
    frees them first."""

    def __init__(self):
        self.key, self.bufs = None, {}

    def group(self, key):
        if key != self.key:
            self.free()
            self.key = key

    def get(self, prec, name, n_elements, fill, guard):
        """Buffer `name` of n_elements, allocated on first use: every word
        `fill`, PAD words of `guard` on either side."""
        if name not in self.bufs:
            assert len(self.bufs) < 2
            words = n_elements * prec.words_per_element
            buf = torch.full((words + 2 * sd.PAD,), fill,
                             dtype=getattr(torch, prec.word), device='cuda')
            buf[:sd.PAD] = guard
            buf[-sd.PAD:] = guard
            assert buf[sd.PAD:].data_ptr() % 16 == 0
            self.bufs[name] = buf
        return self.bufs[name]

    def free(self):
        self.bufs.clear()
        torch.cuda.empty_cache()


def view_ptr(prec, buf, element=0):
    """Device address of `element` of the view behind the leading guard."""
    itemsize = prec.words_per_element * buf.element_size()
    return buf.data_ptr() + sd.PAD * buf.element_size() + element * itemsize


def _span(prec, element, n_elements):
    lo = sd.PAD + element * prec.words_per_element
    return lo, lo + n_elements * prec.words_per_element


def write_window(prec, buf, element, bits):
    words = sd._words(prec, bits)
    lo, hi = _span(prec, element, bits.size)
    assert hi <= buf.numel() - sd.PAD and hi - lo == words.size
    if not words.flags.writeable:       # torch wants a writable source
        words = words.copy()
    buf[lo:hi].copy_(torch.from_numpy(words))


def fill_window(prec, buf, element, n_elements, value):
    lo, hi = _span(prec, element, n_elements)
    assert hi <= buf.numel() - sd.PAD
    buf[lo:hi] = value


def read_window(prec, buf, element, shape):
    lo, hi = _span(prec, element, int(np.prod(shape)))
    return buf[lo:hi].cpu().numpy().view(prec.bits_dtype).reshape(shape)


def holds_outside(prec, buf, element, n_elements, value):
    """Every word of the view outside [element, element + n_elements) is
    `value`: compared on the device, SLICE_BYTES at a time."""
    lo, hi = _span(prec, element, n_elements)
    step = SLICE_BYTES // buf.element_size()
    ok = torch.ones((), dtype=torch.bool, device='cuda')
    for a, b in ((sd.PAD, lo), (hi, buf.numel() - sd.PAD)):
        for s in range(a, b, step):
            ok &= (buf[s:min(s + step, b)] == value).all()
    return bool(ok.item())


# ---------------------------------------------------------------------------
# the SpMM entry points
# ---------------------------------------------------------------------------

_blocks = {}


def far_block(prec, case, m, pl):
    key = (case['role'], case['k'], case['queue'])
    if key not in _blocks:
        if pl['cols'] is not None:
            m = dict(m, cols=pl['cols'])
        _blocks[key] = ch.upload(prec, case, m, row_ids=pl['row_ids'])
    return _blocks[key]


def run_spmm_case(prec, case, tall):
    m = sc.matrix(case['matrix'])
    plan = sd.check_plan(prec, case, int(m['cols'].size))
    if case['k'] == far.TWO_LAUNCHES[prec.name]:
        assert plan['launches'] == 2
    lens = np.diff(m['indptr'])
    assert (lens > sc.SEG_NNZ).any()
    k, beta, role, entry = case['k'], case['beta'], case['role'], case['entry']
    dual = bool(m['n1'])

    X0, X1, C0, R, P, _, X0v, X1v = ad.shared(prec, case)
    cp = far.compact(prec.name, case, shared=(X0, X1, C0, R, P))
    rows, ref = cp['rows'], cp['ref']
    pl = far.placement(prec.name, case)
    C0_bits, R_bits = prec.bits(C0), prec.bits(R)
    r_guard, d_guard = ad.R_GUARD[prec.name], nd.D_GUARD[prec.name]
    n_out = C0.shape[0]
    checks = []          # (what, function) run after the launch

    if role == 'read':
        xbuf = tall.get(prec, 'X', pl['tall']['X'] * k, prec.x_guard,
                        prec.x_guard)
        for name, arr in (('X0', X0), ('X1', X1)):
            _, first, n = pl['windows'][name]
            assert arr.shape == (n, k)
            write_window(prec, xbuf, first * k, prec.bits(arr))
        x0p = x1p = view_ptr(prec, xbuf)
        cbuf, cv = sd.guarded(prec, C0_bits, prec.c_guard, 'cuda')
        if not beta:
            cv.fill_(prec.c_fill)
        cptr = cv.data_ptr()
        read_c = lambda: sd.host_bits(prec, cv, C0_bits.shape)
        checks.append(("sentinels around C were overwritten",
                       lambda: sd.guards_intact(cbuf, prec.c_guard)))
        rbuf, rv = sd.guarded(prec, R_bits, r_guard, 'cuda')
        rptr = rv.data_ptr()
        checks.append(("R or the sentinels around it were written", lambda: (
            sd.guards_intact(rbuf, r_guard)
            and (sd.host_bits(prec, rv, R_bits.shape) == R_bits).all())))
        D_bits = dptr = None
        if entry == 'norm':
            D_bits = prec.bits(cp['D'])
            dbuf, dv = sd.guarded(prec, D_bits, d_guard, 'cuda')
            dptr = dv.data_ptr()
            checks.append(("D or the sentinels around it were written",
                           lambda: (
                               sd.guards_intact(dbuf, d_guard)
                               and (sd.host_bits(prec, dv, D_bits.shape)
                                    == D_bits).all())))
    else:
        _, out_base, W = pl['windows']['C']
        assert W == n_out
        x0p, x1p = X0v.data_ptr(), X1v.data_ptr()
        ctall = tall.get(prec, 'C', pl['tall']['C'] * k, prec.c_fill,
                         prec.c_guard)
        # C0 goes into the window rows only; the rest keeps the fill
        if beta:
            write_window(prec, ctall, out_base * k, C0_bits)
        else:
            fill_window(prec, ctall, out_base * k, W * k, prec.c_fill)
        cptr = view_ptr(prec, ctall)
        read_c = lambda: read_window(prec, ctall, out_base * k, (W, k))
        checks.append(("sentinels around C were overwritten",
                       lambda: sd.guards_intact(ctall, prec.c_guard)))
        checks.append(("C was written below its window", lambda: holds_outside(
            prec, ctall, out_base * k, W * k, prec.c_fill)))
        rptr = dptr = D_bits = None
        if case['has_R']:
            rtall = tall.get(prec, 'R', pl['tall']['R'] * k, r_guard, r_guard)
            write_window(prec, rtall, out_base * k, R_bits)
            rptr = view_ptr(prec, rtall)
            checks.append(("R or the words around it were written", lambda: (
                sd.guards_intact(rtall, r_guard)
                and holds_outside(prec, rtall, out_base * k, W * k, r_guard)
                and (read_window(prec, rtall, out_base * k, (W, k))
                     == R_bits).all())))
            if entry == 'norm':          # D = R
                assert cp['D'] is R
                D_bits, dptr = R_bits, rptr
    if not case['has_R']:
        rptr = None

    blk = far_block(prec, case, m, pl)
    if entry == 'spmm':
        if dual:
            blk.spmm_dual(x0p, x1p, cptr, k, beta, ch.stream(),
                          feat_dtype=prec.feat_dtype)
        else:
            blk.spmm(x0p, cptr, k, beta, ch.stream(),
                     feat_dtype=prec.feat_dtype)
        rc = 0
    else:
        aptr = None
        if entry == 'norm':
            abuf, accv = nd.acc_buffer()
            aptr = accv.data_ptr()
        rc, msg = ad.tier_call(
            prec, '_affine_norm' if entry == 'norm' else '_affine', blk,
            (x0p, x1p) if dual else (x0p,), cptr, rptr, dptr, aptr, k,
            case['alpha'], case['gamma'], beta)
    torch.cuda.synchronize()
    if rc != 0:
        raise Mismatch(f"{entry} call failed ({rc}): {msg}")

    got = read_c()
    for what, check in checks:
        if not check():
            raise Mismatch(what)
    untouched = np.setdiff1d(np.arange(n_out), rows)
    if untouched.size:
        keep = C0_bits[untouched] if beta else sd.fill_bits(prec)
        if not (got[untouched] == keep).all():
            raise Mismatch("rows outside row_ids were written")
    info = dict(prec.exact(got[rows], ref, lens))
    if entry == 'norm':
        if not ch.f64_guards_intact(abuf):
            raise Mismatch("sentinels around the accumulators were "
                           "overwritten")
        info.update(nd.check_acc(prec, case, accv.cpu().numpy(),
                                 nd.values(prec, got[rows]),
                                 nd.values(prec, D_bits[rows])))
    info.update(plan=plan, sentinels='intact')
    return info


# ---------------------------------------------------------------------------
# the route kernels
# ---------------------------------------------------------------------------

def run_route_case(prec, op, k, side, tall):
    rp = far.route_placement(prec.name, op, k, side)
    rc, base, n = rp['rc'], rp['base'], far.ROUTE_N
    src_bits, dst_bits = prec.bits(rc['src']), prec.bits(rc['dst0'])
    want = prec.bits(rc['ref'])
    rows_tall = rp['tall'][side]
    if side == 'src':
        sbuf = tall.get(prec, 'src', rows_tall * k, prec.x_guard,
                        prec.x_guard)
        write_window(prec, sbuf, base * k, src_bits)
        sptr = view_ptr(prec, sbuf, rp['ptr_row'] * k)
        dbuf, dst = sd.guarded(prec, dst_bits, prec.c_guard, 'cuda')
        dptr = dst.data_ptr()
    else:
        _, sv = sd.guarded(prec, src_bits, prec.x_guard, 'cuda')
        sptr = sv.data_ptr()
        dbuf = tall.get(prec, 'dst', rows_tall * k, prec.c_fill,
                        prec.c_guard)
        write_window(prec, dbuf, base * k, dst_bits)
        dptr = view_ptr(prec, dbuf, rp['ptr_row'] * k)
    idx = {key: rc[key] for key in ('src_idx', 'dst_idx')}
    idx[side + '_idx'] = rp['idx']
    idx = {key: torch.from_numpy(v).cuda() for key, v in idx.items()
           if v is not None}
    dt = dict(dtype=prec.route_dtype)
    if op == 'gather':
        hip.gather_rows(sptr, dptr, idx['src_idx'].data_ptr(), n, k,
                        ch.stream(), **dt)
    elif op in ('scatter', 'scatter_add'):
        fn = hip.scatter_rows if op == 'scatter' else hip.scatter_add_rows
        fn(dptr, sptr, idx['dst_idx'].data_ptr(), n, k, ch.stream(), **dt)
    else:
        fn = hip.permute_rows if op == 'permute' else hip.permute_add_rows
        fn(dptr, sptr, idx['dst_idx'].data_ptr(), idx['src_idx'].data_ptr(),
           n, k, ch.stream(), **dt)
    torch.cuda.synchronize()
    if not sd.guards_intact(dbuf, prec.c_guard):
        raise Mismatch("sentinels around dst were overwritten")
    if side == 'dst':
        got = read_window(prec, dbuf, base * k, want.shape)
        if not holds_outside(prec, dbuf, base * k, want.size, prec.c_fill):
            raise Mismatch("dst was written below its window")
    else:
        got = sd.host_bits(prec, dst, want.shape)
    # bit for bit; rows outside the index set keep dst0's bits
    if not (got == want).all():
        raise Mismatch("differs from the reference, bit for bit")
    return dict(sentinels='intact')


# ---------------------------------------------------------------------------
# the contiguous kernels
# ---------------------------------------------------------------------------

def _typed(prec, buf, total):
    lo, hi = _span(prec, 0, total)
    return buf[lo:hi].view(TORCH_DTYPE[prec.name])


def _slices(total):
    for lo in range(0, total, FORMULA_SLICE):
        hi = min(lo + FORMULA_SLICE, total)
        yield lo, hi, torch.arange(lo, hi, dtype=torch.int64, device='cuda')


def run_contig_case(prec, kernel, n, k, tall):
    """axpby_rows / diffnorm_rows over one n x k block of integers in
    [-8, 8] that far.formula builds on the device from the flat index."""
    total = n * k
    assert total > far.B
    dtype, bits = TORCH_DTYPE[prec.name], BITS_DTYPE[prec.name]
    alpha, gamma, second = far.CONTIG_PAIR[prec.name]
    assert second == (far.contig_operands(prec.name, kernel) == 2)
    o_guard = ad.R_GUARD[prec.name]
    cbuf = tall.get(prec, 'C', total, prec.c_fill, prec.c_guard)
    cv = _typed(prec, cbuf, total)
    obuf = ov = None
    if second:
        obuf = tall.get(prec, 'O', total, o_guard, o_guard)
        ov = _typed(prec, obuf, total)
    for lo, hi, i in _slices(total):
        cv[lo:hi] = far.formula(i, 0).to(dtype)
        if second:
            ov[lo:hi] = far.formula(i, 1).to(dtype)
    optr = view_ptr(prec, obuf) if second else 0
    if kernel == 'axpby':
        hip.axpby_rows(view_ptr(prec, cbuf), optr, n, k, alpha, gamma,
                       ch.stream(), dtype=prec.route_dtype)
    else:
        abuf, accv = nd.acc_buffer()
        hip.diffnorm_rows(view_ptr(prec, cbuf), optr, n, k, accv.data_ptr(),
                          ch.stream(), dtype=prec.route_dtype)
    torch.cuda.synchronize()
    for buf, guard in ((cbuf, prec.c_guard), (obuf, o_guard)):
        if buf is not None and not sd.guards_intact(buf, guard):
            raise Mismatch("sentinels around an operand were overwritten")

    # the same integers again, slice by slice: what C and the second operand
    # must hold now, and the int64 sums
    ok = torch.ones((), dtype=torch.bool, device='cuda')
    sums = torch.zeros(2, dtype=torch.int64, device='cuda')
    for lo, hi, i in _slices(total):
        c = far.formula(i, 0)
        o = far.formula(i, 1) if second else None
        if kernel == 'axpby':
            want = alpha * c.to(dtype)
            if second:
                want = want + gamma * o.to(dtype)
        else:
            want = c.to(dtype)
            sums[0] += ((c - o) ** 2 if second else c ** 2).sum()
            sums[1] += (c ** 2).sum()
        ok &= (cv[lo:hi].view(bits) == want.view(bits)).all()
        if second:
            ok &= (ov[lo:hi].view(bits) == o.to(dtype).view(bits)).all()
    if not ok.item():
        raise Mismatch("C differs from the same expression in torch, bit "
                       "for bit" if kernel == 'axpby' else
                       "an input of the pass was written")
    info = dict(sentinels='intact', elements=total)
    if kernel == 'diffnorm':
        if not ch.f64_guards_intact(abuf):
            raise Mismatch("sentinels around the accumulators were "
                           "overwritten")
        want = tuple(float(s) for s in sums.tolist())
        assert all(s < 2 ** 53 for s in sums.tolist())
        got = tuple(accv.cpu().tolist())
        if got != want:
            raise Mismatch(f"accumulators {got} != exact {want}")
        info['acc'] = list(want)
    return info


# ---------------------------------------------------------------------------
# row ids that do not fit int32
# ---------------------------------------------------------------------------

def run_rowid_misuse(prec):
    """Output row ids 2**31, 2**31 + 5 and -1: refused with -1 and a message
    naming `row id` and `int32`; no handle is created (the next valid create
    gets the number that follows the last one's)."""
    lib = hip._load()
    m = sc.matrix('std')
    f64 = prec.struct_dtype == np.float64
    indptr = np.ascontiguousarray(m['indptr'], dtype=np.int64)
    cols = np.ascontiguousarray(m['cols'], dtype=np.int32)
    vals = np.ascontiguousarray(m['vals'], dtype=prec.struct_dtype)
    create = lib.arrow_csr_create_f64 if f64 else lib.arrow_csr_create_opts
    ctype = ctypes.c_double if f64 else ctypes.c_float

    def make(rid):
        return create(m['rows'], m['n0'], cols.size,
                      indptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                      cols.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                      vals.ctypes.data_as(ctypes.POINTER(ctype)),
                      rid.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 0)

    good = np.arange(m['rows'], dtype=np.int64)
    before = make(good)
    if before < 0:
        raise Mismatch("a valid structure was refused")
    for bad in (2 ** 31, 2 ** 31 + 5, -1):
        rid = good.copy()
        rid[7] = bad
        rc = make(rid)
        msg = lib.arrow_last_error().decode()
        if rc != -1:
            raise Mismatch(f"row id {bad} accepted (rc {rc})")
        if not all(w in msg for w in ('row id', 'int32', str(bad), 'row 7')):
            raise Mismatch(f"message does not name the limit and the row: "
                           f"{msg!r}")
    after = make(good)
    if after != before + 1:
        raise Mismatch(f"a refused create took a handle: {before} then "
                       f"{after}")
    for h in (before, after):
        lib.arrow_csr_destroy(h)
    return dict(refused=3)


# ---------------------------------------------------------------------------

def jobs(prec, tall):
    """(name, case group, function): the tall buffers live as long as the
    group does."""
    out = [(c['name'], ('spmm', c['role'], c['k']),
            lambda c=c: run_spmm_case(prec, c, tall))
           for c in far.spmm_cases(prec.name)]
    out += [(name, name, lambda a=(op, k, side): run_route_case(prec, *a, tall))
            for name, op, k, side in far.route_cases(prec.name)]
    out += [(name, name,
             lambda a=(kernel, n, k): run_contig_case(prec, *a, tall))
            for name, kernel, n, k in far.contig_cases(prec.name)]
    out.append(('rowid_misuse', 'rowid_misuse',
                lambda: run_rowid_misuse(prec)))
    assert [j[0] for j in out] == far.job_names(prec.name)
    return out


def main(argv):
    prec = sd.PRECISIONS[argv[1]]
    only = argv[2:]          # job-name prefixes, for a run by hand
    ch.started_with(sc.KERNEL_VARS, {})
    ch.open_gpu("the far driver needs a HIP GPU")

    tall = Tall()
    t_start = time.perf_counter()
    todo = [j for j in jobs(prec, tall)
            if not only or any(j[0].startswith(p) for p in only)]
    group_of = {name: group for name, group, _ in todo}

    def before(name):
        tall.group(group_of[name])  # frees the last group's before the
        torch.cuda.reset_peak_memory_stats()    # peak resets

    def after(line):
        line['peak_bytes'] = int(torch.cuda.max_memory_allocated())

    # an allocation that fails is a failed case, not an errored child
    status = ch.run_jobs([(name, job) for name, _, job in todo],
                         {'prec': prec.name},
                         failed=(AssertionError, torch.cuda.OutOfMemoryError),
                         before=before, after=after)
    if status:
        return status
    tall.free()
    print(json.dumps({'case': 'total', 'prec': prec.name, 'ok': True,
                      's': round(time.perf_counter() - t_start, 1)}),
          flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
