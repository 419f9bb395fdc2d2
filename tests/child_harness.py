"""What every GPU test child needs, once: the job loop and its three outcomes,
the refusal check, the guarded buffers, the upload of a case's matrix and the
start-up checks. The drivers (tests/*_driver.py) hold the cases' own checks;
tests/gpu_children.py starts them and reads their verdict. This is a plain
module, not a test file.

A driver started as a script (`python tests/<name>_driver.py ...`) has tests/
on sys.path and not the repository, so it begins with

    if not __package__:
        import child_harness  # noqa: F401
    from tests import child_harness as ch

The first import only puts the repository on sys.path; everything is used
through tests.child_harness, so there is one Mismatch.
"""
import json
import os
import sys
import time
import traceback

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from arrow_matrix_amd import hip  # noqa: E402
from tests import spmm_cases as sc  # noqa: E402

PAD = 64                 # guard words before and after every raw-word view
F64_GUARD = -7.0         # around every float64 vector
# a job raised something that is not a failed comparison; not 0, not 1 and no
# member of gpu_children.FATAL_STATUS
EXIT_ERRORED = 70
# fields of a case spec that are copied into its line
SPEC_KEYS = ('matrix', 'kind', 'k', 'beta', 'queue', 'op', 'n')


class Mismatch(AssertionError):
    pass


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------
# the start of a child
# ---------------------------------------------------------------------------

def started_with(names, variables):
    """The process started with exactly `variables` among `names`."""
    for var in names:
        assert os.environ.get(var) == variables.get(var), var


def open_gpu(message, set_device=True):
    """set_device: the kernel drivers call the library directly and select
    the device for it; the engines do that themselves."""
    assert torch.cuda.is_available(), message
    if set_device:
        hip.set_device(torch.cuda.current_device())


# ---------------------------------------------------------------------------
# the job loop
# ---------------------------------------------------------------------------

def run_jobs(jobs, tags, failed=(AssertionError,), before=None, after=None):
    """Runs (name, function[, case spec]) jobs in order and prints one JSON
    line each: case, the tags, SPEC_KEYS of the spec, what the function
    returns, ok, error, ms. Stops at the first line that is not ok. Returns
    the exit status:

      0             every job returned
      1             a job raised one of `failed`: a failed case
      EXIT_ERRORED  a job raised anything else (a library error, a HIP error
                    text): the line says errored, the traceback goes to
                    stderr, and the parent starts nothing more on the GPU

    before(name) runs ahead of each job, after(line) once it has ended."""
    for name, job, *spec in jobs:
        line = {'case': name, **tags}
        if spec:
            line.update({key: spec[0][key] for key in SPEC_KEYS
                         if key in spec[0]})
        t0 = time.perf_counter()
        if before:
            before(name)
        try:
            line.update(job())
            line['ok'] = True
        except failed as e:
            line.update(ok=False, error=str(e)[:2000])
        except Exception as e:
            traceback.print_exc()
            line.update(ok=False, errored=True,
                        error=f"{type(e).__name__}: {e}"[:2000])
        if after:
            after(line)
        line['ms'] = round(1e3 * (time.perf_counter() - t0), 1)
        print(json.dumps(line), flush=True)
        if not line['ok']:
            return EXIT_ERRORED if line.get('errored') else 1
    return 0


# ---------------------------------------------------------------------------
# guarded device buffers: raw words of a precision, and float64 vectors
# ---------------------------------------------------------------------------

def _words(prec, bits):
    """The raw bits as a flat array of guard-buffer words."""
    return np.ascontiguousarray(bits).view(prec.word).reshape(-1)


def guarded(prec, bits, guard, device):
    """A copy of the raw `bits` on `device` as a view into a larger buffer
    of prec.word words, with PAD words holding `guard` on either side; the
    view stays 16-byte aligned. Returns (buffer, view)."""
    words = _words(prec, bits)
    buf = torch.full((words.size + 2 * PAD,), guard,
                     dtype=getattr(torch, prec.word), device=device)
    view = buf[PAD:PAD + words.size]
    view.copy_(torch.from_numpy(words))
    assert view.data_ptr() % 16 == 0
    return buf, view


def _intact(buf, pad, guard):
    return bool((buf[:pad] == guard).all().item()
                and (buf[-pad:] == guard).all().item())


def guards_intact(buf, guard):
    return _intact(buf, PAD, guard)


def host_bits(prec, view, shape):
    """The view's words back on the host, as raw bits of `shape`."""
    return view.cpu().numpy().view(prec.bits_dtype).reshape(shape)


def fill_bits(prec):
    """The raw bits of one element whose every word is c_fill."""
    return np.full(prec.words_per_element, prec.c_fill,
                   dtype=prec.word).view(prec.bits_dtype)[0]


def guarded_f64(values, pad, device='cuda'):
    """(buffer, view): a float64 vector between `pad` words of F64_GUARD on
    either side. The buffer remembers its pad."""
    values = np.asarray(values, dtype=np.float64)
    buf = torch.full((values.size + 2 * pad,), F64_GUARD, dtype=torch.float64,
                     device=device)
    buf.pad = pad
    view = buf[pad:pad + values.size]
    view.copy_(torch.from_numpy(values))
    return buf, view


def f64_guards_intact(*bufs):
    return all(_intact(buf, buf.pad, F64_GUARD) for buf in bufs)


# ---------------------------------------------------------------------------
# refused calls
# ---------------------------------------------------------------------------

def refused(call, words, unchanged):
    """call() -> (rc, message) is refused: a negative code, a message that
    holds every one of `words`, and nothing is launched: every entry of
    `unchanged`, {name: (buffer, view, guard, original bits or values)} of
    either guarded form, keeps its guards and its contents."""
    rc, msg = call()
    if any(buf.is_cuda for buf, *_ in unchanged.values()):
        torch.cuda.synchronize()
    if not rc < 0:
        raise Mismatch(f"misuse accepted: {words} (rc {rc})")
    if not all(w in msg for w in words):
        raise Mismatch(f"message does not name {words}: {msg!r}")
    for name, (buf, view, guard, original) in unchanged.items():
        original = np.asarray(original)
        now = view.cpu().numpy().view(original.dtype).reshape(original.shape)
        if not (_intact(buf, getattr(buf, 'pad', PAD), guard)
                and (now == original).all()):
            raise Mismatch(f"{name} was written by a refused call: {words}")


# ---------------------------------------------------------------------------
# a case's matrix on the device
# ---------------------------------------------------------------------------

def upload(prec, case, m=None, row_ids=None):
    """The CsrBlockGPU of a case, with its queue settings. m: the matrix
    (default: the one the case names); row_ids: instead of
    spmm_cases.row_ids(case)."""
    m = sc.matrix(case['matrix']) if m is None else m
    blk = hip.CsrBlockGPU(
        arrays=((m['rows'], m['n0']), m['indptr'], m['cols'],
                prec.a_values(case, m)),
        row_ids=sc.row_ids(case) if row_ids is None else row_ids,
        col_items=case.get('col_items', 0), dtype=prec.struct_dtype)
    prec.check_block(blk)
    if case['queue'] is not None:    # None: the handle follows ARROW_QUEUE
        blk.set_queue(case['queue'])
    if case.get('qblocks'):
        blk.set_qblocks(case['qblocks'])
    return blk


def own_and_other(prec):
    """(matrix, handle, handle): `std` uploaded at the precision's own
    structure dtype and at the other one."""
    m = sc.matrix('std')
    arrays = ((m['rows'], m['n0']), m['indptr'], m['cols'], m['vals'])
    other = np.float32 if prec.struct_dtype == np.float64 else np.float64
    return m, hip.CsrBlockGPU(arrays=arrays, dtype=prec.struct_dtype), \
        hip.CsrBlockGPU(arrays=arrays, dtype=other)
