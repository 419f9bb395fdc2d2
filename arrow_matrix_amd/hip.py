"""ctypes binding to libarrowspmm.so (the C-ABI HIP compute library).

This is the product GPU path. It FAILS LOUDLY if the extension is missing or
a call errors — there is no CPU fallback here (the explicit `--device cpu`
mode of the package is a separate, deliberate scipy path mirroring the
reference's own cpu mode, arrow_slim_mpi.py:78-156).
"""
import ctypes
import os
from typing import Optional

import numpy as np

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libarrowspmm.so')
_lib: Optional[ctypes.CDLL] = None


class ArrowSpmmError(RuntimeError):
    pass


def _load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise ArrowSpmmError(
            f"libarrowspmm.so not found at {_LIB_PATH}. Build it with "
            f"`make -C arrow_matrix_amd/csrc` (or __graft_entry__.build()). "
            f"The GPU path does not fall back to CPU.")
    lib = ctypes.CDLL(_LIB_PATH)
    lib.arrow_abi_version.restype = ctypes.c_int
    lib.arrow_last_error.restype = ctypes.c_char_p
    lib.arrow_device_count.restype = ctypes.c_int
    lib.arrow_set_device.argtypes = [ctypes.c_int]
    lib.arrow_set_device.restype = ctypes.c_int
    lib.arrow_synchronize.restype = ctypes.c_int
    lib.arrow_csr_create.restype = ctypes.c_int64
    lib.arrow_csr_create.argtypes = [
        ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
        ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32),
        ctypes.POINTER(ctypes.c_float)]
    lib.arrow_csr_create_rows.restype = ctypes.c_int64
    lib.arrow_csr_create_rows.argtypes = [
        ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
        ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32),
        ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)]
    lib.arrow_csr_create_opts.restype = ctypes.c_int64
    lib.arrow_csr_create_opts.argtypes = [
        ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
        ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32),
        ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64),
        ctypes.c_int]
    lib.arrow_csr_destroy.argtypes = [ctypes.c_int64]
    lib.arrow_csr_destroy.restype = ctypes.c_int
    lib.arrow_csr_nnz.argtypes = [ctypes.c_int64]
    lib.arrow_csr_nnz.restype = ctypes.c_int64
    lib.arrow_csr_set_xcd_remap.argtypes = [ctypes.c_int64, ctypes.c_int]
    lib.arrow_csr_set_xcd_remap.restype = ctypes.c_int
    lib.arrow_csr_set_queue.argtypes = [ctypes.c_int64, ctypes.c_int]
    lib.arrow_csr_set_queue.restype = ctypes.c_int
    lib.arrow_csr_set_qblocks.argtypes = [ctypes.c_int64, ctypes.c_int]
    lib.arrow_csr_set_qblocks.restype = ctypes.c_int
    # Everything below is written once for all precisions:
    #   ABI 1003  float64: arrow_csr_create_f64 / arrow_csr_dtype, the _f64
    #             SpMM, plan and routing entry points
    #   ABI 1004  bfloat16 features: the _bf16 entry points; no create call,
    #             they take a float32 structure handle
    #   ABI 1005  affine step: arrow_spmm[_dual]_affine*, arrow_axpby_rows_*
    #   ABI 1006  step norms: arrow_spmm[_dual]_affine_norm*,
    #             arrow_diffnorm_rows_*
    #   ABI 1007  operator scaling: arrow_csr_sums, arrow_csr_scale (float32
    #             and float64 handles; float64 device vectors in both)
    i64, cint, ptr, dbl = (ctypes.c_int64, ctypes.c_int, ctypes.c_void_p,
                          ctypes.c_double)

    def declare(name, argtypes, restype=ctypes.c_int):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, restype
    declare('arrow_csr_create_f64', [
        i64, i64, i64, ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_int32),
        ctypes.POINTER(dbl), ctypes.POINTER(i64), cint], restype=i64)
    declare('arrow_csr_dtype', [i64])
    # (handle, row, col0, col1, absolute, stream) / (handle, r, c0, c1, stream)
    declare('arrow_csr_sums', [i64, ptr, ptr, ptr, cint, ptr])
    declare('arrow_csr_scale', [i64, ptr, ptr, ptr, ptr])
    for sfx in _SPMM_SUFFIX.values():
        for dual in (False, True):
            for tier in _SPMM_TIERS:
                # the list the call itself passes, with types for values
                declare(_spmm_symbol(dual, tier, sfx), _spmm_args(
                    tier, i64, [ptr] * (2 if dual else 1), ptr, ptr, ptr, ptr,
                    i64, dbl, dbl, cint, ptr))
        declare('arrow_spmm_plan' + sfx,
                [i64, i64, cint, ctypes.POINTER(ctypes.c_int32), cint])
    for sfx in _SPMM_SUFFIX:
        for argtypes, names in (
                # (a, b, idx, n, k, stream)
                ([ptr, ptr, ptr, i64, i64, ptr],
                 ('gather_rows', 'scatter_rows', 'scatter_add_rows')),
                # (dst, src, dst_idx, src_idx, n, k, stream)
                ([ptr, ptr, ptr, ptr, i64, i64, ptr],
                 ('permute_rows', 'permute_add_rows')),
                # the stand-alone tail (C, R, n, k, alpha, gamma, stream)
                ([ptr, ptr, i64, i64, dbl, dbl, ptr], ('axpby_rows',)),
                # the stand-alone norms (C, D, n, k, acc, stream)
                ([ptr, ptr, i64, i64, ptr, ptr], ('diffnorm_rows',))):
            for name in names:
                declare(f'arrow_{name}_{sfx}', argtypes)
    _lib = lib
    return lib


def is_built() -> bool:
    return os.path.exists(_LIB_PATH)


def _check(rc, what: str):
    if rc < 0:
        raise ArrowSpmmError(f"{what} failed: {_load().arrow_last_error().decode()}")
    return rc


def is_bf16(dtype) -> bool:
    """True for the two spellings of the bfloat16 feature dtype,
    torch.bfloat16 and 'bfloat16' (numpy has no bfloat16)."""
    if isinstance(dtype, str):
        return dtype == 'bfloat16'
    return (type(dtype).__module__ == 'torch'
            and type(dtype).__name__ == 'dtype'
            and str(dtype) == 'torch.bfloat16')


def _suffix(dtype) -> str:
    """'f32' or 'f64' for a supported numpy dtype, 'bf16' for torch.bfloat16
    or 'bfloat16' (features only: A stays float32); TypeError for any
    other."""
    if is_bf16(dtype):
        return 'bf16'
    try:
        dt = np.dtype(dtype)
    except (TypeError, ValueError):
        dt = None
    if dt == np.float32:
        return 'f32'
    if dt == np.float64:
        return 'f64'
    raise TypeError(f"the HIP kernels compute in float32 or float64, "
                    f"not {dtype!r}")


# the SpMM family (arrow_spmm*, arrow_spmm_plan*) spells float32 with no
# suffix; every other entry point takes '_' + _suffix(dtype)
_SPMM_SUFFIX = {'f32': '', 'f64': '_f64', 'bf16': '_bf16'}
_SPMM_TIERS = ('', '_affine', '_affine_norm')


def _spmm_symbol(dual: bool, tier: str, sfx: str) -> str:
    return 'arrow_spmm' + ('_dual' if dual else '') + tier + sfx


def _spmm_args(tier, handle, xs, C, R, D, acc, k, alpha, gamma, beta, stream):
    """The positional list of arrow_spmm[_dual]<tier>* (include/arrow_spmm.h):
    handle, X.., C, [R], [D, acc], k, [alpha, gamma], beta, stream. Called
    with values to launch and with ctypes types to declare, so a declaration
    cannot drift from its call."""
    args = [handle, *xs, C]
    if tier:
        args.append(R)
    if tier == '_affine_norm':
        args += [D, acc]
    args.append(k)
    if tier:
        args += [alpha, gamma]
    return args + [beta, stream]


class CsrBlockGPU:
    """A CSR block resident in HBM (uploaded ONCE — unlike the reference,
    which re-uploads A every iteration, arrow_slim_mpi.py:184-232)."""

    def __init__(self, csr=None, arrays=None, row_ids=None, col_items=False,
                 dtype=np.float32):
        """csr: scipy CSR, or arrays=(shape, indptr, indices, data) for raw
        uploads (the fused layouts use negative column indices, which scipy
        would reject). row_ids: optional explicit output-row id per
        structure row (reordered layouts). col_items: work-item ordering
        mode (hub structures; see arrow_csr_create_opts flags): 0/False
        row order, 1/True global column sort, 2 column sort WITHIN each
        XCD queue segment (two-level). dtype: float32 or float64 — the
        precision of the resident values, fixed here; spmm / spmm_dual
        then take device pointers of that precision. A float32 structure
        also serves bfloat16 FEATURES (raw bf16 X and C, fp32 accumulation):
        pass feat_dtype=torch.bfloat16 / 'bfloat16' to spmm / spmm_dual."""
        if is_bf16(dtype):
            raise TypeError("A stays float32 under bfloat16 features: create "
                            "the structure with dtype=float32 and pass "
                            "feat_dtype to spmm / spmm_dual")
        f64 = _suffix(dtype) == 'f64'
        self.dtype = np.dtype(dtype)
        lib = _load()
        if arrays is not None:
            (rows, cols), indptr, indices, data = arrays
        else:
            csr = csr.tocsr()
            rows, cols = csr.shape
            indptr, indices, data = csr.indptr, csr.indices, csr.data
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        data = np.ascontiguousarray(data, dtype=self.dtype)
        self.shape = (rows, cols)
        self.nnz = int(indices.size)
        rid = (np.ascontiguousarray(row_ids, dtype=np.int64)
               if row_ids is not None else None)
        # every create entry point reaches the same C routine; null row_ids
        # and flags 0 are its defaults
        create, ctype, what = (
            (lib.arrow_csr_create_f64, ctypes.c_double, "arrow_csr_create_f64")
            if f64 else
            (lib.arrow_csr_create_opts, ctypes.c_float, "arrow_csr_create_opts"))
        self._handle = _check(create(
            rows, cols, self.nnz,
            indptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            indices.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            data.ctypes.data_as(ctypes.POINTER(ctype)),
            (rid.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
             if rid is not None else None), int(col_items)), what)

    def _entry(self, name: str, feat_dtype):
        """The SpMM entry point for features of feat_dtype (None: the
        structure's own precision)."""
        sfx = _SPMM_SUFFIX[
            _suffix(self.dtype if feat_dtype is None else feat_dtype)]
        return getattr(_load(), name + sfx), name + sfx

    def _spmm(self, xs, C_ptr, k, beta, stream, feat_dtype, alpha, gamma,
              R_ptr, norm):
        """spmm (one X pointer in xs) and spmm_dual (two): the norm tier when
        norm is given, else the affine tier when alpha, gamma or R_ptr is,
        else the plain entry point."""
        tier = ('_affine_norm' if norm is not None else
                '_affine' if alpha != 1.0 or gamma != 0.0 or R_ptr else '')
        fn, name = self._entry(_spmm_symbol(len(xs) == 2, tier, ''),
                               feat_dtype)
        D_ptr, acc_ptr = norm if norm is not None else (0, 0)
        _check(fn(*_spmm_args(tier, self._handle, xs, C_ptr, R_ptr or None,
                              D_ptr or None, acc_ptr or None, k, float(alpha),
                              float(gamma), beta, stream)), name)

    def spmm(self, X_ptr: int, C_ptr: int, k: int, beta: int, stream: int = 0,
             feat_dtype=None, alpha: float = 1.0, gamma: float = 0.0,
             R_ptr: int = 0, norm=None):
        """C (+)= A @ X on device pointers (e.g. torch tensor data_ptr()).
        With alpha, gamma or R_ptr given: the fused affine step
        C = alpha * (A @ X) + gamma * R + beta * C (arrow_spmm_affine*;
        R_ptr 0 needs gamma 0). Without them the plain entry point is
        called, as before. norm=(D_ptr, acc_ptr): the step also adds
        sum (C - D)^2 and sum C^2 into the two device doubles at acc_ptr
        (arrow_spmm_affine_norm*; beta 0 only, D_ptr 0 means D = 0)."""
        self._spmm((X_ptr,), C_ptr, k, beta, stream, feat_dtype, alpha, gamma,
                   R_ptr, norm)

    def set_xcd_remap(self, enable: bool):
        _check(_load().arrow_csr_set_xcd_remap(self._handle, 1 if enable else 0),
               "arrow_csr_set_xcd_remap")

    def set_queue(self, mode: int):
        """Per-XCD queue scheduler: 1 on, 0 off, -1 follow ARROW_QUEUE env."""
        _check(_load().arrow_csr_set_queue(self._handle, int(mode)),
               "arrow_csr_set_queue")

    def set_qblocks(self, blocks: int):
        """Per-structure queue-grid override (0 = ARROW_Q_BLOCKS default)."""
        _check(_load().arrow_csr_set_qblocks(self._handle, int(blocks)),
               "arrow_csr_set_qblocks")

    def spmm_dual(self, X0_ptr: int, X1_ptr: int, C_ptr: int, k: int,
                  beta: int, stream: int = 0, feat_dtype=None,
                  alpha: float = 1.0, gamma: float = 0.0, R_ptr: int = 0,
                  norm=None):
        """Fused dual-operand SpMM: negative column indices (encoded at
        upload as -(idx+1)) read X1 (see include/arrow_spmm.h). alpha, gamma,
        R_ptr and norm as in spmm (arrow_spmm_dual_affine*,
        arrow_spmm_dual_affine_norm*)."""
        self._spmm((X0_ptr, X1_ptr), C_ptr, k, beta, stream, feat_dtype, alpha,
                   gamma, R_ptr, norm)

    def sums(self, row_sum_ptr: int = 0, col_sum0_ptr: int = 0,
             col_sum1_ptr: int = 0, absolute: bool = False, stream: int = 0):
        """ADD the sums of the resident values into float64 device vectors
        (arrow_csr_sums): row_sum by output row, as C; col_sum0 by column
        c >= 0, as X0; col_sum1 at -c-1 for c < 0, as X1. absolute sums |v|.
        A pointer of 0 skips that output; all three 0 is an error."""
        _check(_load().arrow_csr_sums(
            self._handle, row_sum_ptr or None, col_sum0_ptr or None,
            col_sum1_ptr or None, 1 if absolute else 0, stream),
            "arrow_csr_sums")

    def scale(self, row_scale_ptr: int = 0, col_scale0_ptr: int = 0,
              col_scale1_ptr: int = 0, stream: int = 0):
        """Rescale the resident values in place (arrow_csr_scale):
        val = T((float64(val) * r) * c), r and c from float64 device vectors
        indexed as in sums; a pointer of 0 is the factor 1. Must not overlap
        in time with an SpMM on this structure."""
        _check(_load().arrow_csr_scale(
            self._handle, row_scale_ptr or None, col_scale0_ptr or None,
            col_scale1_ptr or None, stream), "arrow_csr_scale")

    def __del__(self):
        if getattr(self, '_handle', None) is not None and _lib is not None:
            try:
                _lib.arrow_csr_destroy(self._handle)
            except Exception:
                pass


def set_device(device: int):
    _check(_load().arrow_set_device(device), "arrow_set_device")


def synchronize():
    _check(_load().arrow_synchronize(), "arrow_synchronize")


def _route(name: str, dtype):
    name = f'arrow_{name}_{_suffix(dtype)}'
    return getattr(_load(), name), name


def gather_rows(src_ptr: int, dst_ptr: int, idx_ptr: int, n: int, k: int,
                stream: int = 0, dtype=np.float32):
    fn, name = _route('gather_rows', dtype)
    _check(fn(src_ptr, dst_ptr, idx_ptr, n, k, stream), name)


def scatter_rows(dst_ptr: int, src_ptr: int, idx_ptr: int, n: int, k: int,
                 stream: int = 0, dtype=np.float32):
    fn, name = _route('scatter_rows', dtype)
    _check(fn(dst_ptr, src_ptr, idx_ptr, n, k, stream), name)


def scatter_add_rows(dst_ptr: int, src_ptr: int, idx_ptr: int, n: int, k: int,
                     stream: int = 0, dtype=np.float32):
    fn, name = _route('scatter_add_rows', dtype)
    _check(fn(dst_ptr, src_ptr, idx_ptr, n, k, stream), name)


def permute_rows(dst_ptr, src_ptr, dst_idx_ptr, src_idx_ptr, n, k, stream=0,
                 dtype=np.float32):
    fn, name = _route('permute_rows', dtype)
    _check(fn(dst_ptr, src_ptr, dst_idx_ptr, src_idx_ptr, n, k, stream), name)


def permute_add_rows(dst_ptr, src_ptr, dst_idx_ptr, src_idx_ptr, n, k,
                     stream=0, dtype=np.float32):
    fn, name = _route('permute_add_rows', dtype)
    _check(fn(dst_ptr, src_ptr, dst_idx_ptr, src_idx_ptr, n, k, stream), name)


def axpby_rows(C_ptr: int, R_ptr: int, n: int, k: int, alpha: float,
               gamma: float, stream: int = 0, dtype=np.float32):
    """C = alpha * C + gamma * R over n contiguous rows of width k (the
    stand-alone tail of the affine step; R_ptr 0 needs gamma 0)."""
    fn, name = _route('axpby_rows', dtype)
    _check(fn(C_ptr, R_ptr or None, n, k, float(alpha), float(gamma), stream),
           name)


def diffnorm_rows(C_ptr: int, D_ptr: int, n: int, k: int, acc_ptr: int,
                  stream: int = 0, dtype=np.float32):
    """acc[0] += sum (C - D)^2, acc[1] += sum C^2 over n contiguous rows of
    width k (the stand-alone step norms; D_ptr 0 means D = 0; acc_ptr is two
    device doubles the caller zeroed)."""
    fn, name = _route('diffnorm_rows', dtype)
    _check(fn(C_ptr, D_ptr or None, n, k, acc_ptr or None, stream), name)


PLAN_FIELDS = ('vec', 'group', 'scheduler', 'nt_mode', 'chunk_items',
               'grid_cap', 'launches')
SCHED_GRID_STRIDE, SCHED_QUEUE_BLOCK, SCHED_QUEUE_WAVE = 0, 1, 2


def spmm_plan(k: int, nnz: int, queue_mode: int = -1,
              dtype=np.float32) -> dict:
    """The launch plan arrow_spmm (or, for dtype float64, arrow_spmm_f64;
    for the bfloat16 feature dtype, arrow_spmm_bf16) takes for a structure
    of `nnz` nonzeros at width k (arrow_spmm_plan / _f64 / _bf16; needs no
    device). The ARROW_* kernel-tuning variables are read once per process,
    on first use."""
    name = 'arrow_spmm_plan' + _SPMM_SUFFIX[_suffix(dtype)]
    out = (ctypes.c_int32 * len(PLAN_FIELDS))()
    n = _check(getattr(_load(), name)(int(k), int(nnz), int(queue_mode), out,
                                      len(PLAN_FIELDS)), name)
    if n != len(PLAN_FIELDS):
        raise ArrowSpmmError(f"arrow_spmm_plan: library has {n} plan fields, "
                             f"binding expects {len(PLAN_FIELDS)}")
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def abi_version() -> int:
    return _load().arrow_abi_version()
