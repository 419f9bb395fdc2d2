"""Compute backends for the arrow engine.

- GpuBackend: the product path — torch CUDA tensors for storage/comm,
  hand-written HIP kernels via the C ABI (hip.py / libarrowspmm.so) for all
  compute. FAILS LOUDLY if the extension is missing; never falls back.
- CpuBackend: the reference's own `--device cpu` semantics — scipy CSR `@`
  (arrow_slim_mpi.py:78-156). This is a deliberate feature (it IS the parity
  reference named by BASELINE.json), not a fallback for the GPU path.

Both expose the same small surface so ArrowSlimMPI/ArrowDecompositionMPI
have a single code path.
"""
from typing import Optional

import numpy as np
import torch

from . import hip


_TORCH_DTYPE = {np.dtype(np.float32): torch.float32,
                np.dtype(np.float64): torch.float64}


class CpuBackend:
    device = 'cpu'

    def __init__(self, dtype=np.float32):
        if hip.is_bf16(dtype):
            raise NotImplementedError(
                "bfloat16 features run on device='gpu' only: the cpu device "
                "is the scipy parity reference, which has no bfloat16")
        self.np_dtype = np.dtype(dtype)
        self.torch_dtype = _TORCH_DTYPE[self.np_dtype]
        # the feature side of the surface, as on GpuBackend
        self.bf16 = False
        self.feat_dtype = self.np_dtype
        self.feat_itemsize = self.np_dtype.itemsize
        self.norm_launches = 0      # no scipy launch measures its own step
        self.diffnorm_launches = 0

    def zeros(self, shape):
        return torch.zeros(shape, dtype=self.torch_dtype)

    def asarray(self, x) -> torch.Tensor:
        if isinstance(x, torch.Tensor):
            return x.to(self.torch_dtype).cpu()
        return torch.from_numpy(np.ascontiguousarray(x, dtype=self.np_dtype))

    def index_tensor(self, idx: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64))

    def upload_block(self, csr):
        from scipy import sparse
        return sparse.csr_matrix(csr)

    def spmm_block(self, block, X: torch.Tensor, C: torch.Tensor, beta: int,
                   alpha: float = 1.0, gamma: float = 0.0, R=None):
        """C (+)= block @ X (scipy kernel, the reference CPU path); with
        alpha / gamma / R the affine step C = alpha*(block@X) + gamma*R
        (+ C), the parity reference of the fused GPU launch."""
        res = block @ X.numpy()
        if alpha != 1.0 or gamma != 0.0 or R is not None:
            dt = self.np_dtype.type
            res = dt(alpha) * res
            if R is not None:
                res = res + dt(gamma) * R.numpy()
        if beta == 0:
            C.numpy()[:] = res
        else:
            C.numpy()[:] += res

    def gather_rows(self, src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        return src[idx]

    def scatter_rows(self, dst: torch.Tensor, idx: torch.Tensor, src: torch.Tensor):
        dst[idx] = src

    def scatter_add_rows(self, dst: torch.Tensor, idx: torch.Tensor, src: torch.Tensor):
        dst[idx] += src

    def permute_rows(self, dst, dst_idx, src, src_idx):
        dst[dst_idx] = src[src_idx]

    def permute_add_rows(self, dst, dst_idx, src, src_idx):
        dst[dst_idx] += src[src_idx]

    def axpby_rows(self, C: torch.Tensor, R, alpha: float, gamma: float):
        """C = alpha * C + gamma * R in place (numpy)."""
        dt = self.np_dtype.type
        c = C.numpy()
        c *= dt(alpha)
        if R is not None:
            c += dt(gamma) * R.numpy()

    def diffnorm_rows(self, C: torch.Tensor, D, acc: torch.Tensor):
        """acc[0] += sum (C - D)^2, acc[1] += sum C^2, the definition of the
        step norms in float64 (D None means 0); the parity reference of the
        GPU kernels."""
        self.diffnorm_launches += 1
        c = C.numpy().astype(np.float64)
        d = D.numpy().astype(np.float64) if D is not None else 0.0
        acc[0] += float(np.square(c - d).sum())
        acc[1] += float(np.square(c).sum())

    def norm_acc(self) -> torch.Tensor:
        """The two-double accumulator of the step norms."""
        return torch.zeros(2, dtype=torch.float64)

    # -- operator scaling (the parity reference of arrow_csr_sums / _scale) --

    def scale_vector(self, x) -> torch.Tensor:
        """A float64 vector of the operator passes, on this backend."""
        return torch.from_numpy(np.array(x, dtype=np.float64))

    @staticmethod
    def _block_coo(block):
        """(csr, output row per nonzero) of a scipy block or of a folded
        (csr, row_ids) pair."""
        csr, rid = block if isinstance(block, tuple) else (block, None)
        rows = np.repeat(np.arange(csr.shape[0], dtype=np.int64),
                         np.diff(csr.indptr))
        return csr, (rows if rid is None else np.asarray(rid)[rows])

    def block_sums(self, block, row_sum, col_sum0, col_sum1, absolute=False):
        """ADD the sums of block's stored values into the float64 vectors,
        indexed as arrow_csr_sums indexes them: row_sum by output row (after
        the row_ids of a folded pair), col_sum0 by column c >= 0, col_sum1
        at -c-1 for c < 0. None skips an output."""
        if row_sum is None and col_sum0 is None and col_sum1 is None:
            raise ValueError("block_sums: all three outputs are None")
        csr, rows = self._block_coo(block)
        v = csr.data.astype(np.float64)
        if absolute:
            v = np.abs(v)
        cols = csr.indices.astype(np.int64)
        pos = cols >= 0
        if row_sum is not None:
            np.add.at(row_sum.numpy(), rows, v)
        if col_sum0 is not None:
            np.add.at(col_sum0.numpy(), cols[pos], v[pos])
        if col_sum1 is not None:
            np.add.at(col_sum1.numpy(), -cols[~pos] - 1, v[~pos])

    def block_scale(self, block, r, c0, c1):
        """val = T((float64(val) * r) * c) in place, the rounding formula of
        arrow_csr_scale; None is the factor 1."""
        if r is None and c0 is None and c1 is None:
            return
        csr, rows = self._block_coo(block)
        cols = csr.indices.astype(np.int64)
        pos = cols >= 0
        rf = r.numpy()[rows] if r is not None else 1.0
        cf = np.ones(cols.size, dtype=np.float64)
        if c0 is not None:
            cf[pos] = c0.numpy()[cols[pos]]
        if c1 is not None:
            cf[~pos] = c1.numpy()[-cols[~pos] - 1]
        csr.data[:] = ((csr.data.astype(np.float64) * rf) * cf).astype(
            csr.data.dtype)

    def synchronize(self):
        pass


class GpuBackend:
    device = 'cuda'

    def __init__(self, device_index: Optional[int] = None, dtype=np.float32):
        # bfloat16 FEATURES (X, C and everything routed): the matrix values
        # and np_dtype stay float32, torch_dtype / feat_dtype say bfloat16,
        # and feat_itemsize is what the HBM-capacity guards count
        self.bf16 = hip.is_bf16(dtype)
        self.np_dtype = np.dtype(np.float32 if self.bf16 else dtype)
        if self.np_dtype not in _TORCH_DTYPE:
            raise NotImplementedError(
                f"the HIP kernels compute in float32 or float64, not "
                f"{self.np_dtype}")
        self.torch_dtype = (torch.bfloat16 if self.bf16
                            else _TORCH_DTYPE[self.np_dtype])
        # what hip.py dispatches the feature kernels on
        self.feat_dtype = torch.bfloat16 if self.bf16 else self.np_dtype
        self.feat_itemsize = 2 if self.bf16 else self.np_dtype.itemsize
        if not torch.cuda.is_available():
            raise hip.ArrowSpmmError(
                "GPU backend requested but no HIP device is available")
        if device_index is None:
            device_index = torch.cuda.current_device()
        self.device_index = device_index
        self.torch_device = torch.device('cuda', device_index)
        # Loading the library here makes a missing .so fail at construction.
        hip.set_device(device_index)
        # how often the measuring entry points were called: fused launches
        # and stand-alone passes (the engine tests read them)
        self.norm_launches = 0
        self.diffnorm_launches = 0

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device_index).cuda_stream

    def zeros(self, shape):
        return torch.zeros(shape, dtype=self.torch_dtype, device=self.torch_device)

    def asarray(self, x) -> torch.Tensor:
        if isinstance(x, torch.Tensor):
            return x.to(self.torch_device, dtype=self.torch_dtype)
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=self.np_dtype)).to(self.torch_device)
        # bf16 features: one round-to-nearest-even cast of the float32 values
        return t.to(self.torch_dtype) if self.bf16 else t

    def index_tensor(self, idx: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(self.torch_device)

    def upload_block(self, csr):
        return hip.CsrBlockGPU(csr, dtype=self.np_dtype)

    @staticmethod
    def _ptr_like(C, T) -> int:
        """data_ptr() of a tensor laid out like C (R or D); 0 for None."""
        if T is None:
            return 0
        assert T.is_contiguous() and T.shape == C.shape and T.dtype == C.dtype
        return T.data_ptr()

    def _launch(self, spmm, xs, C, beta, alpha, gamma, R, norm):
        """block.spmm (one X in xs) or block.spmm_dual (two) on tensors.
        hip.py picks the entry point: the plain one when alpha, gamma, R and
        norm are all at their defaults."""
        assert all(X.is_contiguous() for X in xs) and C.is_contiguous()
        if norm is not None:
            D, acc = norm
            assert acc.dtype == torch.float64 and acc.numel() == 2 \
                and acc.device == C.device
            self.norm_launches += 1
            norm = (self._ptr_like(C, D), acc.data_ptr())
        spmm(*(X.data_ptr() for X in xs), C.data_ptr(), C.shape[1], beta,
             self._stream(), feat_dtype=self.feat_dtype, alpha=alpha,
             gamma=gamma, R_ptr=self._ptr_like(C, R), norm=norm)

    def spmm_block(self, block: hip.CsrBlockGPU, X: torch.Tensor, C: torch.Tensor, beta: int,
                   alpha: float = 1.0, gamma: float = 0.0, R=None, norm=None):
        """norm=(D, acc): the launch also adds sum (C - D)^2 and sum C^2 into
        the two float64 of the device tensor acc (beta 0 only)."""
        self._launch(block.spmm, (X,), C, beta, alpha, gamma, R, norm)

    def upload_arrays(self, shape, indptr, indices, data, row_ids=None,
                      col_items=False) -> hip.CsrBlockGPU:
        return hip.CsrBlockGPU(arrays=(shape, indptr, indices, data),
                               row_ids=row_ids, col_items=col_items,
                               dtype=self.np_dtype)

    def spmm_dual(self, block: hip.CsrBlockGPU, X0: torch.Tensor,
                  X1: torch.Tensor, C: torch.Tensor, beta: int,
                  alpha: float = 1.0, gamma: float = 0.0, R=None, norm=None):
        self._launch(block.spmm_dual, (X0, X1), C, beta, alpha, gamma, R,
                     norm)

    def diffnorm_rows(self, C: torch.Tensor, D, acc: torch.Tensor):
        """acc[0] += sum (C - D)^2, acc[1] += sum C^2 over the rows of C
        (arrow_diffnorm_rows_*; D None means 0)."""
        assert C.is_contiguous() and acc.dtype == torch.float64 \
            and acc.numel() == 2 and acc.device == C.device
        D_ptr = self._ptr_like(C, D)
        self.diffnorm_launches += 1
        if C.shape[0]:
            hip.diffnorm_rows(C.data_ptr(), D_ptr, C.shape[0], C.shape[1],
                              acc.data_ptr(), self._stream(),
                              dtype=self.feat_dtype)

    def norm_acc(self) -> torch.Tensor:
        """The two-double device accumulator of the step norms."""
        return torch.zeros(2, dtype=torch.float64, device=self.torch_device)

    # -- operator scaling (arrow_csr_sums / arrow_csr_scale) ----------------

    def scale_vector(self, x) -> torch.Tensor:
        """A float64 device vector of the operator passes."""
        return torch.from_numpy(np.array(x, dtype=np.float64)).to(
            self.torch_device)

    def _vec_ptr(self, v) -> int:
        if v is None:
            return 0
        assert v.dtype == torch.float64 and v.is_contiguous() \
            and v.device == self.torch_device
        return v.data_ptr()

    def block_sums(self, block: hip.CsrBlockGPU, row_sum, col_sum0, col_sum1,
                   absolute=False):
        """ADD the sums of the resident values of block into float64 device
        vectors (views are fine: a row vector starts at the block's first
        output row). None skips an output."""
        block.sums(self._vec_ptr(row_sum), self._vec_ptr(col_sum0),
                   self._vec_ptr(col_sum1), absolute, self._stream())

    def block_scale(self, block: hip.CsrBlockGPU, r, c0, c1):
        """Rescale the resident values of block in place by float64 device
        vectors; None is the factor 1."""
        block.scale(self._vec_ptr(r), self._vec_ptr(c0), self._vec_ptr(c1),
                    self._stream())

    def axpby_rows(self, C: torch.Tensor, R, alpha: float, gamma: float):
        """C = alpha * C + gamma * R in place (arrow_axpby_rows_*)."""
        assert C.is_contiguous()
        R_ptr = self._ptr_like(C, R)
        if C.shape[0]:
            hip.axpby_rows(C.data_ptr(), R_ptr, C.shape[0], C.shape[1], alpha,
                           gamma, self._stream(), dtype=self.feat_dtype)

    def gather_rows(self, src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        out = torch.empty((idx.shape[0], src.shape[1]), dtype=self.torch_dtype,
                          device=self.torch_device)
        if idx.shape[0]:
            hip.gather_rows(src.data_ptr(), out.data_ptr(), idx.data_ptr(),
                            idx.shape[0], src.shape[1], self._stream(),
                            dtype=self.feat_dtype)
        return out

    def scatter_rows(self, dst: torch.Tensor, idx: torch.Tensor, src: torch.Tensor):
        if idx.shape[0]:
            hip.scatter_rows(dst.data_ptr(), src.data_ptr(), idx.data_ptr(),
                             idx.shape[0], dst.shape[1], self._stream(),
                             dtype=self.feat_dtype)

    def scatter_add_rows(self, dst: torch.Tensor, idx: torch.Tensor, src: torch.Tensor):
        if idx.shape[0]:
            hip.scatter_add_rows(dst.data_ptr(), src.data_ptr(), idx.data_ptr(),
                                 idx.shape[0], dst.shape[1], self._stream(),
                                 dtype=self.feat_dtype)

    def permute_rows(self, dst, dst_idx, src, src_idx):
        if dst_idx.shape[0]:
            hip.permute_rows(dst.data_ptr(), src.data_ptr(), dst_idx.data_ptr(),
                             src_idx.data_ptr(), dst_idx.shape[0], dst.shape[1],
                             self._stream(),
                             dtype=self.feat_dtype)

    def permute_add_rows(self, dst, dst_idx, src, src_idx):
        if dst_idx.shape[0]:
            hip.permute_add_rows(dst.data_ptr(), src.data_ptr(),
                                 dst_idx.data_ptr(), src_idx.data_ptr(),
                                 dst_idx.shape[0], dst.shape[1], self._stream(),
                                 dtype=self.feat_dtype)

    def synchronize(self):
        torch.cuda.synchronize(self.device_index)


def make_backend(device: str, dtype=np.float32):
    if device in ('gpu', 'cuda'):
        if hip.is_bf16(dtype):
            return GpuBackend(dtype=dtype)
        if np.dtype(dtype) not in _TORCH_DTYPE:
            raise NotImplementedError(
                "the HIP kernels compute in float32 (the reference benchmark "
                "default, arrow_bench.py:21) or float64, not "
                f"{np.dtype(dtype)}")
        return GpuBackend(dtype=dtype)
    if device == 'cpu':
        return CpuBackend(dtype)
    raise ValueError(f"unknown device {device!r} (use 'cpu' or 'gpu')")
