"""PETSc-style 1D row-slice SpMM behind the kept MatrixSlice API
(SURVEY.md §8f-2).

Re-implements the semantics of the reference's
`arrow/baseline/spmm_petsc.py`:

    Y_i += A_i_local @ X_i_local + A_i_nonlocal @ X_i_nonlocal

with the non-local X rows exchanged by a sparse neighbourhood pattern
(one message per peer, spmm_exchange_x_bulk, spmm_petsc.py:105-144) that is
OVERLAPPED with the local multiply (spmm_petsc.py:193-211). Here the slices
are resident on the GPU (the reference re-uploads per call,
spmm_petsc.py:224-307), the exchange is grouped p2p over xGMI, and the
multiplies are the hand-written CSR kernel. The reference's GPU column
tiling (compute_gpu_tiling_size, :323-395) is unnecessary with 288 GB of
HBM3E per GPU and is intentionally not reproduced.
"""
import time
from typing import Optional

import numpy as np
import torch

from .backends import make_backend
from .comm import Comm
from .common import wb_logging
from .matrix_slice import MatrixSlice


class SpmmPETSc:
    """Resident 1D-slice SpMM engine over a MatrixSlice."""

    def __init__(self, comm: Optional[Comm], matrix_slice: MatrixSlice,
                 device: str = 'cpu', dtype=np.float32):
        self.comm = comm if comm is not None else Comm()
        self.ms = matrix_slice
        from .hip import is_bf16
        if is_bf16(dtype):
            raise NotImplementedError(
                "SpmmPETSc is the float32/float64 baseline: bfloat16 "
                "features are an arrow-engine option (its exchange would "
                "move and sum bfloat16 rows)")
        self.backend = make_backend(device, dtype)
        self.A_local = self.backend.upload_block(matrix_slice.A_i_local)
        self.A_nonlocal = (self.backend.upload_block(matrix_slice.A_i_nonlocal)
                           if matrix_slice.A_i_nonlocal.shape[1] > 0 else None)
        self.n_local = matrix_slice.A_i_local.shape[0]
        self._send_rows = self.backend.index_tensor(
            np.asarray(matrix_slice.x_index_out_localized, dtype=np.int64))
        self.send_counts = [int(c) for c in matrix_slice.send_count]
        self.recv_counts = [int(c) for c in matrix_slice.recv_count]

    def spmm(self, X_local: torch.Tensor, Y_local: Optional[torch.Tensor] = None
             ) -> torch.Tensor:
        """Y (+)= A_i @ X, overlapping the neighbourhood exchange with the
        local multiply (reference spmm_cpu/spmm_gpu, spmm_petsc.py:179-307)."""
        be = self.backend
        X_local = be.asarray(X_local)
        k = X_local.shape[1]
        beta = 1
        if Y_local is None:
            Y_local = be.zeros((self.n_local, k))
            beta = 0

        # post the neighbourhood exchange (one buffer per peer)
        tic = time.perf_counter()
        sendbuf = be.gather_rows(X_local, self._send_rows)
        recv_future = self._alltoallv_begin(sendbuf)
        wb_logging.log({"comm_init_time": time.perf_counter() - tic})

        # local multiply while the exchange is in flight
        tic = time.perf_counter()
        be.spmm_block(self.A_local, X_local.contiguous(), Y_local, beta)
        wb_logging.log({"local_spmm_kernel_time": time.perf_counter() - tic})

        tic = time.perf_counter()
        X_nonlocal = self._alltoallv_end(recv_future)
        wb_logging.log({"receive_wait_time": time.perf_counter() - tic})

        tic = time.perf_counter()
        if self.A_nonlocal is not None and X_nonlocal.shape[0] > 0:
            be.spmm_block(self.A_nonlocal, X_nonlocal.contiguous(), Y_local, 1)
        elif beta == 0:
            pass  # Y already zero-filled by the local beta=0 multiply
        wb_logging.log({"nonlocal_spmm_kernel_time": time.perf_counter() - tic})
        return Y_local

    # The recv rows arrive ordered by source rank == ascending global column
    # (rank column ranges are contiguous), matching A_i_nonlocal's column
    # order (x_index_in sorted, matrix_slice.py:47).
    def _alltoallv_begin(self, sendbuf):
        return self.comm.alltoallv_async(sendbuf, self.send_counts,
                                         self.recv_counts)

    def _alltoallv_end(self, fut):
        recv, works = fut
        for w in works:
            w.wait()
        return recv
