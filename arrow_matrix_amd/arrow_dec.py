"""ArrowDecompositionMPI — multi-matrix orchestration of the hot path.

Re-implements the semantics of the reference's `arrow/arrow_dec_mpi.py`
(class of the same name): per iteration

  1. forward feature propagation matrix i -> i+1 along the composed
     permutations (_propagate_features_forwards, arrow_dec_mpi.py:507-610),
  2. per-matrix slim arrow SpMM (arrow_slim.py),
  3. backward partial-result aggregation matrix i -> i-1 with scatter-add
     (_aggregate_features_backwards, arrow_dec_mpi.py:404-505).

MI355X-first deviations:
  * SHARED-RANK layout: every rank hosts a contiguous stripe of EVERY
    decomposition part (the reference gives each part a disjoint rank set,
    needing sum(n_blocks) ranks). All parts' SpMMs run on all GPUs; the
    inter-part permutation exchange becomes ONE alltoallv over the node's
    xGMI links, with the rank-local share never leaving HBM.
    Consequently matrix_index == 0 on every rank and `B` is the part-0
    engine (the part that carries X, the reference's postcondition).
  * Permutation gathers/scatters run as device kernels (C ABI) instead of
    host fancy-indexing (arrow_dec_mpi.py:421,437,526,544).
  * The loader reads the decomposition on every rank (one node, shared
    filesystem, mmap) instead of root-scatter over MPI.
"""
import os
import sys
import time
import warnings
from typing import List, Optional

import numpy as np
import torch

from . import graphio, hip, tables
from .arrow_matrix import ArrowMatrix
from .arrow_slim import AffineStep, ArrowSlimMPI, normalizing_factors
from .comm import Comm, default_comm
from .common import wb_logging


class _Exchange:
    """Routing tables + index tensors for one matrix pair (i -> i+1)."""

    def __init__(self, send_counts, send_rows, recv_counts, recv_rows, backend):
        self.send_counts = [int(c) for c in send_counts]
        self.recv_counts = [int(c) for c in recv_counts]
        self.send_rows = backend.index_tensor(send_rows)
        self.recv_rows = backend.index_tensor(recv_rows)


class ArrowDecompositionMPI:

    def __init__(self, comm: Comm, engines: List[ArrowSlimMPI], n_blocks: np.ndarray,
                 width: int, n_feature_columns: int,
                 to_prev: List[Optional[np.ndarray]], to_next: List[Optional[np.ndarray]],
                 device: str = 'cpu'):
        self.comm = comm
        self.engines = engines
        self.n_blocks = np.asarray(n_blocks)
        self.decomposition_length = len(engines)
        self.matrix_index = 0  # shared-rank layout: every rank hosts part 0
        self.device = device
        self._n_rows_per_rank = width
        self._n_feature_columns = n_feature_columns
        self.width = width
        self._to_prev = to_prev
        self._to_next = to_next
        self._forward: List[Optional[_Exchange]] = []
        self._backward: List[Optional[_Exchange]] = []
        # folded-permutation mode (single process, L > 1): parts i >= 1 are
        # re-indexed through the composed forward/backward permutations into
        # part 0's X/C numbering and run as extra beta=1 SpMM launches — the
        # per-iteration permutation exchange disappears entirely (see
        # _build_folded). _fold_maps[i] = (M_i, R_i): part-i X row r reads
        # part-0 X row M_i[r]; part-i C row r accumulates into part-0 C row
        # R_i[r] (-1 = unmapped).
        self._folded: Optional[List] = None
        self._fold_maps: Optional[List] = None
        # affine step (set_affine_step): part 0's AffineStep or None
        self._affine: Optional[AffineStep] = None
        # step norms (track_step_norms): at L == 1 part 0's engine measures
        # its own step; at L > 1 this accumulator takes one stand-alone pass
        # over part 0's finished result
        self._norms_on = False
        self._norm_acc = None
        self._initialize_all_to_all_tables()

    @property
    def B(self) -> ArrowMatrix:
        return self.engines[0]

    # -- setup ---------------------------------------------------------------

    @staticmethod
    def initialize(comm: Optional[Comm], n_blocks: np.ndarray,
                   to_prev_permutation, to_next_permutation,
                   rows_per_rank: int, feature_columns: int, device: str = 'cpu',
                   block_diagonal: bool = True, slim: bool = True,
                   dtype=np.float32):
        """Factory, keeping the reference's signature
        (arrow_dec_mpi.py:106-177). to_prev/to_next are the per-rank
        permutation slices as returned by load_decomposition_new (lists with
        one entry per decomposition part). dtype (float32 or float64) is
        passed to every engine: on the GPU the precision is fixed here, at
        construction. torch.bfloat16 / 'bfloat16'
        selects bfloat16 features (device='gpu', one process)."""
        assert not slim or block_diagonal  # reference arrow_dec_mpi.py:131
        comm = comm if comm is not None else default_comm()
        if slim:
            engines = [ArrowSlimMPI(comm, tiles_per_side=int(nb), device=device,
                                    dtype=dtype)
                       for nb in n_blocks]
        else:
            from .arrow_mpi import ArrowMPI
            engines = [ArrowMPI(comm, is_block_diagonal=block_diagonal,
                                tiles_per_side=int(nb), device=device,
                                dtype=dtype)
                       for nb in n_blocks]
        return ArrowDecompositionMPI(comm, engines, n_blocks, rows_per_rank,
                                     feature_columns, to_prev_permutation,
                                     to_next_permutation, device=device)

    def _initialize_all_to_all_tables(self) -> None:
        """Build the forward/backward exchange tables
        (reference arrow_dec_mpi.py:210-281,325-384, generalised to the
        shared-rank layout in tables.routing_*_tables)."""
        P = self.comm.size
        w = self.width
        L = self.decomposition_length
        self._forward = [None] * L
        self._backward = [None] * L
        for i in range(L - 1):
            eng_s, eng_r = self.engines[i], self.engines[i + 1]
            own_s = tables.contiguous_block_owners(int(self.n_blocks[i]), P)
            own_r = tables.contiguous_block_owners(int(self.n_blocks[i + 1]), P)
            # forward (features i -> i+1): sender tables on my to_next slice
            # of matrix i, receiver tables on my to_prev slice of matrix i+1
            # to_prev/to_next are ALREADY this rank's slices (one per part,
            # as load_decomposition_new returns them — the reference's
            # loader also hands each rank its own slice,
            # arrow_dec_mpi.py:772-781)
            tn_i = self._checked_slice(self._to_next[i], eng_s)
            tp_n = self._checked_slice(self._to_prev[i + 1], eng_r)
            s_cnt, s_rows = tables.routing_send_tables(
                tn_i, w, own_r, int(self.n_blocks[i + 1]), P)
            r_cnt, r_rows = tables.routing_recv_tables(
                tp_n, w, own_s, int(self.n_blocks[i]), P)
            self._forward[i] = _Exchange(s_cnt, s_rows, r_cnt, r_rows, eng_s.backend)
            # backward (partials i+1 -> i): sender tables on my to_prev slice
            # of matrix i+1, receiver tables on my to_next slice of matrix i
            s_cnt, s_rows = tables.routing_send_tables(
                tp_n, w, own_s, int(self.n_blocks[i]), P)
            r_cnt, r_rows = tables.routing_recv_tables(
                tn_i, w, own_r, int(self.n_blocks[i + 1]), P)
            self._backward[i + 1] = _Exchange(s_cnt, s_rows, r_cnt, r_rows, eng_r.backend)
        if P == 1 and L > 1:
            self._compute_fold_maps()

    def _compute_fold_maps(self) -> None:
        """Compose the per-pair permutations into direct part-i -> part-0
        maps (single process only). Forward (features): part-i row s holds
        X_0[M_i[s]] — from to_next[i-1][r] = s (X_{i}[tn[r]] = X_{i-1}[r],
        the net effect of _propagate_features at P=1). Backward (results):
        part-i C row s accumulates into part-0 C row R_i[s] — from
        to_prev[i][s] (C_{i-1}[tp[s]] += C_i[s], the net effect of
        _aggregate at P=1). Sentinel/out-of-range entries map to -1."""
        w = self.width
        L = self.decomposition_length
        n0 = int(self.n_blocks[0]) * w
        M_prev = np.arange(n0, dtype=np.int64)
        R_prev = np.arange(n0, dtype=np.int64)
        self._fold_maps = [None]
        for i in range(1, L):
            ni = int(self.n_blocks[i]) * w
            n_prev = int(self.n_blocks[i - 1]) * w
            tn = np.asarray(self._to_next[i - 1], dtype=np.int64)
            tp = np.asarray(self._to_prev[i], dtype=np.int64)
            fmap = np.full(ni, -1, dtype=np.int64)
            valid = tn < ni
            fmap[tn[valid]] = np.flatnonzero(valid)
            M_i = np.where(fmap >= 0, M_prev[np.clip(fmap, 0, None)], -1)
            dmap = np.where(tp < n_prev, tp, -1)
            R_i = np.where(dmap >= 0, R_prev[np.clip(dmap, 0, None)], -1)
            self._fold_maps.append((M_i, R_i))
            M_prev, R_prev = M_i, R_i

    def _checked_slice(self, perm_slice: np.ndarray, engine: ArrowSlimMPI) -> np.ndarray:
        """Validate a per-rank permutation slice against the rank's span."""
        w = self.width
        expect = engine.n_owned * w
        perm_slice = np.asarray(perm_slice)
        assert perm_slice.size == expect, \
            f"permutation slice has {perm_slice.size} rows, rank owns {expect}"
        return perm_slice

    def load_data_from_blocks(self, blocked) -> None:
        """blocked: one block grid per decomposition part
        (reference arrow_dec_mpi.py:179-181).

        Folded-permutation mode (ARROW_FOLD, single process, L > 1): parts
        i >= 1 are re-indexed into part 0's numbering through the composed
        permutation maps and kept as extra resident structures instead of
        separate engines + per-step exchanges (see _build_folded). Falls
        back to the sequential path when the permutation chain does not
        cover every referenced row (the exchange would read rows no sender
        wrote)."""
        assert len(blocked) == self.decomposition_length
        # ARROW_FOLD: '0' sequential exchange, '1' full fold, '2' row fold
        # (backward cascade only), 'auto' (default): full fold in the
        # launch-bound / memory-pressure regimes, row fold otherwise at
        # world=1 on GPU (measured: row fold keeps part-i band locality
        # and removes the backward passes)
        fold_env = os.environ.get('ARROW_FOLD', 'auto')
        self._fold_cols = True
        # auto: fold only in the LAUNCH-BOUND small regime (part-0 rows <=
        # 4M). At larger scale the sequential path wins: materialising the
        # permuted X deduplicates the ~deg-many reads each part-i entry
        # would otherwise do through a random permutation (measured at 20M
        # rows L=2: fold 3060 vs sequential 3155 GF/s, and the gap grows
        # with size — profiles/r02_ab2_sweep.log L2_fold/L2_seq).
        n0_rows = int(self.n_blocks[0]) * self.width
        auto_fold = False
        if (fold_env == 'auto' and self._fold_maps is not None
                and self.comm.size == 1 and self.device == 'gpu'):
            auto_fold = n0_rows <= 4_000_000
            if not auto_fold:
                # fold also when the SEQUENTIAL layout's extra per-part
                # X/C buffers would not fit in HBM (fold keeps only part
                # 0's buffers): e.g. L=2 at 100M rows x k=128 needs ~260
                # GB sequentially but ~175 GB folded
                try:
                    free, total = torch.cuda.mem_get_info()
                    k = self._n_feature_columns
                    itemsize = self.engines[0].backend.feat_itemsize
                    need = [itemsize * k * (2 * eng.n_owned * self.width
                                     + 2 * self.width)
                            for eng in self.engines]
                    # sequential fits only if ALL parts' X/C buffers plus a
                    # 25% margin (caller-side feature stripe, structures,
                    # allocator slack) fit what is free now
                    auto_fold = sum(need) + 0.25 * total > free
                except Exception:
                    pass
        foldable = (self._fold_maps is not None and self.comm.size == 1
                    and len(blocked) > 1
                    and not any(getattr(e, 'banded', False)
                                for e in self.engines))
        # row fold (backward cascade only) is the default remaining-GPU
        # choice at world=1: keeps part-i X locality via the materialised
        # forward exchange while removing the backward passes
        want_row_fold = (foldable and fold_env == '2'
                         or (foldable and fold_env == 'auto'
                             and self.device == 'gpu' and not auto_fold))
        want_fold = foldable and (fold_env == '1' or auto_fold)
        if os.environ.get('ARROW_FOLD_DEBUG') == '1':
            print(f"# fold decision: full={want_fold} row={want_row_fold} "
                  f"auto={auto_fold} env={fold_env} "
                  f"maps={self._fold_maps is not None} "
                  f"P={self.comm.size} L={len(blocked)}", file=sys.stderr)
        if want_fold:
            self.engines[0].load_sparse_matrix_from_blocks(blocked[0])
            folded, dropped = self._build_folded(blocked, fold_cols=True)
            if folded is not None:
                self._folded = folded
                self._fold_cols = True
                return
            warnings.warn(
                f"ARROW_FOLD: {dropped} entries reference rows outside the "
                f"composed permutation chain; falling back to the "
                f"sequential exchange path")
            for eng, blocks in zip(self.engines[1:], blocked[1:]):
                eng.load_sparse_matrix_from_blocks(blocks)
            return
        if want_row_fold:
            self.engines[0].load_sparse_matrix_from_blocks(blocked[0])
            folded, _ = self._build_folded(blocked, fold_cols=False)
            self._folded = folded
            self._fold_cols = False
            return
        for eng, blocks in zip(self.engines, blocked):
            eng.load_sparse_matrix_from_blocks(blocks)

    def _build_folded(self, blocked, fold_cols=True):
        """Build one re-indexed structure per part i >= 1.

        fold_cols=True (FULL fold): entry (r, c, v) of part i becomes
        (R_i[r], M_i[c], v) — a direct contribution
        C_0[R_i[r]] += v * X_0[M_i[c]] — so part i runs as one beta=1 SpMM
        against part 0's buffers with NO permutation exchange at all.
        Returns (None, n_dropped) when entries fall outside the composed
        maps (the exchange would read rows no sender wrote).

        fold_cols=False (ROW fold): only the BACKWARD cascade folds —
        entry (r, c, v) becomes (R_i[r], c, v) reading part i's OWN
        exchanged features X_i (the forward permutation still
        materialises X_i, preserving part i's banded X locality) and
        accumulating straight into part 0's C. This removes the backward
        gather + scatter-add passes (3 stripe sweeps) at the cost of one
        C read-modify-write inside the launch. Rows with R_i < 0 are rows
        whose results the sequential cascade DISCARDS (never sent
        backwards) — dropped here identically, not an error.

        Per output row the accumulation order equals the sequential
        path's (each part-i row is summed as its own work item, then
        added once)."""
        w = self.width
        eng0 = self.engines[0]
        be = eng0.backend
        n0 = int(self.n_blocks[0]) * w
        gpu = be.device == 'cuda'
        folded = []
        for i in range(1, self.decomposition_length):
            M_i, R_i = self._fold_maps[i]
            ni = int(self.n_blocks[i]) * w
            rows_l, cols_l, data_l = [], [], []
            for br, rowlist in enumerate(blocked[i]):
                for bc, blk in enumerate(rowlist):
                    if blk is None:
                        continue
                    csr = blk.tocsr()
                    rows_l.append(np.repeat(
                        np.arange(csr.shape[0], dtype=np.int64),
                        np.diff(csr.indptr)) + br * w)
                    cols_l.append(csr.indices.astype(np.int64) + bc * w)
                    data_l.append(csr.data.astype(eng0.np_dtype))
            rows = np.concatenate(rows_l) if rows_l else np.empty(0, np.int64)
            cols = np.concatenate(cols_l) if cols_l else np.empty(0, np.int64)
            data = np.concatenate(data_l) if data_l else np.empty(0, eng0.np_dtype)
            nr = R_i[np.clip(rows, 0, None)]
            if fold_cols:
                nc = M_i[np.clip(cols, 0, None)]
                keep = (nr >= 0) & (nc >= 0)
                n_drop = int(rows.size - keep.sum())
                if n_drop:
                    return None, n_drop
            else:
                nc = cols
                keep = nr >= 0  # discarded-by-the-cascade rows drop
            rows_k = rows[keep]
            nr, nc, data = nr[keep], nc[keep], data[keep]
            n_cols = n0 if fold_cols else ni
            # STRUCTURE ORDER decides the queue scheduler's X window. FULL
            # fold reads part-0 X through the composed map (random either
            # way) — group by TARGET row so C writes walk in order. ROW
            # fold reads part i's own X — keep SOURCE-row order so the
            # banded X window survives (the scatter lives in row_ids;
            # target-ordered was measured -17% at 20M L=2); writes stay
            # exclusive either way (R_i is injective).
            key = nr if fold_cols else rows_k
            order = np.argsort(key, kind='stable')
            key_s = key[order]
            nr, nc, data = nr[order], nc[order], data[order]
            uniq_key, starts, counts = np.unique(key_s, return_index=True,
                                                 return_counts=True)
            uniq = nr[starts]  # target row of each structure row
            indptr = np.zeros(uniq_key.size + 1, dtype=np.int64)
            np.cumsum(counts, out=indptr[1:])
            if gpu:
                h = be.upload_arrays((uniq.size, n_cols), indptr,
                                     nc.astype(np.int32), data,
                                     row_ids=uniq.astype(np.int64))
                h.x_rows = n_cols
                folded.append(h)
            else:
                from scipy import sparse
                csr = sparse.csr_matrix(
                    (data.astype(be.np_dtype), nc.astype(np.int64), indptr),
                    shape=(uniq.size, n_cols))
                folded.append((csr, uniq))
        return folded, 0

    def zero_rhs(self, width: int, n_features: int, dtype=np.float32) -> None:
        for i, eng in enumerate(self.engines):
            if self._folded is not None and self._fold_cols and i > 0:
                continue  # FULL-folded parts have no buffers of their own
                # (row-folded parts keep X/C for the forward exchange)
            eng.zero_rhs(width, n_features, dtype=dtype)

    # -- affine step ---------------------------------------------------------

    def set_affine_step(self, alpha: float = 1.0, gamma: float = 0.0,
                        residual=None) -> None:
        """Make every later step() compute X <- alpha * A@X + gamma * R on
        the whole decomposition (A the recomposed matrix). `residual` is in
        part 0's layout, like the features given to B.set_features; part 0's
        engine copies it into a buffer of its own (ArrowSlimMPI.
        set_affine_step). Call after zero_rhs. Single process only. On the
        GPU the default single-launch layout and both folds carry the step
        inside their launches; every other layout runs one tail kernel on
        part 0's finished result."""
        if self.comm.size > 1:
            raise NotImplementedError(
                "the affine step is single-process only (no multi-GPU rig "
                "to validate the reduced block row 0 against)")
        eng0 = self.engines[0]
        eng0.set_affine_step(alpha, gamma, residual)
        self._affine = eng0._affine

    def clear_affine_step(self) -> None:
        self._affine = None
        self.engines[0].clear_affine_step()

    def _affine_inside(self) -> bool:
        """Who finishes the affine step of the decomposition, decided here
        alone: True when part 0's own step (ArrowSlimMPI._spmm_step, which
        asks its _launch_finishes_step) and the folded launches carry it;
        False when step() runs the plain step and then the tail on part 0's
        aggregated result."""
        if self.decomposition_length == 1:
            return True
        return (self._folded is not None
                and self.engines[0].backend.device == 'cuda')

    # -- step norms ----------------------------------------------------------

    def track_step_norms(self, on: bool = True) -> None:
        """Make every later step() also measure itself: sum (C - X)^2 and
        sum C^2 over part 0's finished result C against part 0's features X
        before the step (DESIGN.md §step norms). L = 1 measures inside part
        0's own spmm() (fused into the default single launch on the GPU);
        both folds and the sequential L > 1 layout run one stand-alone pass
        after the last launch, aggregate or tail. The accumulator is
        allocated here, never inside step(). Single process only."""
        if on and self.comm.size > 1:
            raise NotImplementedError(
                "step norms are single-process only: block row 0 would have "
                "to be counted exactly once across ranks, and there is no "
                "multi-GPU rig to validate that")
        eng0 = self.engines[0]
        self._norms_on = bool(on)
        if self.decomposition_length == 1:
            eng0.track_step_norms(on)
        else:
            self._norm_acc = eng0.backend.norm_acc() if on else None

    def last_step_norms(self):
        """(||C - X_prev||_2, ||C||_2) of the last step() as floats.
        Synchronises and reads 16 bytes."""
        if not self._norms_on:
            raise RuntimeError("last_step_norms: call track_step_norms() "
                               "before the step")
        if self.decomposition_length == 1:
            return self.engines[0].last_step_norms()
        d2, c2 = self._norm_acc.tolist()
        return float(np.sqrt(d2)), float(np.sqrt(c2))

    def iterate(self, max_steps: int, tol: float = None,
                check_every: int = 1):
        """Run step() up to max_steps times, feeding part 0's result back as
        its features after every step, and return (steps_done, rel) with
        rel = ||X_new - X_old||_2 / ||X_new||_2 of the last step read. rel is
        read every check_every steps (and after the last one); the loop stops
        when tol is not None and rel <= tol. Turns step-norm tracking on.
        Single process only."""
        if self.comm.size > 1:
            raise NotImplementedError(
                "iterate is single-process only, as the step norms it reads")
        if max_steps < 1 or check_every < 1:
            raise ValueError("iterate: max_steps and check_every must be >= 1")
        if not self._norms_on:
            self.track_step_norms()
        eng0 = self.engines[0]
        rel = float('nan')
        for t in range(1, max_steps + 1):
            self.step()
            eng0.set_features(eng0.result_tile())
            if t % check_every == 0 or t == max_steps:
                d, c = self.last_step_norms()
                rel = d / c if c > 0.0 else (0.0 if d == 0.0 else float('inf'))
                if tol is not None and rel <= tol:
                    return t, rel
        return max_steps, rel

    # -- operator scaling ----------------------------------------------------

    def _operator_parts(self):
        """The recomposed matrix as its resident pieces beyond part 0, each
        (i, piece, rows_folded, cols_folded): piece is part i's engine, or
        its folded structure; rows_folded / cols_folded say that the piece's
        rows / columns are already in part 0's layout (else in part i's,
        reached through _fold_maps[i] = (M_i, R_i))."""
        for i in range(1, self.decomposition_length):
            if self._folded is None:
                yield i, self.engines[i], False, False
            else:
                yield i, self._folded[i - 1], True, self._fold_cols

    def _check_operator_scaling(self, who: str) -> int:
        if self.comm.size > 1:
            raise NotImplementedError(
                f"{who} is single-process only (no multi-GPU rig to validate "
                f"the reduced sums and the broadcast factors against)")
        return int(self.n_blocks[0]) * self.width

    @staticmethod
    def _gather_factors(v, index):
        """v[index] with the factor 0 where index is -1 (rows the cascade
        discards, feature rows no part-0 row feeds); None stays None."""
        if v is None:
            return None
        return np.where(index >= 0, v[np.clip(index, 0, None)], 0.0)

    def operator_sums(self, absolute: bool = False):
        """(row_sums, col_sums) of the RECOMPOSED matrix: float64 numpy
        vectors of n_blocks[0] * width entries in part 0's layout, exactly
        as features and the residual are. Every resident structure is summed
        on the device (arrow_csr_sums); the per-part vectors are routed into
        part 0's layout on the host, once (DESIGN.md §operator scaling).
        Single process only."""
        n0 = self._check_operator_scaling('operator_sums')
        eng0 = self.engines[0]
        be = eng0.backend
        absolute = bool(absolute)
        rows, cols = eng0._operator_sums_stripe(absolute)
        for i, piece, rows_folded, cols_folded in self._operator_parts():
            M_i, R_i = self._fold_maps[i]
            if isinstance(piece, ArrowSlimMPI):
                ri, ci = piece._operator_sums_stripe(absolute)
            else:
                ni = int(self.n_blocks[i]) * self.width
                rv = be.scale_vector(np.zeros(n0))
                cv = be.scale_vector(np.zeros(n0 if cols_folded else ni))
                be.block_sums(piece, rv, cv, None, absolute)
                be.synchronize()
                ri, ci = rv.cpu().numpy(), cv.cpu().numpy()
            if rows_folded:
                rows += ri
            else:
                np.add.at(rows, R_i[R_i >= 0], ri[R_i >= 0])
            if cols_folded:
                cols += ci
            else:
                np.add.at(cols, M_i[M_i >= 0], ci[M_i >= 0])
        return rows, cols

    def scale_operator(self, row_scale=None, col_scale=None) -> None:
        """A <- diag(row_scale) A diag(col_scale) on the recomposed matrix,
        in place on the resident values of every part (arrow_csr_scale; one
        rounding per value). Vectors in part 0's layout, None is no factor:
        part i takes row_scale[R_i] and col_scale[M_i] through the fold maps.
        Needs no zero_rhs; feature buffers, the affine step and a captured
        graph stay valid. Single process only."""
        n0 = self._check_operator_scaling('scale_operator')
        eng0 = self.engines[0]
        be = eng0.backend
        r = eng0._stripe_vector('scale_operator', 'row_scale', row_scale, n0)
        c = eng0._stripe_vector('scale_operator', 'col_scale', col_scale, n0)
        if r is None and c is None:
            return
        eng0._operator_scale_stripe(r, c)
        for i, piece, rows_folded, cols_folded in self._operator_parts():
            M_i, R_i = self._fold_maps[i]
            ri = r if rows_folded else self._gather_factors(r, R_i)
            ci = c if cols_folded else self._gather_factors(c, M_i)
            if isinstance(piece, ArrowSlimMPI):
                piece._operator_scale_stripe(ri, ci)
            else:
                be.block_scale(piece,
                               None if ri is None else be.scale_vector(ri),
                               None if ci is None else be.scale_vector(ci),
                               None)
                be.synchronize()

    def normalize_operator(self, kind: str, absolute: bool = False):
        """Normalise the recomposed matrix ('row': D^-1 A, 'col': A D^-1,
        'sym': D_r^-1/2 A D_c^-1/2; see ArrowSlimMPI.normalize_operator) and
        return the (row_scale, col_scale) applied, in part 0's layout.
        operator_sums followed by scale_operator, nothing else."""
        row_sums, col_sums = self.operator_sums(absolute)
        r, c = normalizing_factors(kind, row_sums, col_sums)
        self.scale_operator(r, c)
        return r, c

    # -- iteration -----------------------------------------------------------

    def step(self) -> None:
        """One iteration; with an affine step set, X <- alpha*A@X + gamma*R
        (see _step_affine for the step itself). With step norms tracked at
        L > 1, one pass over part 0's finished result follows."""
        if self._norm_acc is None:
            self._step_affine()
            return
        eng0 = self.engines[0]
        X_pre = eng0.feature_tile()  # its buffer is not written by the step
        self._step_affine()
        self._norm_acc.zero_()
        eng0.backend.diffnorm_rows(eng0.C_i, X_pre, self._norm_acc)

    def _step_affine(self) -> None:
        """The step with what _affine_inside() decided handed down as an
        argument: part 0's engine state is read, never written."""
        if self._affine is None:
            # part 0 applies whatever was set on its engine directly
            self._step_plain(self.engines[0]._affine)
        elif self._affine_inside():
            self._step_plain(self._affine)
        else:
            self._step_plain(None)
            self.engines[0]._affine_tail(self._affine)

    def _spmm_part(self, i: int, affine: Optional[AffineStep]) -> None:
        """Part i's arrow SpMM; part 0 applies `affine` (None: plain)."""
        eng = self.engines[i]
        if i == 0:
            eng._spmm_step(affine, eng._norm_acc)
        else:
            eng.spmm()

    def _step_plain(self, affine: Optional[AffineStep] = None) -> None:
        """One X <- A @ X iteration (reference arrow_dec_mpi.py:283-307), or
        with `affine` the affine step inside part 0's launches.
        At world>1 with L>1 the forward exchange for pair (i, i+1) is
        POSTED asynchronously and part i's SpMM runs while the transfer is
        in flight — the reference's own overlap (the Ialltoallv posted at
        arrow_dec_mpi.py:304 is waited only after the local compute at
        :306). Data dependencies (and results) are identical to the
        sequential schedule."""
        if self._folded is not None:
            self._step_folded(affine)
            return
        if self.comm.size > 1 and self.decomposition_length > 1:
            tic = time.perf_counter()
            self._step_overlapped_forward(affine)
            wb_logging.log({'spmm_arrow_time': time.perf_counter() - tic})
        else:
            tic = time.perf_counter()
            self._propagate_features()
            wb_logging.log({"spmm_bcast_time": time.perf_counter() - tic})
            tic = time.perf_counter()
            for i in range(self.decomposition_length):
                self._spmm_part(i, affine)
            wb_logging.log({'spmm_arrow_time': time.perf_counter() - tic})

        tic = time.perf_counter()
        self._aggregate()
        wb_logging.log({"spmm_reduce_time": time.perf_counter() - tic})

    def _step_overlapped_forward(self, affine=None) -> None:
        """Forward exchange posted async, overlapped with the previous
        part's SpMM (world>1). Same dependency chain as
        _propagate_features + the spmm loop: exchange i reads part i's
        features (set by exchange i-1), part i+1's features are set before
        its spmm."""
        L = self.decomposition_length
        pending = None
        for i in range(L):
            if pending is not None:
                ex, recvbuf, works = pending
                for wk in works:
                    wk.wait()
                eng_r = self.engines[i]
                eng_r.backend.scatter_rows(eng_r.C_i, ex.recv_rows, recvbuf)
                eng_r._x0_valid = False
                eng_r.set_features(eng_r.C_i)
                pending = None
            if i < L - 1:
                ex = self._forward[i]
                eng_s = self.engines[i]
                sendbuf = eng_s.backend.gather_rows(eng_s.feature_tile(),
                                                    ex.send_rows)
                recvbuf, works = self.comm.alltoallv_async(
                    sendbuf, ex.send_counts, ex.recv_counts)
                pending = (ex, recvbuf, works)
            self._spmm_part(i, affine)

    def _step_folded(self, affine: Optional[AffineStep] = None) -> None:
        """Folded iteration: part 0's arrow SpMM, then each folded part as
        one beta=1 SpMM accumulating into part 0's fresh C — results
        identical to the sequential propagate/spmm/aggregate cascade (same
        per-row sums). FULL fold reads part 0's pre-step X through the
        composed maps (no exchange at all); ROW fold first materialises
        each part's X via the forward exchange (band locality kept) and
        folds only the backward cascade into the launch's output rows."""
        eng0 = self.engines[0]
        # affine step: part 0's launch carried alpha and gamma * R, the
        # folded beta=1 launches carry alpha only
        alpha = affine.alpha if affine is not None else 1.0
        if not self._fold_cols:
            tic = time.perf_counter()
            self._propagate_features()
            wb_logging.log({"spmm_bcast_time": time.perf_counter() - tic})
        X_pre = eng0.feature_tile()
        tic = time.perf_counter()
        self._spmm_part(0, affine)
        for i, h in enumerate(self._folded, start=1):
            X_op = X_pre if self._fold_cols \
                else self.engines[i].feature_tile()
            if eng0.backend.device == 'cuda':
                eng0._timed(lambda h=h, X_op=X_op: eng0.backend.spmm_block(
                    h, X_op, eng0.C_i, 1, alpha=alpha),
                    h.nnz, h.shape[0], h.x_rows)
            else:
                csr, rid = h
                eng0.C_i.numpy()[rid] += csr @ X_op.numpy()
        # C was mutated after the C_0 head was captured: any cached X_0
        # (the allreduce_x0 fast path) is stale now
        eng0._x0_valid = False
        wb_logging.log({'spmm_arrow_time': time.perf_counter() - tic})

    def _propagate_features(self) -> None:
        """Forward: route matrix i's features to matrix i+1 along the
        composed permutation (arrow_dec_mpi.py:507-610)."""
        for i in range(self.decomposition_length - 1):
            ex = self._forward[i]
            eng_s, eng_r = self.engines[i], self.engines[i + 1]
            if self.comm.size == 1:
                # rank-local: one fused permute pass, no staging buffers
                eng_r.backend.permute_rows(eng_r.C_i, ex.recv_rows,
                                           eng_s.feature_tile(), ex.send_rows)
            else:
                sendbuf = eng_s.backend.gather_rows(eng_s.feature_tile(), ex.send_rows)
                recvbuf = self.comm.alltoallv(sendbuf, ex.send_counts, ex.recv_counts)
                # C_i[recv_perm] = recvbuf; X := C (arrow_dec_mpi.py:544-545)
                eng_r.backend.scatter_rows(eng_r.C_i, ex.recv_rows, recvbuf)
            # the exchange mutated C in place: any cached X_0 (the
            # allreduce_x0 fast path) is stale now
            eng_r._x0_valid = False
            eng_r.set_features(eng_r.C_i)

    def _aggregate(self) -> None:
        """Backward: cascade partial results matrix i -> i-1 with
        scatter-add (arrow_dec_mpi.py:404-505)."""
        for i in reversed(range(1, self.decomposition_length)):
            ex = self._backward[i]
            eng_s, eng_r = self.engines[i], self.engines[i - 1]
            if self.comm.size == 1:
                eng_r.backend.permute_add_rows(eng_r.C_i, ex.recv_rows,
                                               eng_s.result_tile(), ex.send_rows)
            else:
                sendbuf = eng_s.backend.gather_rows(eng_s.result_tile(), ex.send_rows)
                recvbuf = self.comm.alltoallv(sendbuf, ex.send_counts, ex.recv_counts)
                # C_i[recv_perm] += recvbuf; X := C (arrow_dec_mpi.py:437-438)
                eng_r.backend.scatter_add_rows(eng_r.C_i, ex.recv_rows, recvbuf)
            eng_r._x0_valid = False  # C mutated after spmm; cached X_0 stale
            eng_r.set_features(eng_r.C_i)

    # -- loading -------------------------------------------------------------

    @staticmethod
    def number_of_blocks(adjacency, width: int) -> int:
        """Reference arrow_dec_mpi.py:612-627."""
        if isinstance(adjacency, tuple):
            indptr = adjacency[2]
            nnz_per_row = np.asarray(indptr[1:]) - np.asarray(indptr[:-1])
        else:
            nnz_per_row = adjacency.getnnz(1)
        return tables.number_of_blocks(nnz_per_row, width)

    @staticmethod
    def load_decomposition_new(comm: Optional[Comm], filename: str, width: int,
                               is_block_diagonal: bool = True, datatype=np.float32,
                               slim: bool = True, use_npy: bool = True,
                               use_mmap: bool = True):
        """Load a decomposed graph and build this rank's blocks + permutation
        slices. Keeps the reference's signature and return shape
        (arrow_dec_mpi.py:629-930): returns
        (blocks, n_blocks, to_prev, to_next) — here `blocks` is one grid per
        part and to_prev/to_next are per-part lists of this rank's slices
        (the shared-rank layout hosts every part on every rank).

        Every rank reads the files itself (single node, shared FS, mmap) —
        no root scatter. Zero-block cutting, permutation padding /
        one-based normalisation / overflow sentinel follow
        arrow_dec_mpi.py:680-749 exactly (tables.pad_and_compose_permutations).
        """
        comm = comm if comm is not None else default_comm()
        P = comm.size
        rank = comm.rank

        if use_npy:
            decomposition = graphio.load_decomposition_new(
                filename, width, block_diagonal=is_block_diagonal, mem_map=use_mmap)
        else:
            decomposition = graphio.load_decomposition(
                filename, width, block_diagonal=is_block_diagonal)
        if len(decomposition) == 0:
            raise FileNotFoundError(
                f"decomposition {filename!r} width={width} not found")

        n_blocks = np.zeros(len(decomposition), dtype=np.int32)
        for i, (adjacency, _) in enumerate(decomposition):
            n_blocks[i] = ArrowDecompositionMPI.number_of_blocks(adjacency, width)

        perms = [p for _, p in decomposition]
        _, to_prev_full, to_next_full = tables.pad_and_compose_permutations(
            perms, n_blocks, width)

        blocks_per_part = []
        to_prev_sliced: List[Optional[np.ndarray]] = []
        to_next_sliced: List[Optional[np.ndarray]] = []
        for i, (adjacency, _) in enumerate(decomposition):
            nb = int(n_blocks[i])
            bpr = -(-nb // P)
            first = min(rank * bpr, nb)
            last = min(first + bpr, nb)
            from scipy import sparse
            if isinstance(adjacency, tuple):
                data, indices, indptr = adjacency
            else:
                data, indices, indptr = adjacency.data, adjacency.indices, adjacency.indptr
            # adjacency matrices are square (reference asserts this,
            # graphio.py:427); build with the explicit n x n shape instead of
            # inferring cols from max(indices)+1 as csr_matrix would
            n_rows = indptr.size - 1
            A = sparse.csr_matrix((data, indices, indptr), shape=(n_rows, n_rows))
            # bfloat16 is a FEATURE dtype: A stays float32 under it
            A = A.astype(np.float32 if hip.is_bf16(datatype) else datatype)
            grid: List[List[Optional[object]]] = [[None] * nb for _ in range(nb)]
            # first block-row tiles for owned columns; diagonal + first
            # block-column for owned rows (slim layout,
            # arrow_slim_mpi.py:298-326)
            for c in range(first, last):
                grid[0][c] = _extract_block(A, 0, c, width)
            for r in range(max(first, 1), last):
                grid[r][r] = _extract_block(A, r, r, width)
                grid[r][0] = _extract_block(A, r, 0, width)
                if not is_block_diagonal:
                    # banded off-diagonals (reference sends A_ii-1/A_ii+1,
                    # arrow_dec_mpi.py:804-815)
                    if r >= 2:
                        grid[r][r - 1] = _extract_block(A, r, r - 1, width)
                    if r < nb - 1:
                        grid[r][r + 1] = _extract_block(A, r, r + 1, width)
            blocks_per_part.append(grid)
            w = width
            tp = to_prev_full[i]
            tn = to_next_full[i]
            to_prev_sliced.append(None if tp is None else tp[first * w:last * w])
            to_next_sliced.append(None if tn is None else tn[first * w:last * w])

        return blocks_per_part, n_blocks, to_prev_sliced, to_next_sliced


def _extract_block(A, i: int, j: int, block_size: int):
    """Extract block (i, j) with the reference's split semantics
    (graphio.py:361-406 / load_block_from_bslice:449-495): short last
    block-row edge-padded to block_size and declared square."""
    from scipy import sparse
    rows, cols = A.shape
    r0, r1 = i * block_size, min(rows, (i + 1) * block_size)
    c0, c1 = j * block_size, min(cols, (j + 1) * block_size)
    sl = A[r0:r1, c0:c1]
    pad_width = block_size - (r1 - r0)
    # Always square (block_size, block_size): the reference pads only short
    # last block-ROWS (graphio.py:394-399) and asserts squareness at load
    # (arrow_slim_mpi.py:305), which breaks on a ragged last block-COLUMN;
    # declaring the full square shape (extra rows/cols are empty) keeps the
    # engine's uniform tiles with identical results.
    if pad_width == 0:
        block = sparse.csr_matrix((sl.data, sl.indices, sl.indptr),
                                  shape=(block_size, block_size))
    else:
        indx_ptr = np.pad(sl.indptr, (0, pad_width), mode='edge')
        block = sparse.csr_matrix((sl.data, sl.indices, indx_ptr),
                                  shape=(block_size, block_size))
    block.sum_duplicates()
    block.sort_indices()
    return block
