"""HIP kernel parity vs the scipy oracle arithmetic — runs on a real MI355X
(`pytest -m gpu`). Covers the reference's operating points (k = 16/32/128,
arrow_bench defaults) plus edge cases: empty matrices, empty rows, ragged k,
dense hub rows (the long-row atomic path), k > 256 column tiling,
beta accumulate."""
import numpy as np
import pytest
import torch
from scipy import sparse

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from arrow_matrix_amd import hip
    hip.set_device(torch.cuda.current_device())
    return hip


def _random_csr(rows, cols, density, seed, dtype=np.float32):
    rs = np.random.RandomState(seed)
    m = sparse.random(rows, cols, density=density, format='csr', random_state=rs,
                      dtype=np.float64)
    return sparse.csr_matrix(m, dtype=dtype)


def _check_spmm(gpu, A, k, beta, seed=0, rtol=1e-5, atol=1e-5):
    rng = np.random.default_rng(seed)
    X = (2 * rng.random((A.shape[1], k)) - 1).astype(np.float32)
    C0 = (2 * rng.random((A.shape[0], k)) - 1).astype(np.float32)
    Xt = torch.from_numpy(X).cuda()
    Ct = torch.from_numpy(C0.copy()).cuda()
    blk = gpu.CsrBlockGPU(A)
    blk.spmm(Xt.data_ptr(), Ct.data_ptr(), k, beta,
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ref = (A @ X) + (C0 if beta else 0)
    got = Ct.cpu().numpy()
    scale = max(1.0, float(np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol * scale)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 32, 64, 128])
def test_spmm_k_sweep(gpu, k):
    A = _random_csr(500, 700, 0.02, seed=k)
    _check_spmm(gpu, A, k, beta=0, seed=k)


@pytest.mark.parametrize("k", [16, 128])
def test_spmm_accumulate(gpu, k):
    A = _random_csr(300, 300, 0.05, seed=40 + k)
    _check_spmm(gpu, A, k, beta=1, seed=k)


def test_spmm_k_above_column_tile(gpu):
    # k > 256 exercises the column-offset loop; 260 also the guard
    for k in (260, 512):
        A = _random_csr(100, 120, 0.05, seed=k)
        _check_spmm(gpu, A, k, beta=0, seed=k)


def test_spmm_empty_matrix(gpu):
    A = sparse.csr_matrix((64, 64), dtype=np.float32)
    _check_spmm(gpu, A, 16, beta=0)   # beta=0 must zero all rows
    _check_spmm(gpu, A, 16, beta=1)   # beta=1 must leave C unchanged


def test_spmm_empty_rows_beta0_zeroes(gpu):
    A = _random_csr(200, 200, 0.02, seed=3).tolil()
    A[50:100] = 0
    A = sparse.csr_matrix(A, dtype=np.float32)
    _check_spmm(gpu, A, 32, beta=0)


def test_spmm_dense_hub_rows_long_row_split(gpu):
    """Rows with nnz >> SEG_NNZ take the segmented atomic path."""
    rows, cols = 64, 20000
    A = _random_csr(rows, cols, 0.001, seed=5).tolil()
    rs = np.random.RandomState(6)
    for r in (0, 13):
        A[r] = rs.rand(cols) * (rs.rand(cols) < 0.6)  # ~12000 nnz
    A = sparse.csr_matrix(A, dtype=np.float32)
    assert int(A.getnnz(1).max()) > 2048
    for beta in (0, 1):
        _check_spmm(gpu, A, 128, beta=beta, rtol=1e-4, atol=1e-4)


def test_spmm_single_row_single_col(gpu):
    A = sparse.csr_matrix(np.array([[2.5]], dtype=np.float32))
    _check_spmm(gpu, A, 7, beta=0)


def test_spmm_dual_negative_columns(gpu):
    """arrow_spmm_dual: negative-encoded columns read the second operand."""
    rng = np.random.default_rng(7)
    rows, n0, n1, k = 200, 150, 60, 32
    A0 = _random_csr(rows, n0, 0.05, seed=70)
    A1 = _random_csr(rows, n1, 0.08, seed=71)
    # merged arrays: per row, A0 entries then A1 entries (negative encoding)
    indptr = np.zeros(rows + 1, dtype=np.int64)
    cols, vals = [], []
    for r in range(rows):
        c0 = A0.indices[A0.indptr[r]:A0.indptr[r + 1]]
        v0 = A0.data[A0.indptr[r]:A0.indptr[r + 1]]
        c1 = A1.indices[A1.indptr[r]:A1.indptr[r + 1]]
        v1 = A1.data[A1.indptr[r]:A1.indptr[r + 1]]
        cols.append(np.concatenate([c0.astype(np.int64),
                                    -(c1.astype(np.int64) + 1)]))
        vals.append(np.concatenate([v0, v1]))
        indptr[r + 1] = indptr[r] + cols[-1].size
    cols = np.concatenate(cols).astype(np.int32)
    vals = np.concatenate(vals).astype(np.float32)
    blk = gpu.CsrBlockGPU(arrays=((rows, n0), indptr, cols, vals))
    X0 = (2 * rng.random((n0, k)) - 1).astype(np.float32)
    X1 = (2 * rng.random((n1, k)) - 1).astype(np.float32)
    X0t = torch.from_numpy(X0).cuda()
    X1t = torch.from_numpy(X1).cuda()
    Ct = torch.empty((rows, k), dtype=torch.float32, device='cuda')
    blk.spmm_dual(X0t.data_ptr(), X1t.data_ptr(), Ct.data_ptr(), k, 0,
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ref = A0 @ X0 + A1 @ X1
    np.testing.assert_allclose(Ct.cpu().numpy(), ref, rtol=1e-5, atol=1e-5)


def test_gather_scatter_roundtrip(gpu):
    rng = np.random.default_rng(0)
    for k in (4, 16, 33, 128):
        n = 500
        src = torch.from_numpy(rng.random((n, k), dtype=np.float32)).cuda()
        idx_np = rng.permutation(n).astype(np.int64)
        idx = torch.from_numpy(idx_np).cuda()
        dst = torch.empty_like(src)
        s = torch.cuda.current_stream().cuda_stream
        gpu.gather_rows(src.data_ptr(), dst.data_ptr(), idx.data_ptr(), n, k, s)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(dst.cpu().numpy(), src.cpu().numpy()[idx_np])
        # scatter back inverts
        dst2 = torch.empty_like(src)
        gpu.scatter_rows(dst2.data_ptr(), dst.data_ptr(), idx.data_ptr(), n, k, s)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(dst2.cpu().numpy(), src.cpu().numpy())


def test_scatter_add(gpu):
    rng = np.random.default_rng(1)
    n, m, k = 300, 200, 16
    src = rng.random((n, k), dtype=np.float32)
    base = rng.random((m, k), dtype=np.float32)
    idx_np = rng.integers(0, m, size=n).astype(np.int64)  # duplicate targets? no:
    # duplicates in idx would race in the kernel unless atomics; the routing
    # use-case (receive permutation) is duplicate-free — enforce that here
    idx_np = rng.permutation(m)[:min(n, m)].astype(np.int64)
    src = src[:idx_np.size]
    dst = torch.from_numpy(base.copy()).cuda()
    s = torch.cuda.current_stream().cuda_stream
    srct = torch.from_numpy(src).cuda()
    idxt = torch.from_numpy(idx_np).cuda()
    from arrow_matrix_amd import hip
    hip.scatter_add_rows(dst.data_ptr(), srct.data_ptr(), idxt.data_ptr(),
                         idx_np.size, k, s)
    torch.cuda.synchronize()
    ref = base.copy()
    ref[idx_np] += src
    np.testing.assert_allclose(dst.cpu().numpy(), ref, rtol=1e-6, atol=1e-6)


def _check_spmm_queue(gpu, A, k, beta, seed=0, rtol=1e-5, atol=1e-5):
    """Same parity check but with the per-XCD queue scheduler forced on."""
    rng = np.random.default_rng(seed)
    X = (2 * rng.random((A.shape[1], k)) - 1).astype(np.float32)
    C0 = (2 * rng.random((A.shape[0], k)) - 1).astype(np.float32)
    Xt = torch.from_numpy(X).cuda()
    Ct = torch.from_numpy(C0.copy()).cuda()
    blk = gpu.CsrBlockGPU(A)
    blk.set_queue(1)
    blk.spmm(Xt.data_ptr(), Ct.data_ptr(), k, beta,
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ref = (A @ X) + (C0 if beta else 0)
    got = Ct.cpu().numpy()
    scale = max(1.0, float(np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol * scale)


@pytest.mark.parametrize("k", [1, 3, 8, 16, 32, 128])
def test_spmm_queue_k_sweep(gpu, k):
    A = _random_csr(500, 700, 0.02, seed=100 + k)
    _check_spmm_queue(gpu, A, k, beta=0, seed=k)


@pytest.mark.parametrize("beta", [0, 1])
def test_spmm_queue_beta(gpu, beta):
    A = _random_csr(300, 300, 0.05, seed=7)
    _check_spmm_queue(gpu, A, k=128, beta=beta, seed=9)


def test_spmm_queue_hub_split_rows(gpu):
    """Queue scheduler with >SEG_NNZ rows (atomic split path) and empty rows."""
    rows, cols, k = 400, 5000, 128
    rs = np.random.RandomState(3)
    A = sparse.random(rows, cols, density=0.002, format='lil', random_state=rs,
                      dtype=np.float64)
    A[7, :] = rs.rand(cols)   # dense hub rows -> split items
    A[101, :] = rs.rand(cols)
    A[200, :] = 0             # empty row must still be zeroed at beta=0
    A = sparse.csr_matrix(A, dtype=np.float32)
    _check_spmm_queue(gpu, A, k, beta=0, seed=11, rtol=2e-5, atol=2e-5)


def test_spmm_queue_dual_negative_columns(gpu):
    """Queue scheduler through the dual-operand (negative column) path."""
    rng = np.random.default_rng(21)
    rows, n0, n1, k = 200, 300, 64, 32
    nnz_per_row = 6
    indptr = np.arange(0, (rows + 1) * nnz_per_row, nnz_per_row, dtype=np.int64)
    cols = np.empty(rows * nnz_per_row, dtype=np.int32)
    vals = (2 * rng.random(rows * nnz_per_row) - 1).astype(np.float32)
    c0 = rng.integers(0, n0, rows * nnz_per_row)
    c1 = rng.integers(0, n1, rows * nnz_per_row)
    use1 = rng.random(rows * nnz_per_row) < 0.3
    cols[:] = np.where(use1, -(c1 + 1), c0)
    from arrow_matrix_amd import hip
    blk = hip.CsrBlockGPU(arrays=((rows, n0), indptr, cols, vals))
    blk.set_queue(1)
    X0 = (2 * rng.random((n0, k)) - 1).astype(np.float32)
    X1 = (2 * rng.random((n1, k)) - 1).astype(np.float32)
    X0t, X1t = torch.from_numpy(X0).cuda(), torch.from_numpy(X1).cuda()
    Ct = torch.zeros((rows, k), device='cuda')
    blk.spmm_dual(X0t.data_ptr(), X1t.data_ptr(), Ct.data_ptr(), k, 0,
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ref = np.zeros((rows, k), dtype=np.float64)
    for r in range(rows):
        for t in range(indptr[r], indptr[r + 1]):
            c = cols[t]
            xrow = X1[-c - 1] if c < 0 else X0[c]
            ref[r] += float(vals[t]) * xrow
    np.testing.assert_allclose(Ct.cpu().numpy(), ref, rtol=2e-5, atol=2e-5)


def test_spmm_col_items_hub(gpu):
    """Column-ordered work items (arrow_csr_create_opts flags=1): identical
    results on a hub-heavy structure with split rows and empty rows."""
    from arrow_matrix_amd import hip
    rows, cols, k = 300, 4000, 128
    rs = np.random.RandomState(5)
    A = sparse.random(rows, cols, density=0.003, format='lil', random_state=rs,
                      dtype=np.float64)
    A[3, :] = rs.rand(cols)
    A[177, :] = rs.rand(cols)
    A[50, :] = 0
    A = sparse.csr_matrix(A, dtype=np.float32)
    rng = np.random.default_rng(6)
    X = (2 * rng.random((cols, k)) - 1).astype(np.float32)
    Xt = torch.from_numpy(X).cuda()
    for beta in (0, 1):
        C0 = (2 * rng.random((rows, k)) - 1).astype(np.float32)
        Ct = torch.from_numpy(C0.copy()).cuda()
        blk = hip.CsrBlockGPU(A, col_items=True)
        blk.set_queue(1)
        blk.spmm(Xt.data_ptr(), Ct.data_ptr(), k, beta,
                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ref = (A @ X) + (C0 if beta else 0)
        scale = max(1.0, float(np.abs(ref).max()))
        np.testing.assert_allclose(Ct.cpu().numpy(), ref, rtol=2e-5,
                                   atol=2e-5 * scale)


def test_spmm_col_items_row_ids(gpu):
    """col_items composed with explicit row_ids (reordered output rows)."""
    from arrow_matrix_amd import hip
    rng = np.random.default_rng(8)
    n_struct, out_rows, cols, k = 50, 80, 600, 32
    nnz_pr = 5
    indptr = np.arange(0, (n_struct + 1) * nnz_pr, nnz_pr, dtype=np.int64)
    idx = rng.integers(0, cols, n_struct * nnz_pr).astype(np.int32)
    vals = (2 * rng.random(n_struct * nnz_pr) - 1).astype(np.float32)
    row_ids = rng.choice(out_rows, n_struct, replace=False).astype(np.int64)
    blk = hip.CsrBlockGPU(arrays=((n_struct, cols), indptr, idx, vals),
                          row_ids=row_ids, col_items=True)
    blk.set_queue(1)
    X = (2 * rng.random((cols, k)) - 1).astype(np.float32)
    Xt = torch.from_numpy(X).cuda()
    Ct = torch.full((out_rows, k), 7.0, device='cuda')
    blk.spmm(Xt.data_ptr(), Ct.data_ptr(), k, 1,
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ref = np.full((out_rows, k), 7.0, dtype=np.float64)
    for r in range(n_struct):
        for t in range(indptr[r], indptr[r + 1]):
            ref[row_ids[r]] += float(vals[t]) * X[idx[t]]
    np.testing.assert_allclose(Ct.cpu().numpy(), ref, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("k", [4, 8, 16])
def test_spmm_queue_wave_grabs(gpu, k):
    """Per-WAVE queue grabs (spmm_kernel_qw): the default queue scheduler at
    GROUP < 8, which these k reach with no variable set. The forced variants
    (ARROW_QWAVE=1 at GROUP >= 8, the hub case, ARROW_K16_G8) need a process
    of their own — the variables are read once — and live in
    test_gpu_variants.py."""
    A = _random_csr(600, 800, 0.02, seed=300 + k)
    _check_spmm_queue(gpu, A, k, beta=0, seed=40 + k)
    _check_spmm_queue(gpu, A, k, beta=1, seed=41 + k)


def test_spmm_within_segment_col_sort(gpu):
    """Two-level item order (arrow_csr_create_opts flags=2): identical
    results on a hub structure (row segments kept, columns sorted inside)."""
    from arrow_matrix_amd import hip
    rows, cols, k = 300, 4000, 32
    rs = np.random.RandomState(17)
    A = sparse.random(rows, cols, density=0.01, format='lil', random_state=rs,
                      dtype=np.float64)
    A[5, :] = rs.rand(cols)
    A = sparse.csr_matrix(A, dtype=np.float32)
    rng = np.random.default_rng(17)
    X = (2 * rng.random((cols, k)) - 1).astype(np.float32)
    Xt = torch.from_numpy(X).cuda()
    blk = hip.CsrBlockGPU(arrays=((rows, cols), A.indptr.astype(np.int64),
                                  A.indices.astype(np.int32), A.data),
                          col_items=2)
    blk.set_queue(1)
    Ct = torch.zeros((rows, k), device='cuda')
    blk.spmm(Xt.data_ptr(), Ct.data_ptr(), k, 0,
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ref = A @ X
    np.testing.assert_allclose(Ct.cpu().numpy(), ref, rtol=2e-5, atol=2e-5)
