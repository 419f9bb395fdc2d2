"""The bfloat16-feature test inputs check themselves, and the bf16 launch plan
is the hand-written table — on the CPU, against the built library (the plan
query needs no device)."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import spmm_cases as sc
from tests import spmm_cases_bf16 as s16

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def hip():
    from arrow_matrix_amd import hip
    if not hip.is_built():
        subprocess.run(['make', '-C',
                        os.path.join(REPO, 'arrow_matrix_amd', 'csrc')],
                       check=True, capture_output=True)
    return hip


def test_table_matches_its_rule():
    for k, (vec, group, launches) in s16.PLAN_TABLE.items():
        assert k % 8 == 0 and vec == 8
        assert group == min(64, 1 << (k // 8 - 1).bit_length())
        assert launches == -(-k // (8 * group))


@pytest.mark.parametrize('queue', [-1, 0, 1])
def test_bf16_plan_equals_the_table(hip, queue):
    for k in s16.PLAN_TABLE:
        for nnz in (1000, 1 << 26):
            sched = {0: s16.GRID, 1: s16.default_queued(k),
                     -1: s16.policy(k, nnz)}[queue]
            for dtype in (torch.bfloat16, 'bfloat16'):
                got = hip.spmm_plan(k, nnz, queue, dtype=dtype)
                assert got == s16.plan(k, sched), (k, nnz, queue)


@pytest.mark.parametrize('k', s16.K_BAD)
def test_bf16_plan_refuses_k_not_a_multiple_of_8(hip, k):
    lib = hip._load()
    out = (__import__('ctypes').c_int32 * 7)()
    assert lib.arrow_spmm_plan_bf16(k, 1000, -1, out, 7) < 0
    assert 'k % 8' in lib.arrow_last_error().decode()
    with pytest.raises(hip.ArrowSpmmError, match='k % 8'):
        hip.spmm_plan(k, 1000, -1, dtype=torch.bfloat16)
    # the same k is fine in float32
    assert hip.spmm_plan(k, 1000, -1)['launches'] >= 1


def test_suffix_accepts_exactly_the_two_spellings(hip):
    assert hip._suffix(torch.bfloat16) == hip._suffix('bfloat16') == 'bf16'
    for other in ('bf16', 'BFLOAT16', 'bfloat', np.float16, torch.float16,
                  torch.float32, torch.int16, np.int16):
        with pytest.raises(TypeError, match='float32 or float64'):
            hip._suffix(other)
    assert hip._suffix(np.float32) == 'f32' and hip._suffix(np.float64) == 'f64'


def test_backend_and_baselines_refuse_what_the_issue_refuses():
    from arrow_matrix_amd.backends import make_backend
    with pytest.raises(NotImplementedError, match='cpu'):
        make_backend('cpu', torch.bfloat16)
    with pytest.raises(NotImplementedError):
        make_backend('gpu', np.float16)
    from arrow_matrix_amd.arrow_slim import ArrowSlimMPI
    with pytest.raises(NotImplementedError, match='cpu'):
        ArrowSlimMPI(None, tiles_per_side=2, device='cpu',
                     dtype=torch.bfloat16)
    e = ArrowSlimMPI(None, tiles_per_side=2, device='cpu')
    with pytest.raises(NotImplementedError, match='cpu'):
        e.zero_rhs(8, 8, dtype='bfloat16')

    # world > 1: refused before any device is touched
    from arrow_matrix_amd.comm import Comm

    class TwoRanks(Comm):
        size = 2

    for device in ('gpu', 'cpu'):
        with pytest.raises(NotImplementedError, match='world>1|cpu'):
            ArrowSlimMPI(TwoRanks(), tiles_per_side=2, device=device,
                         dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match='world>1'):
        ArrowSlimMPI(TwoRanks(), tiles_per_side=2, device='gpu',
                     dtype='bfloat16')

    # the baselines stay float32 / float64, on either device
    from scipy import sparse
    from arrow_matrix_amd.matrix_slice import MatrixSlice
    from arrow_matrix_amd.spmm_petsc import SpmmPETSc
    from arrow_matrix_amd.spmm_15d import Spmm15D
    A = sparse.identity(16, dtype=np.float32, format='csr')
    ms = MatrixSlice.initialize(None, A)
    for device in ('gpu', 'cpu'):
        with pytest.raises(NotImplementedError, match='bfloat16'):
            SpmmPETSc(None, ms, device=device, dtype=torch.bfloat16)
        with pytest.raises(NotImplementedError, match='bfloat16'):
            Spmm15D(None, A, 8, device=device, dtype='bfloat16')


def test_abi_version(hip):
    assert hip.abi_version() >= 1004


def test_round_once_oracle_on_ties():
    """bf16 keeps 8 significant bits: in [256, 512) the spacing is 2, so 257
    and 259 are ties. Round-to-nearest-even sends 257 to 256 and 259 to 260;
    torch's cast and the rule written out on the bit pattern agree."""
    x = np.array([257, 259, 258, 261, 263, -257, -259, 0.5, 1.0, 8.0, 384.5,
                  385.0, 387.0, 1027.0, 1030.0, 1034.0], dtype=np.float32)
    want = np.array([256, 260, 258, 260, 264, -256, -260, 0.5, 1.0, 8.0, 384,
                     384, 388, 1024, 1032, 1032], dtype=np.float64)
    got = s16.bf16_bits(x)
    np.testing.assert_array_equal(s16.bf16_to_f64(got), want)
    np.testing.assert_array_equal(got, s16.bf16_bits_by_hand(x))
    np.testing.assert_array_equal(got, s16.bf16_bits(x.astype(np.float64)))
    rng = np.random.default_rng(16)
    r = (rng.integers(-2 ** 19, 2 ** 19, 20000) * 0.5).astype(np.float32)
    np.testing.assert_array_equal(s16.bf16_bits(r), s16.bf16_bits_by_hand(r))
    # float64 values that float32 cannot hold would be rounded twice
    with pytest.raises(AssertionError):
        s16.bf16_bits(np.array([1.0 + 2.0 ** -30]))


def test_exact_class_discriminates_per_segment_rounding():
    """The exact-class reference stays inside fp32's exact range, its long
    rows produce ties and sums past 8 bits, and rounding each 2048-nonzero
    segment to bf16 before adding (what a bf16 atomic does) lands on other
    bits: the case can fail."""
    c = s16.case('std', 8, 1, 0, None)
    m = sc.matrix('std')
    X0, X1, C0 = s16.operands(c)
    _, G = s16.reference(c, X0, X1, C0)
    assert np.abs(G * 2).max() < 2 ** 18
    assert (G * 2 == np.rint(G * 2)).all()
    want = s16.bf16_bits(G)
    lens = np.diff(m['indptr'])
    assert sorted(lens[lens > sc.SEG_NNZ]) == [2049, 4097]
    r = int(np.argmax(lens))
    b, e = m['indptr'][r], m['indptr'][r + 1]
    vals = m['vals'].astype(np.float64)
    acc = C0[r].astype(np.float64)
    for s in range(b, e, sc.SEG_NNZ):
        t = slice(s, min(s + sc.SEG_NNZ, e))
        part = (vals[t, None] * X0[m['cols'][t]].astype(np.float64)).sum(0)
        acc = s16.bf16_to_f64(s16.bf16_bits(acc + part))
    assert (s16.bf16_bits(acc) != want[r]).any()


def test_real_bound_holds_for_an_fp32_chain_rounded_once():
    c = s16.case('real', 24, 1, 0, None, matrix='real', kind='real')
    m = sc.matrix('real')
    X0, X1, C0 = s16.operands(c)
    _, G = s16.reference(c, X0, X1, C0)
    bound = s16.real_bound(c, X0, X1, C0, G)
    out = np.zeros_like(G, dtype=np.float32)
    for r in range(m['rows']):
        acc = np.zeros(24, dtype=np.float32)
        for t in range(m['indptr'][r], m['indptr'][r + 1]):
            acc = (m['vals'][t] * X0[m['cols'][t]] + acc).astype(np.float32)
        out[r] = C0[r] + acc
    got = s16.bf16_to_f64(s16.bf16_bits(out))
    assert (np.abs(got - G) <= bound).all()


def test_env_table_is_well_formed():
    for name, (variables, cases) in s16.env_table().items():
        names = [c['name'] for c in cases]
        assert len(names) == len(set(names)), name
        ks = {c['k'] for c in cases if c['matrix'] == 'std'}
        assert set(s16.K_GPU) <= ks, name
        assert any(c['kind'] == 'real' for c in cases), name
        assert {c['beta'] for c in cases} == {0, 1}, name
    cases = s16.env_table()['default'][1]
    assert {c['matrix'] for c in cases} == {'std', 'std_dual', 'stride',
                                            'zero_rows', 'real'}
    assert any(c.get('row_ids') for c in cases)
    scheds = {c['plan']['scheduler'] for _, cs in s16.env_table().values()
              for c in cs}
    assert scheds == {s16.GRID, s16.QBLOCK, s16.QWAVE}
