"""hip.py's launch path against include/arrow_spmm.h: which symbol each call
reaches and with which positional arguments, recorded by a stand-in for the
library (no GPU, no built library), and, where the library is built, the
declared argtypes against the header's parameter counts."""
import os
import re

import numpy as np
import pytest
import torch

from arrow_matrix_amd import hip
from tests.test_cabi import HEADER, LIB, _declared_symbols

H, X0, X1, C, R, D, ACC, STREAM, K = (7, 0x1000, 0x1800, 0x2000, 0x3000,
                                      0x4000, 0x5000, 0x77, 8)
IDX, IDX2, N = 0x6000, 0x6800, 5


class _RecordingLib:
    """Every attribute is an entry point that records (name, args) and
    succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name == 'arrow_last_error':
            return lambda: b''

        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


@pytest.fixture
def lib(monkeypatch):
    rec = _RecordingLib()
    monkeypatch.setattr(hip, '_lib', rec)
    return rec


# (handle dtype, feat_dtype, suffix of the SpMM family)
PRECISIONS = [(np.float32, None, ''), (np.float64, None, '_f64'),
              (np.float32, 'bfloat16', '_bf16')]

# keywords of spmm / spmm_dual -> (symbol without 'arrow_spmm[_dual]' and
# suffix, the arguments between C and beta), in the order of the header:
# [R], [D, acc], k, [alpha, gamma]
STEPS = [
    (dict(), '', (K,)),
    (dict(alpha=2.0), '_affine', (None, K, 2.0, 0.0)),
    (dict(gamma=0.5, R_ptr=R), '_affine', (R, K, 1.0, 0.5)),
    (dict(alpha=0.85, gamma=0.15, R_ptr=R, norm=(D, ACC)), '_affine_norm',
     (R, D, ACC, K, 0.85, 0.15)),
    (dict(norm=(D, ACC)), '_affine_norm', (None, D, ACC, K, 1.0, 0.0)),
    (dict(norm=(0, ACC)), '_affine_norm', (None, None, ACC, K, 1.0, 0.0)),
]


@pytest.mark.parametrize('dtype,feat_dtype,sfx', PRECISIONS)
@pytest.mark.parametrize('kw,tier,middle', STEPS)
@pytest.mark.parametrize('dual', [False, True])
def test_spmm_symbol_and_arguments(lib, dual, kw, tier, middle, dtype,
                                   feat_dtype, sfx):
    block = object.__new__(hip.CsrBlockGPU)
    block._handle, block.dtype = H, np.dtype(dtype)
    try:
        if dual:
            block.spmm_dual(X0, X1, C, K, 0, STREAM, feat_dtype=feat_dtype,
                            **kw)
            want = ('arrow_spmm_dual' + tier + sfx,
                    (H, X0, X1, C) + middle + (0, STREAM))
        else:
            block.spmm(X0, C, K, 0, STREAM, feat_dtype=feat_dtype, **kw)
            want = ('arrow_spmm' + tier + sfx,
                    (H, X0, C) + middle + (0, STREAM))
    finally:
        block._handle = None    # nothing to destroy
    assert lib.calls == [want]
    # alpha and gamma cross as Python floats, null pointers as None
    assert [type(a) for a in lib.calls[0][1]] == [type(a) for a in want[1]]


def test_spmm_beta_and_default_stream(lib):
    block = object.__new__(hip.CsrBlockGPU)
    block._handle, block.dtype = H, np.dtype(np.float32)
    block.spmm(X0, C, K, 1)
    block.spmm_dual(X0, X1, C, K, 1, alpha=2)
    block._handle = None
    assert lib.calls == [
        ('arrow_spmm', (H, X0, C, K, 1, 0)),
        ('arrow_spmm_dual_affine', (H, X0, X1, C, None, K, 2.0, 0.0, 1, 0))]
    assert type(lib.calls[1][1][6]) is float


@pytest.mark.parametrize('dtype,sfx', [(np.float32, '_f32'),
                                       (np.float64, '_f64'),
                                       (torch.bfloat16, '_bf16')])
def test_route_and_tail_symbols_and_arguments(lib, dtype, sfx):
    hip.gather_rows(X0, C, IDX, N, K, STREAM, dtype=dtype)
    hip.scatter_rows(C, X0, IDX, N, K, STREAM, dtype=dtype)
    hip.scatter_add_rows(C, X0, IDX, N, K, STREAM, dtype=dtype)
    hip.permute_rows(C, X0, IDX, IDX2, N, K, STREAM, dtype=dtype)
    hip.permute_add_rows(C, X0, IDX, IDX2, N, K, STREAM, dtype=dtype)
    hip.axpby_rows(C, R, N, K, 0.85, 0.15, STREAM, dtype=dtype)
    hip.axpby_rows(C, 0, N, K, 2, 0.0, STREAM, dtype=dtype)
    hip.diffnorm_rows(C, D, N, K, ACC, STREAM, dtype=dtype)
    hip.diffnorm_rows(C, 0, N, K, ACC, STREAM, dtype=dtype)
    assert lib.calls == [
        ('arrow_gather_rows' + sfx, (X0, C, IDX, N, K, STREAM)),
        ('arrow_scatter_rows' + sfx, (C, X0, IDX, N, K, STREAM)),
        ('arrow_scatter_add_rows' + sfx, (C, X0, IDX, N, K, STREAM)),
        ('arrow_permute_rows' + sfx, (C, X0, IDX, IDX2, N, K, STREAM)),
        ('arrow_permute_add_rows' + sfx, (C, X0, IDX, IDX2, N, K, STREAM)),
        ('arrow_axpby_rows' + sfx, (C, R, N, K, 0.85, 0.15, STREAM)),
        ('arrow_axpby_rows' + sfx, (C, None, N, K, 2.0, 0.0, STREAM)),
        ('arrow_diffnorm_rows' + sfx, (C, D, N, K, ACC, STREAM)),
        ('arrow_diffnorm_rows' + sfx, (C, None, N, K, ACC, STREAM)),
    ]
    assert type(lib.calls[6][1][4]) is float


def _header_parameter_counts():
    """{function name: parameter count} for every prototype of the header."""
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    counts = {}
    for name in _declared_symbols():
        m = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, src)
        if m is None:
            continue    # named in a comment only
        params = m.group(1).strip()
        counts[name] = 0 if params in ('', 'void') else params.count(',') + 1
    return counts


def test_header_parser_reads_the_known_prototypes():
    counts = _header_parameter_counts()
    assert counts['arrow_abi_version'] == 0
    assert counts['arrow_spmm'] == 6
    assert counts['arrow_csr_create_opts'] == 8
    assert counts['arrow_spmm_dual_affine_norm_bf16'] == 12
    assert len(counts) >= 57    # the prototypes of ABI 1006


@pytest.mark.skipif(not os.path.exists(LIB), reason="libarrowspmm.so not built")
def test_declared_argtypes_match_the_header(monkeypatch):
    monkeypatch.setattr(hip, '_lib', None)
    loaded = hip._load()
    for name, n_params in _header_parameter_counts().items():
        declared = getattr(loaded, name).argtypes
        assert len(declared or ()) == n_params, \
            f"{name}: {n_params} parameters in the header, " \
            f"{len(declared or ())} argtypes declared in hip._load()"
