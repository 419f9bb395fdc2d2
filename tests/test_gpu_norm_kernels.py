"""The step norms sum (c - d)^2 and sum c^2 on the GPU, fused into the affine
launch (arrow_spmm*_affine_norm*) and stand-alone (arrow_diffnorm_rows_*), in
float32, float64 and bfloat16 features: one child process
(tests/norm_driver.py) per (precision, environment), so that all three
schedulers and both store forms really run. The cases, references and bounds
are tests/spmm_cases_norm.py's.
"""
import os

import pytest
import torch

from tests import gpu_children
from tests import norm_driver as drv
from tests import spmm_cases_norm as sn
from tests.spmm_cases import KERNEL_VARS

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(gpu_children.REPO, 'tests', 'norm_driver.py')
# the affine children's limits: the default set adds the k = 1024 products of
# `zero_rows` on the host, the stand-alone shapes and the misuse calls
LIMIT_S = {'default': 240}


@pytest.mark.parametrize('env', list(sn.ENVS))
@pytest.mark.parametrize('prec', sn.PRECISIONS)
def test_norm_kernels(prec, env):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lines = gpu_children.child_ok(
        (DRIVER, prec, env), [DRIVER, prec, env], sn.ENVS[env], KERNEL_VARS,
        LIMIT_S.get(env, 120), f"{prec} norm kernel child '{env}'",
        drv.job_names(prec, env))
    # every scheduler the environment can select was launched
    scheds = {ln['scheduler'] for ln in lines.values() if 'scheduler' in ln}
    want = {'default': {sn.GRID, sn.QBLOCK, sn.QWAVE},
            'nt0': {sn.GRID, sn.QBLOCK, sn.QWAVE},
            'qwave1': {sn.GRID, sn.QWAVE},
            'qwave0': {sn.GRID, sn.QBLOCK}}[env]
    assert scheds == want
