"""The fused affine step C = alpha * (A@X) + gamma * R + beta * C and the tail
kernel C = alpha * C + gamma * R on the GPU, in float32, float64 and bfloat16
features: one child process (tests/affine_driver.py) per (precision,
environment), so that all three schedulers and both store forms really run.
The cases, references and bounds are tests/spmm_cases_affine.py's.
"""
import os

import pytest
import torch

from tests import affine_driver as drv
from tests import gpu_children
from tests import spmm_cases_affine as sa
from tests.spmm_cases import KERNEL_VARS

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(gpu_children.REPO, 'tests', 'affine_driver.py')
# process start + GPU initialisation + a few hundred launches of a 330-row
# matrix; the default set adds the k = 1024 products of `zero_rows` on the
# host and the tail-kernel shapes
LIMIT_S = {'default': 240}


@pytest.mark.parametrize('env', list(sa.ENVS))
@pytest.mark.parametrize('prec', sa.PRECISIONS)
def test_affine_kernels(prec, env):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lines = gpu_children.child_ok(
        (DRIVER, prec, env), [DRIVER, prec, env], sa.ENVS[env], KERNEL_VARS,
        LIMIT_S.get(env, 120), f"{prec} affine kernel child '{env}'",
        drv.job_names(prec, env))
    # every scheduler the environment can select was launched
    scheds = {ln['scheduler'] for ln in lines.values() if 'scheduler' in ln}
    want = {'default': {sa.GRID, sa.QBLOCK, sa.QWAVE},
            'nt0': {sa.GRID, sa.QBLOCK, sa.QWAVE},
            'qwave1': {sa.GRID, sa.QWAVE},
            'qwave0': {sa.GRID, sa.QBLOCK}}[env]
    assert scheds == want
