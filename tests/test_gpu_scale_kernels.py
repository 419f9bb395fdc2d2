"""arrow_csr_sums / arrow_csr_scale on the GPU (ABI 1007): one child process
per precision runs tests/scale_driver.py in the default environment."""
import os

import pytest

from tests import scale_driver
from tests.gpu_children import REPO, child_ok
from tests.spmm_cases import KERNEL_VARS

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(REPO, 'tests', 'scale_driver.py')


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_scale_kernels(prec):
    child_ok((DRIVER, prec), [DRIVER, prec], {}, KERNEL_VARS, 300,
             f"{prec} scale kernel child", scale_driver.job_names(prec))
