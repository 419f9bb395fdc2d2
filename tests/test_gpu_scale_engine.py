"""operator_sums / scale_operator / normalize_operator on the GPU engines: one
child process per layout runs tests/engine_scale_driver.py on the gpu device,
in float32, float64 and bfloat16 features."""
import os

import pytest

from tests import engine_scale_driver as esd
from tests.gpu_children import ENGINE_VARS, REPO, child_ok

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(REPO, 'tests', 'engine_scale_driver.py')


@pytest.mark.parametrize('mode', sorted(esd.MODES))
def test_scale_engine(mode):
    lines = child_ok((DRIVER, mode), [DRIVER, mode, 'gpu'], esd.MODES[mode][0],
                     ENGINE_VARS, 300, f"scale engine child '{mode}'",
                     esd.PRECISIONS['gpu'])
    assert sorted(lines) == sorted(esd.PRECISIONS['gpu'])
