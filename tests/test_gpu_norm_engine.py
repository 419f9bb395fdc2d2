"""Step norms through the engine on one GPU, in float32, float64 and bfloat16
features, with and without an affine step: the default single-launch layout
measures in its own launch (in-process here), every layout an environment
variable selects (two-launch, L = 2 sequential, full fold, row fold) runs one
stand-alone pass, each in a child process that starts with its environment.
The checks are tests/engine_norm_driver.py's.
"""
import os

import pytest
import torch

from tests import engine_norm_driver as drv
from tests import gpu_children

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(gpu_children.REPO, 'tests', 'engine_norm_driver.py')
CHILD_LIMIT_S = 150      # process start + GPU initialisation + 6 x 2 tiny steps


@pytest.mark.parametrize('affine', [False, True])
@pytest.mark.parametrize('precision', drv.PRECISIONS)
def test_default_layout_measures_in_its_launch(precision, affine):
    """The norm entry point is the one called, with or without an affine
    step, and the stand-alone pass never runs."""
    gpu_children.need_gpu()
    _, _, fused = drv.MODES['default']
    arrow, n_fused, n_alone, _ = drv.run_tracked(precision, affine, **drv.ead.L1)
    assert arrow.engines[0]._A_all is not None
    drv.check_counters(fused, n_fused, n_alone)


@pytest.mark.parametrize('mode', [m for m in drv.MODES if m != 'default'])
def test_environment_selected_layouts(mode):
    gpu_children.need_gpu()
    variables, _, _ = drv.MODES[mode]
    lines = gpu_children.child_ok(
        (DRIVER, mode), [DRIVER, mode], variables, gpu_children.ENGINE_VARS,
        CHILD_LIMIT_S, f"norm engine child '{mode}'",
        [f'{p}_affine{a}' for p in drv.PRECISIONS for a in (0, 1)])
    assert set(lines) == {f'{p}_affine{a}' for p in drv.PRECISIONS
                          for a in (0, 1)}
    for ln in lines.values():
        assert (ln['fused_launches'], ln['stand_alone']) == (0, drv.STEPS)


@pytest.mark.parametrize('precision', drv.PRECISIONS)
def test_iterate_stops_on_a_contraction(precision):
    """Row-scaled matrix at damping 0.5: iterate stops before max_steps with
    rel <= tol, after as many steps as the cpu engine takes (which has no
    bfloat16)."""
    gpu_children.need_gpu()
    steps, rel = drv.run_iterate(precision, 'gpu')
    assert 1 < steps < drv.ITER_MAX
    assert rel <= drv.ITER_TOL[precision]
    if precision != 'bfloat16':
        cpu_steps, cpu_rel = drv.run_iterate(precision, 'cpu')
        assert steps == cpu_steps
        assert rel == pytest.approx(cpu_rel, rel=1e-3)


def test_untracked_engine_refuses_to_report():
    gpu_children.need_gpu()
    arrow, *_ = drv.ead.build(precision='float32', **drv.ead.L1)
    with pytest.raises(RuntimeError, match='track_step_norms'):
        arrow.last_step_norms()
    arrow.track_step_norms()
    acc = arrow.engines[0]._norm_acc
    assert acc.is_cuda and acc.dtype == torch.float64 and acc.numel() == 2
    arrow.track_step_norms(False)
    assert arrow.engines[0]._norm_acc is None
