"""Every kernel with its operands across 2**31 elements and 4 GiB: the SpMM
entry points (plain, affine, affine-norm; grid-stride and queued), the five
route kernels and the two contiguous passes, in float32, float64 and bfloat16
features. One child process (tests/far_driver.py) per precision, with the
default kernel variables. The geometry, the cases and the peak-memory figures
are tests/spmm_cases_far.py's (checked on the CPU by test_spmm_cases_far.py);
the references are the compact cases' own, compared bit for bit.

No case is skipped: an allocation that fails prints ok: false. Each child
holds at most two tall buffers at a time; the peak torch reports per case
must stay within the figure derived from the shapes plus 1 GiB (the
structure, the near operands and the slice temporaries).

Wall time of a child, measured once on an MI355X (a shared card; most of it
is the host side: torch start-up, the compact references, and a few hundred
small launches), and its limit, four times that rounded up to 10 s:

    f32   11.7 s (106 cases)  ->  50 s
    f64   19.5 s  (86 cases)  ->  80 s
    bf16   4.5 s  (64 cases)  ->  20 s
"""
import os

import pytest
import torch

from tests import gpu_children
from tests import spmm_cases_far as far
from tests.spmm_cases import KERNEL_VARS

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(gpu_children.REPO, 'tests', 'far_driver.py')
LIMIT_S = {'f32': 50, 'f64': 80, 'bf16': 20}
ALLOWANCE = 1 << 30


@pytest.mark.parametrize('prec', far.PRECISIONS)
def test_far_offsets(prec):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    peaks = far.job_peaks(prec)
    lines = gpu_children.child_ok(
        (DRIVER, prec), [DRIVER, prec], {}, KERNEL_VARS, LIMIT_S[prec],
        f"{prec} far-offset child", peaks)
    over = {c: (lines[c]['peak_bytes'], peaks[c]) for c in peaks
            if lines[c]['peak_bytes'] > peaks[c] + ALLOWANCE}
    assert not over, f"{prec}: peak memory above the derived figure: {over}"
    # both schedulers ran, and the tall buffers really were allocated
    scheds = {ln['plan']['scheduler'] for ln in lines.values() if 'plan' in ln}
    assert len(scheds) >= 2 and far.sc.GRID in scheds
    top = max(lines[c]['peak_bytes'] for c in peaks)
    assert top >= 2 * far.B * far.ITEMSIZE[prec]
