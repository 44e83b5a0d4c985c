"""The slab drivers on the HIP plan issue the same launches, transport operations and stream operations, in the same
order, on the same streams and on the same buffers, as the commit their traces were recorded at
(slab_schedule_trace.py): one rank that is its own neighbour, fp32, the point-to-point and the copy transport.  The
peer-window transport needs a process group and symmetric memory and is not traced; test_gpu_slab_gloo.py covers it."""
import pytest

from slab_schedule_trace import GPU_CASES, assert_same_trace

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(GPU_CASES))
def test_slab_driver_issues_the_recorded_schedule_on_the_gpu(case):
    assert_same_trace(case)
