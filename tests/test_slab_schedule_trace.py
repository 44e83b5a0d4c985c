"""The slab drivers issue the same engine calls and transport operations, in the same order and on the same buffers,
as the commit their traces were recorded at (slab_schedule_trace.py): one rank, oracle-backed engine, no overlap."""
import pytest

from slab_schedule_trace import CPU_CASES, assert_same_trace


@pytest.mark.parametrize("case", list(CPU_CASES))
def test_slab_driver_issues_the_recorded_schedule(case):
    assert_same_trace(case)
