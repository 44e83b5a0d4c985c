"""What ``lt.Simulation`` keeps between two batches, pinned from outside: the ``Plan`` calls it issues for a script of
looks, assignments, in-place edits and changed settings equal the recorded ones line for line, on the caller's dense
tensors and on the engine's resident populations, and the populations equal those of a twin that never carries on
(``stepper_call_trace.py`` says how a trace is taken).  The fixtures were recorded before the steppers shared one
kept-state record (``lettuce_amd/_kept.py``)."""
import pytest

import stepper_call_trace as sct

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(sct.CASES))
def test_the_stepper_issues_the_recorded_plan_calls(name):
    sct.assert_same_trace(name)


def test_masks_edited_while_a_pass_is_pending_restart_the_resident_path_from_flow_f():
    """Replaced masks mean the same on every launch path: the next batch starts from ``flow.f``.  With the populations
    in the engine and the pass pending that is the pass (``resident_store``), a collide pass from what it showed
    (``resident_load``) and k - 1 fused steps -- as the dense path does it (fixture ``masks-dense``, event 11) -- where
    the resident path once carried on with k fused steps.  The populations are the twin's either way."""
    marks = []

    def script(pair):
        pair.trace.note("1 a first batch")
        pair.batch()
        assert pair.sim.flow._pending is not None
        pair.both(sct._edit_mask((12, 1)))
        marks.append(len(pair.trace.lines))
        pair.batch()
        marks.append(len(pair.trace.lines))
        pair.look()                                  # asserts torch.equal with the twin

    lines = sct.run_case("masks-resident", script)
    issued = [line for line in lines[marks[0]:marks[1]] if line.startswith("resident_")]
    print("\n".join(lines))
    assert [line.split()[0] for line in issued] == ["resident_store", "resident_load", "resident_advance"], issued
    assert issued[2].startswith(f"resident_advance {sct.TAU:.6g} {sct.K - 1} "), issued[2]
