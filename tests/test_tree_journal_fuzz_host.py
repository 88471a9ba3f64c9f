"""The checkpoint fuzz plan (tests/tree_journal_fuzz_plan.py) on the CPU: for
every committed seed the plan really contains a roll back over at least two
records, one across a full record, one that shortens a tree by a level and a
release followed by a roll back -- by ``coverage``'s own walk of the ops, so a
plan that reaches none of them fails here instead of passing quietly on the
device.  The plan is reproducible, and its steps are tree_fuzz_plan.py's."""
import pytest

from tests import tree_fuzz_plan as TP
from tests import tree_journal_fuzz_plan as JP

NEED = ("two_records", "across_full", "shorter", "release_then_rollback")


@pytest.mark.parametrize("seed", JP.SEEDS)
def test_the_plan_reaches_every_roll_back_shape(seed):
    ops = JP.make_plan(seed)
    cov = JP.coverage(ops)
    for what in NEED:
        assert cov[what] >= 1, f"seed {seed}: no roll back with {what}: {cov}"
    assert cov["rollbacks"] >= 5 and cov["releases"] >= 2 and cov["nested"] >= 2, cov
    kinds = {op[0] for op in ops}
    assert kinds >= {"step", "flush", "assign", "truncate", "erase", "put", "checkpoint", "rollback", "release"}, kinds


@pytest.mark.parametrize("seed", JP.SEEDS)
def test_the_random_part_alone_reaches_roll_backs(seed):
    """Without the directed passages the walk still rolls back over records (the directed ones are not all there is)."""
    cov = JP.coverage(JP.make_plan(seed, random_ops=200, directed=False))
    assert cov["rollbacks"] >= 3 and cov["two_records"] >= 1, cov


def test_a_plan_that_reaches_nothing_is_seen():
    """coverage is not satisfied by construction: a plan without roll backs, and one whose only roll back has
    nothing to undo, report zeros."""
    ops = [("assign", t, tr[4], t) for t, tr in enumerate(JP.TREES)] + [("flush",), ("checkpoint",), ("release", 0)]
    assert all(JP.coverage(ops)[w] == 0 for w in NEED)
    ops = ops[:-1] + [("put", 1), ("flush",), ("rollback", 0)]
    cov = JP.coverage(ops)
    assert cov["rollbacks"] == 1 and all(cov[w] == 0 for w in NEED)


def test_reproducible_and_built_on_the_tree_fuzz_steps():
    assert JP.make_plan(2) == JP.make_plan(2) and JP.make_plan(1) != JP.make_plan(2)
    assert JP.draw_step is TP.draw_step and set(JP.STEP_KINDS) <= set(TP.STEP_KINDS)
