"""Checkpoints of a tree set (mk_tree_set_checkpoint / _rollback / _release,
``TreeSet.checkpoint`` / ``rollback`` / ``release``): a small
set of the three kinds plus ``put``, the host model a list of Python copies.
After every roll back: ``root()`` and every ``tree_root`` equal the values
taken at the checkpoint AND the oracle root of the model, the items are equal,
``audit()`` is clean, ``diff`` against a clone taken at the checkpoint is empty,
branches of a few indices verify, and a further slot applied afterwards matches
the oracle.  (Model, _rand and einval are test_gpu_tree_set.py's.)"""
import numpy as np
import pytest

from prysm_amd import _lib
from prysm_amd.listtree import verify_branches
from tests.test_gpu_tree_set import BYTES, LIST, STRUCT, Model, _rand, einval, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

N = [2048, 300, 1024]  # a list of 8-B items, a struct list of 40-B records, a bytes list of 48-B elements


def make(salt, caps=(4096, 512, 2048)):
    m = Model(104)
    m.add(LIST, 8, 0, caps[0])
    m.add(STRUCT, 40, 40, caps[1])
    m.add(BYTES, 48, 72, caps[2])
    for t, n in enumerate(N):
        m.assign(t, _rand(n, m.trees[t][1], salt + t))
    m.put(32, bytes(range(8)))
    m.check("built")
    return m


class Mark:
    """A checkpoint and what the set was when it was taken."""

    def __init__(self, m):
        self.cp = m.s.checkpoint()
        self.root = m.s.root()
        self.tree_roots = [m.s.tree_root(t) for t in range(len(m.trees))]
        self.rows = [t[2].copy() for t in m.trees]
        self.msg = m.msg.copy()
        self.clone = m.s.clone()


def slot(m, salt, k=(2, 2, 2), app=(1, 1, 0)):  # below every kind's dirty share: all three climb
    """A few changed values and appends in every tree, and another field of the message."""
    rng = np.random.default_rng(salt)
    for t, (kind, L, rows, _) in enumerate(m.trees):
        if k[t] and len(rows):
            idx = np.sort(rng.choice(len(rows), min(k[t], len(rows)), replace=False)).astype(np.uint64)
            m.update(t, idx, _rand(len(idx), L, salt + 10 + t))
        if app[t]:
            m.append(t, _rand(app[t], L, salt + 20 + t))
    m.put(32, bytes((salt + i) % 251 for i in range(8)))


def back(m, mk, what, salt):
    m.s.rollback(mk.cp)
    for t in range(len(m.trees)):
        m.trees[t][2] = mk.rows[t].copy()
    m.msg = mk.msg.copy()
    assert m.s.root() == mk.root == m.want_root(), f"{what}: root()"
    for t, (kind, L, rows, off) in enumerate(m.trees):
        assert m.s.count(t) == len(rows), f"{what}: count of tree {t}"
        assert m.s.tree_root(t) == mk.tree_roots[t] == m.want_tree_root(t), f"{what}: root of tree {t}"
        assert np.array_equal(m.s.items(t), rows), f"{what}: items of tree {t}"
    assert all(r[0] == 0 for r in m.s.audit()), f"{what}: audit {m.s.audit()}"
    d = m.s.diff(mk.clone)
    assert all(d[t][1] == 0 and d[t][2] == d[t][3] for t in range(len(m.trees))), f"{what}: diff {d}"
    assert d["container"][0] == 0, f"{what}: the message differs from the clone's"
    for t, (kind, L, rows, off) in enumerate(m.trees):
        n = len(rows)
        if n == 0:
            continue
        idx = np.unique(np.array([0, n // 2, n - 1], dtype=np.uint64))
        vals, br, cont = m.s.branches(t, idx)
        ok = verify_branches(vals, idx, n, m.s.leaf_len(t), br, m.s.root(), cont, m.s.container_off(t))
        assert ok.all(), f"{what}: branches of tree {t}"
    slot(m, salt)
    m.check(f"{what}: a further slot", items=True)


def test_climb(gpu):  # noqa: F811
    m = make(100)
    assert m.s.journal_bytes() == 0
    mk = Mark(m)
    slot(m, 110)
    m.check("the slot")
    held = m.s.journal_bytes()
    # two work items of depth 7 (2048 x 8 B: 128 chunks) and the old last item, and the two smaller trees:
    # far below one copy of the items alone
    assert 0 < held < 2048 * 8, held
    back(m, mk, "a climb", 120)
    assert m.s.journal_bytes() == 0


def test_two_slots_and_pending_changes_dropped(gpu):  # noqa: F811
    m = make(200)
    mk = Mark(m)
    slot(m, 210)
    m.check("slot 1")
    slot(m, 220)
    m.check("slot 2")
    slot(m, 230)  # never flushed
    back(m, mk, "two records and pending changes", 240)


def test_rebuild_at_the_dirty_share(gpu):  # noqa: F811
    m = make(300)
    mk = Mark(m)
    slot(m, 310, k=(8, 0, 0), app=(0, 0, 0))  # 2048 / 512 = 4 <= 8 dirty: the list tree rebuilds
    m.check("the rebuild")
    assert m.s.journal_bytes() >= 2048 * 8  # a full record of the list tree
    back(m, mk, "a rebuild", 320)


def test_growth_past_the_capacity(gpu):  # noqa: F811
    m = make(400, caps=(2048, 300, 1024))
    mk = Mark(m)
    slot(m, 410, app=(5, 3, 2))
    m.check("the growth")
    caps = [m.s.capacity(t) for t in range(3)]
    assert caps[0] > 2048 and caps[1] > 300 and caps[2] > 1024
    back(m, mk, "a growth", 420)
    assert [m.s.capacity(t) for t in range(3)] >= caps  # capacity is not part of the state


def test_assign_truncate_erase(gpu):  # noqa: F811
    m = make(500)
    mk = Mark(m)
    slot(m, 510)
    m.assign(1, _rand(77, 40, 511))
    m.s.truncate(0, 1000)
    m.trees[0][2] = m.trees[0][2][:1000]
    m.s.erase(2, [3, 150, 4])
    m.trees[2][2] = np.delete(m.trees[2][2], [3, 4, 150], axis=0)
    slot(m, 520)
    m.check("assign, truncate, erase and two slots", items=True)
    back(m, mk, "assign, truncate and erase", 530)


def test_three_nested_rolled_back_to_the_middle(gpu):  # noqa: F811
    m = make(600)
    a = Mark(m)
    slot(m, 610)
    b = Mark(m)
    slot(m, 620)
    m.s.truncate(1, 100)
    m.trees[1][2] = m.trees[1][2][:100]
    c = Mark(m)
    slot(m, 630)
    m.check("three slots")
    back(m, b, "to the middle of three", 640)
    einval(m.s.rollback, c.cp)  # closed with b
    einval(m.s.rollback, b.cp)
    back(m, a, "then to the first", 650)
    assert m.s.journal_bytes() == 0


def test_release_then_rollback(gpu):  # noqa: F811
    m = make(700)
    a = Mark(m)
    slot(m, 710)
    m.check("slot 1")
    b = Mark(m)
    slot(m, 720)
    m.check("slot 2")
    both = m.s.journal_bytes()
    m.s.release(a.cp)
    assert 0 < m.s.journal_bytes() < both
    einval(m.s.rollback, a.cp)
    einval(m.s.release, a.cp)
    back(m, b, "after the release of the oldest", 730)
    c = Mark(m)
    slot(m, 740)
    m.check("slot 3")
    m.s.release(c.cp)
    assert m.s.journal_bytes() == 0
    slot(m, 750)
    m.check("an unjournaled slot", items=True)
    assert m.s.journal_bytes() == 0


def test_journal_reserve_and_errors(gpu):  # noqa: F811
    m = make(800)
    m.s.journal_reserve(1 << 20)
    root = m.s.root()
    cps = [m.s.checkpoint() for _ in range(_lib.MK_CHECKPOINTS_MAX)]
    assert cps == sorted(set(cps))  # ids only grow
    einval(m.s.checkpoint)  # the 65th
    einval(m.s.rollback, cps[-1] + 1)
    einval(m.s.rollback, 0)
    other = make(810)
    einval(m.s.copy_from, other.s)  # into a journaling set
    einval(m.s.add, LIST, 8)
    assert m.s.root() == root
    m.check("after the refusals", items=True)
    other.s.copy_from(m.s)  # out of a journaling set: the state, not the journal
    assert other.s.root() == root and other.s.journal_bytes() == 0
    slot(m, 820)
    m.s.rollback(cps[3])
    assert m.s.root() == root
    einval(m.s.rollback, cps[3])
    einval(m.s.rollback, cps[10])
    m.s.rollback(cps[0])
    assert m.s.root() == root and m.s.journal_bytes() == 0
