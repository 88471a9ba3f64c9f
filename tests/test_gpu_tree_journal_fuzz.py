"""The checkpoint fuzz plan (tests/tree_journal_fuzz_plan.py) on the device:
every op goes through ``listtree.TreeSet`` and a host model of plain copies;
every flush compares ``root()`` and every ``tree_root`` with the oracle of the
model, every roll back also the counts, the items and ``audit()``, and the
journal is empty whenever no checkpoint is open."""
import numpy as np
import pytest

from prysm_amd import _lib
from prysm_amd.listtree import TreeSet
from tests import tree_journal_fuzz_plan as JP

pytestmark = pytest.mark.gpu

LIST, STRUCT, BYTES = JP.LIST, JP.STRUCT, JP.BYTES


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def _vals(rows, L, vseed):
    return np.random.default_rng(vseed).integers(0, 256, (rows, L), dtype=np.uint8)


def tree_root(kind, L, spec, rows):
    from oracle import oracle as O

    n = len(rows)
    flat = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1)
    if kind == LIST:
        return O.merkle_hash_flat(flat, n, L)
    if n == 0:
        return O.merkle_hash_flat(flat, 0, 32)
    lv0 = O.elem_digests(flat, n, L) if kind == BYTES else O.struct_roots(flat.reshape(n, L), n, L, spec)
    return O.merkle_hash_flat(np.ascontiguousarray(lv0).reshape(-1), n, 32)


class Run:
    def __init__(self):
        self.s = TreeSet(JP.CONTAINER_LEN)
        self.rows = []
        for kind, L, spec, off, _n in JP.TREES:
            self.s.add(kind, L, fields=spec, capacity=64, container_off=off)
            self.rows.append(np.zeros((0, L), np.uint8))
        self.msg = np.zeros(JP.CONTAINER_LEN, np.uint8)
        self.cps = []  # (id, rows, msg)

    def check(self, what, deep=False):
        from oracle import oracle as O

        msg = self.msg.copy()
        for t, (kind, L, spec, off, _n) in enumerate(JP.TREES):
            want = tree_root(kind, L, spec, self.rows[t])
            assert self.s.tree_root(t) == want, f"{what}: root of tree {t} ({len(self.rows[t])} values)"
            msg[off:off + 32] = np.frombuffer(want, np.uint8)
        assert self.s.root() == O.keccak256(bytes(msg)), f"{what}: the container root"
        if deep:
            for t in range(len(JP.TREES)):
                assert self.s.count(t) == len(self.rows[t]), f"{what}: count of tree {t}"
                assert np.array_equal(self.s.items(t), self.rows[t]), f"{what}: items of tree {t}"
            assert all(r[0] == 0 for r in self.s.audit()), f"{what}: audit {self.s.audit()}"
        if not self.cps:
            assert self.s.journal_bytes() == 0, f"{what}: {self.s.journal_bytes()} journal bytes with nothing open"

    def op(self, op, what):
        s, L = self.s, [t[1] for t in JP.TREES]
        if op[0] == "step":
            _, t, idx, n_app, vseed = op
            vals = _vals(len(idx) + n_app, L[t], vseed)
            if idx:
                s.update(t, np.array(idx, dtype=np.uint64), vals[:len(idx)])
                self.rows[t][idx] = vals[:len(idx)]
            if n_app:
                s.append(t, vals[len(idx):])
                self.rows[t] = np.concatenate([self.rows[t], vals[len(idx):]])
        elif op[0] == "flush":
            self.check(what)
        elif op[0] == "assign":
            self.rows[op[1]] = _vals(op[2], L[op[1]], op[3])
            s.assign(op[1], self.rows[op[1]])
        elif op[0] == "truncate":
            s.truncate(op[1], op[2])
            self.rows[op[1]] = self.rows[op[1]][:op[2]]
        elif op[0] == "erase":
            s.erase(op[1], op[2])
            self.rows[op[1]] = np.delete(self.rows[op[1]], op[2], axis=0)
        elif op[0] == "put":
            b = _vals(1, JP.PUT_LEN, op[1])[0]
            s.put(JP.PUT_OFF, bytes(b))
            self.msg[JP.PUT_OFF:JP.PUT_OFF + JP.PUT_LEN] = b
        elif op[0] == "checkpoint":
            self.cps.append((s.checkpoint(), [r.copy() for r in self.rows], self.msg.copy()))
        elif op[0] == "rollback":
            cp, rows, msg = self.cps[op[1]]
            s.rollback(cp)
            self.rows, self.msg = [r.copy() for r in rows], msg.copy()
            del self.cps[op[1]:]
            self.check(what, deep=True)
        elif op[0] == "release":
            s.release(self.cps[op[1]][0])
            del self.cps[:op[1] + 1]
        else:
            raise AssertionError(op)


@pytest.mark.parametrize("seed", JP.SEEDS)
def test_fuzz_checkpoints(gpu, seed):
    run = Run()
    ops = JP.make_plan(seed)
    for i, op in enumerate(ops):
        run.op(op, f"seed {seed}, op {i} {op[0]}")
    run.check(f"seed {seed}: the end", deep=True)
    assert run.s.journal_bytes() == 0


def test_a_ring_of_checkpoints_keeps_the_journal_bounded(gpu):
    """The reorg ring: a checkpoint per slot, the oldest released once eight are open, never empty.  What a
    release frees is used again: after many slots the journal's buffer is no larger than a few rings' worth."""
    run = Run()
    for op in JP.make_plan(1, random_ops=0, directed=False):
        run.op(op, "set-up")
    g = JP._Gen(7)
    g.n = [len(r) for r in run.rows]
    caps = []
    for slot in range(300):
        run.op(("checkpoint",), f"slot {slot}")
        if len(run.cps) > 8:
            run.op(("release", 0), f"slot {slot}")
        g.ops = []
        g.step(slot % 3, "scattered")
        for op in g.ops + [("flush",)]:
            run.op(op, f"slot {slot}")
        caps.append(run.s.journal_capacity())
    live = run.s.journal_bytes()
    assert 0 < live <= caps[-1]
    assert caps[-1] == caps[60], f"the journal's buffer grew from {caps[60]} to {caps[-1]} bytes over 240 slots"
    run.op(("rollback", 3), "the ring: back five slots")
    run.op(("rollback", 0), "the ring: back to its oldest")
