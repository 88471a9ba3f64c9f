"""Seeded plan of the stateful checkpoint fuzz: lives of one
tree set of the three kinds under ``checkpoint`` / ``rollback`` / ``release``.
A plain module, no device: tests/test_tree_journal_fuzz_host.py checks what the
plan reaches, tests/test_gpu_tree_journal_fuzz.py runs it.

The steps of a tree (which indices change, how far it grows) are
tests/tree_fuzz_plan.py's ``draw_step``; the handle refuses an index beyond
the count, so the kinds that carry such indices are not drawn.  A plan is a
list of ops:

    ("step", tree, idx, n_app, vseed)   update(idx) and append(n_app values), recorded only
    ("flush",)                          root(): everything pending onto the device
    ("assign", tree, n, vseed)  ("truncate", tree, n)  ("erase", tree, idx)  ("put", vseed)
    ("checkpoint",)  ("rollback", j)  ("release", j)     j: the j-th open checkpoint, oldest first

Every plan opens with four directed passages and goes on at random.
``coverage`` walks a plan on its own -- counts, open checkpoints, the records
each has seen -- and says which roll backs it really contains."""
import random

from prysm_amd import _lib
from prysm_amd import state as ST
from tests.tree_fuzz_plan import chunks_of, draw_step, per_of

LIST, STRUCT, BYTES = _lib.MK_TREE_LIST, _lib.MK_TREE_STRUCT, _lib.MK_TREE_BYTES
# kind, value length, record layout, container offset, first count
TREES = [(LIST, 8, None, 0, 600), (STRUCT, 40, ST.CROSSLINK_FIELDS, 40, 150), (BYTES, 48, None, 72, 90)]
CONTAINER_LEN = 112
PUT_OFF, PUT_LEN = 32, 8
SEEDS = [1, 2, 3]
RANDOM_OPS = 70
MAX_OPEN = 5
MAX_N = 1500  # no tree grows beyond this: the oracle stays quick
STEP_KINDS = ["scattered", "dense_run", "level1_pair", "first_last", "nothing", "append_in_chunk", "append_chunk",
              "append_pair", "append_taller", "append_from_0", "append_1_to_2", "update_append"]


def levels(n, per):
    c, d = chunks_of(n, per), 0
    while (1 << d) < c:
        d += 1
    return d


class _Gen:
    def __init__(self, seed):
        self.rng = random.Random(0x5150 * 1000 + seed)
        self.n = [t[4] for t in TREES]
        self.cps = []  # the counts at every open checkpoint
        self.ops = [("assign", t, n, 17 * seed + t) for t, n in enumerate(self.n)] + [("flush",)]
        self.vseed = 1000 * seed

    def v(self):
        self.vseed += 1
        return self.vseed

    def step(self, t, force=None):
        kind, L = TREES[t][0], TREES[t][1]
        per = per_of(kind, L)
        for _ in range(50):
            s = draw_step(self.rng, self.n[t], MAX_N, per, [0], force=force)
            if s.kind in STEP_KINDS and (force is None or s.kind == force):
                break
            force = None
        else:
            raise AssertionError("no step drawn")
        self.ops.append(("step", t, [int(i) for i in s.idx], int(s.n_new - s.n_old), self.v()))
        self.n[t] = int(s.n_new)

    def flush(self):
        self.ops.append(("flush",))

    def checkpoint(self):
        self.ops.append(("checkpoint",))
        self.cps.append(list(self.n))

    def rollback(self, j):
        self.ops.append(("rollback", j))
        self.n = list(self.cps[j])
        del self.cps[j:]

    def release(self, j):
        self.ops.append(("release", j))
        del self.cps[:j + 1]

    def assign(self, t):
        n = self.rng.choice([0, 1, 5, self.rng.randint(2, 400)])
        self.ops.append(("assign", t, n, self.v()))
        self.n[t] = n

    def truncate(self, t):
        n = self.rng.randint(0, self.n[t])
        self.ops.append(("truncate", t, n))
        self.n[t] = n

    def erase(self, t):
        if self.n[t] == 0:
            return
        idx = sorted(self.rng.sample(range(self.n[t]), self.rng.randint(1, min(self.n[t], 9))))
        self.ops.append(("erase", t, idx))
        self.n[t] -= len(idx)

    def directed(self):
        # two records under one checkpoint
        self.checkpoint(), self.step(0, "scattered"), self.flush(), self.step(1, "scattered"), self.flush()
        self.rollback(0)
        # a full record between two journals
        self.checkpoint(), self.step(2, "scattered"), self.flush(), self.assign(2), self.step(0, "update_append")
        self.flush(), self.rollback(0)
        # the tree grows by a level, the roll back returns to the shorter one
        self.checkpoint(), self.step(0, "append_taller"), self.flush(), self.step(0, "scattered"), self.flush()
        self.rollback(0)
        # the oldest released, then back to a later one
        self.checkpoint(), self.step(1, "update_append"), self.flush(), self.checkpoint(), self.step(0, "scattered")
        self.flush(), self.release(0), self.step(2, "update_append"), self.flush(), self.rollback(0)

    def random(self, nops):
        rng = self.rng
        for _ in range(nops):
            t = rng.randrange(len(TREES))
            op = rng.choices(["step", "flush", "checkpoint", "rollback", "release", "assign", "truncate", "erase", "put"],
                             [50, 14, 9, 7, 4, 3, 3, 3, 5])[0]
            if op == "step":
                self.step(t)
            elif op == "flush":
                self.flush()
            elif op == "checkpoint" and len(self.cps) < MAX_OPEN:
                self.checkpoint()
            elif op == "rollback" and self.cps:
                self.rollback(rng.randrange(len(self.cps)))
            elif op == "release" and self.cps:
                self.release(rng.randrange(len(self.cps)))
            elif op == "assign":
                self.assign(t)
            elif op == "truncate":
                self.truncate(t)
            elif op == "erase":
                self.erase(t)
            elif op == "put":
                self.ops.append(("put", self.v()))
        while self.cps:  # every plan ends with nothing open
            if rng.random() < 0.5:
                self.rollback(len(self.cps) - 1)
            else:
                self.release(0)
        self.flush()


def make_plan(seed, random_ops=RANDOM_OPS, directed=True):
    g = _Gen(seed)
    if directed:
        g.directed()
    g.random(random_ops)
    return g.ops


def coverage(ops):
    """What the roll backs of a plan reach, from a walk of its own.  A record is
    counted only where the handle certainly writes one under an open checkpoint:
    a flush with a recorded step pending (a journal), an assign / truncate /
    erase (a full record; the shrinks flush what is pending first)."""
    n = [0] * len(TREES)          # counts, pending included
    flushed = [0] * len(TREES)    # counts on the device
    pending = False
    cps = []                      # open: {"n", "records", "full", "after_release"}
    released = False              # a release left checkpoints open
    out = {"rollbacks": 0, "two_records": 0, "across_full": 0, "shorter": 0, "release_then_rollback": 0, "releases": 0,
           "nested": 0}

    def flush():
        nonlocal pending
        if pending:
            for c in cps:
                c["records"] += 1
        pending = False
        flushed[:] = n

    def full():
        for c in cps:
            c["records"] += 1
            c["full"] = True

    for op in ops:
        if op[0] == "step":
            _, t, idx, n_app, _ = op
            assert all(0 <= i < n[t] for i in idx), op
            n[t] += n_app
            pending = pending or bool(idx) or n_app > 0
        elif op[0] == "flush":
            flush()
        elif op[0] == "assign":
            n[op[1]] = op[2]
            flushed[op[1]] = op[2]
            full()
        elif op[0] == "truncate":
            assert op[2] <= n[op[1]]
            if op[2] != n[op[1]]:
                flush()
                n[op[1]] = flushed[op[1]] = op[2]
                full()
        elif op[0] == "erase":
            assert all(i < n[op[1]] for i in op[2]) and len(set(op[2])) == len(op[2])
            flush()
            n[op[1]] -= len(op[2])
            flushed[op[1]] = n[op[1]]
            full()
        elif op[0] == "checkpoint":
            flush()
            cps.append({"n": list(n), "records": 0, "full": False, "after_release": released})
            out["nested"] = max(out["nested"], len(cps))
        elif op[0] == "rollback":
            c = cps[op[1]]
            out["rollbacks"] += 1
            out["two_records"] += c["records"] >= 2
            out["across_full"] += c["full"] and c["records"] >= 2
            out["shorter"] += any(levels(c["n"][t], per_of(TREES[t][0], TREES[t][1])) <
                                  levels(flushed[t], per_of(TREES[t][0], TREES[t][1])) for t in range(len(TREES)))
            out["release_then_rollback"] += released and c["records"] >= 1
            n[:] = c["n"]
            flushed[:] = n
            pending = False
            del cps[op[1]:]
            released = released and bool(cps)
        elif op[0] == "release":
            del cps[:op[1] + 1]
            out["releases"] += 1
            released = bool(cps)
        else:
            assert op[0] == "put", op
    assert not cps
    return out
