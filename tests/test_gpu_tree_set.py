"""mk_tree_set (prysm_amd.listtree.TreeSet): up to 16 resident trees and the
hash message of the struct that holds them behind one host handle.  A plain
Python model keeps every list and the message; every root is held against the
oracle (O.merkle_hash_flat over the items, over O.elem_digests, over
O.struct_roots; O.keccak256 of the message with the roots in place).  The
seeded walk is reseedable: MK_TREE_SET_SEED=<int>."""
import os

import numpy as np
import pytest

from prysm_amd import _lib
from prysm_amd import state as ST
from prysm_amd.listtree import TreeSet

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000000 + 3500
LIST, STRUCT, BYTES = _lib.MK_TREE_LIST, _lib.MK_TREE_STRUCT, _lib.MK_TREE_BYTES
DIV = {LIST: _lib.LIST_TREE_REBUILD_DIV, STRUCT: _lib.STRUCT_TREE_REBUILD_DIV, BYTES: _lib.BYTES_TREE_REBUILD_DIV}
# a record with a VARBYTES slot: le32 length + 12 bytes, then a u64
VAR_FIELDS = [(_lib.MK_FIELD_VARBYTES, 0, 12), (_lib.MK_FIELD_RAW, 16, 8)]
SPEC = {40: ST.CROSSLINK_FIELDS, 72: ST.ETH1_VOTE_FIELDS, 24: VAR_FIELDS}


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def _rand(rows, L, salt):
    from oracle import oracle as O

    a = O.splitmix_bytes((rows * L + 7) // 8 * 8 + 8, SEED + salt)[:rows * L].copy().reshape(rows, L)
    if L == 24:  # VAR_FIELDS: a legal length in the slot
        a[:, 0:4] = 0
        a[:, 0] = a[:, 4] % 13
    return a


def _struct_root(rec, fields):
    """The struct hash of one record by the oracle's Keccak (hash.go:141-159):
    K(field outputs); bytes fields K(le32(len) || bytes), u64 raw, a nested struct its own hash."""
    from oracle import oracle as O

    out, i = [], 0
    while i < len(fields):
        kind, off, ln = fields[i]
        i += 1
        if kind == _lib.MK_FIELD_RAW:
            out.append(bytes(rec[off:off + ln]))
        elif kind == _lib.MK_FIELD_BYTES:
            out.append(O.keccak256(ln.to_bytes(4, "little") + bytes(rec[off:off + ln])))
        elif kind == _lib.MK_FIELD_VARBYTES:
            n = int.from_bytes(bytes(rec[off:off + 4]), "little")
            out.append(O.keccak256(n.to_bytes(4, "little") + bytes(rec[off + 4:off + 4 + n])))
        else:  # MK_FIELD_STRUCT: the next ln entries are its fields
            out.append(_struct_root(rec, fields[i:i + ln]))
            i += ln
    return O.keccak256(b"".join(out))


def oracle_root(kind, L, rows):
    from oracle import oracle as O

    n = len(rows)
    flat = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1)
    if kind == LIST:
        return O.merkle_hash_flat(flat, n, L)
    if n == 0:
        return O.merkle_hash_flat(flat, 0, 32)
    if kind == BYTES:
        lv0 = O.elem_digests(flat, n, L)
    elif L == 40:
        lv0 = O.struct_roots(flat.reshape(n, L), n, L, SPEC[L])
    else:  # nested and variable-length fields
        lv0 = np.stack([np.frombuffer(_struct_root(r, SPEC[L]), np.uint8) for r in flat.reshape(n, L)])
    return O.merkle_hash_flat(np.ascontiguousarray(lv0).reshape(-1), n, 32)


class Model:
    """A TreeSet and what it must hold."""

    def __init__(self, container_len=0):
        self.s = TreeSet(container_len)
        self.msg = np.zeros(container_len, np.uint8)
        self.trees = []  # [kind, L, rows (n, L), container_off]

    def add(self, kind, L, off=None, capacity=0):
        t = self.s.add(kind, L, fields=SPEC[L] if kind == STRUCT else None, capacity=capacity, container_off=off)
        assert t == len(self.trees)
        self.trees.append([kind, L, np.zeros((0, L), np.uint8), off])
        return t

    def assign(self, t, rows):
        self.s.assign(t, rows)
        self.trees[t][2] = rows.copy()

    def update(self, t, idx, rows):
        self.s.update(t, idx, rows)
        for i, r in zip(idx, rows):
            self.trees[t][2][int(i)] = r

    def append(self, t, rows):
        self.s.append(t, rows)
        self.trees[t][2] = np.concatenate([self.trees[t][2], rows])

    def put(self, off, data):
        self.s.put(off, data)
        self.msg[off:off + len(data)] = np.frombuffer(bytes(data), np.uint8)

    def want_tree_root(self, t):
        kind, L, rows, _ = self.trees[t]
        return oracle_root(kind, L, rows)

    def want_root(self):
        from oracle import oracle as O

        msg = self.msg.copy()
        for t, (_, _, _, off) in enumerate(self.trees):
            if off is not None:
                msg[off:off + 32] = np.frombuffer(self.want_tree_root(t), np.uint8)
        return O.keccak256(bytes(msg))

    def check(self, what, items=False):
        assert self.s.root() == self.want_root(), f"{what}: the container root"
        for t, (_, L, rows, _) in enumerate(self.trees):
            assert self.s.count(t) == len(rows), f"{what}: count of tree {t}"
            assert self.s.tree_root(t) == self.want_tree_root(t), f"{what}: root of tree {t}"
            if items:
                assert np.array_equal(self.s.items(t), rows), f"{what}: items of tree {t}"


def einval(fn, *a, **kw):
    with pytest.raises(_lib.MerkleError) as e:
        fn(*a, **kw)
    assert e.value.code == _lib.MK_EINVAL, str(e.value)


def test_empty_set(gpu):
    s = TreeSet(64)
    assert len(s) == 0 and s.count(0) == 0
    einval(s.root)  # no tree takes part in the container
    einval(s.tree_root, 0)
    s0 = TreeSet(0)
    einval(s0.root)


def test_all_trees_empty(gpu):
    m = Model(104)
    for i, (kind, L) in enumerate([(LIST, 8), (STRUCT, 40), (BYTES, 32)]):
        m.add(kind, L, off=4 + 32 * i)
    m.put(0, b"\x07\x00\x00\x09")
    m.check("all empty", items=True)
    empty = oracle_root(LIST, 8, np.zeros((0, 8), np.uint8))  # merkleHash([])
    assert [m.s.tree_root(t) for t in range(3)] == [empty] * 3


def test_assign_then_the_same_root_again(gpu):
    m = Model(72)
    a, b = m.add(LIST, 8, off=0), m.add(BYTES, 33, off=40)
    m.put(32, bytes(range(8)))
    m.assign(a, _rand(100, 8, 1))
    m.assign(b, _rand(37, 33, 2))
    want = m.want_root()
    assert m.s.root() == want
    assert m.s.root() == want  # nothing dirty
    assert m.s.tree_root(a) == m.want_tree_root(a)
    assert m.s.root() == want
    m.check("after assign", items=True)


def test_update_rules(gpu):
    """Repeated indices in descending order (the last value wins), an update
    of a pending append, an index beyond the count, a put into a root range."""
    m = Model(100)
    a, b, c = m.add(LIST, 5, off=0), m.add(STRUCT, 40, off=32), m.add(BYTES, 32, off=64)
    for t, (n, L) in zip((a, b, c), [(60, 5), (30, 40), (20, 32)]):
        m.assign(t, _rand(n, L, 10 + t))
    m.put(96, b"abcd")
    m.check("assigned")
    for t, L in ((a, 5), (b, 40), (c, 32)):
        m.update(t, [9, 7, 9, 7, 3, 9], _rand(6, L, 20 + t))
    m.check("descending repeats", items=True)
    for t, L in ((a, 5), (b, 40), (c, 32)):
        n = m.s.count(t)
        m.append(t, _rand(3, L, 30 + t))
        assert m.s.count(t) == n + 3  # pending appends included
        m.update(t, [n + 1, 2, n + 1], _rand(3, L, 40 + t))  # the pending append, twice
    m.check("update of a pending append", items=True)
    before = m.s.root()
    for t, L in ((a, 5), (b, 40), (c, 32)):
        einval(m.s.update, t, [1, m.s.count(t)], _rand(2, L, 50))  # nothing changes, index 1 included
        einval(m.s.items, t, m.s.count(t), 1)
    for off, n in ((0, 1), (31, 2), (60, 8), (95, 2), (64, 32)):
        einval(m.s.put, off, bytes(n))
    assert m.s.root() == before
    m.check("after the refused calls", items=True)


@pytest.mark.parametrize("kind,L", [(LIST, 8), (STRUCT, 72), (BYTES, 33)])
def test_append_across_the_capacity(gpu, kind, L):
    m = Model(40)
    t = m.add(kind, L, off=8, capacity=64)
    other = m.add(LIST, 8)
    m.assign(t, _rand(63, L, 60))  # capacity - 1
    m.assign(other, _rand(9, 8, 61))
    m.check("capacity - 1")
    m.append(t, _rand(1, L, 62))
    m.check("at the capacity")
    m.append(t, _rand(1, L, 63))
    m.update(t, [0, 64], _rand(2, L, 64))  # a resident item and the pending append with it
    m.check("capacity + 1: grown and rebuilt", items=True)
    m.update(t, [64], _rand(1, L, 65))
    m.append(t, _rand(200, L, 66))  # more than the double
    m.check("grown again", items=True)


@pytest.mark.parametrize("kind,L,n", [(LIST, 8, 2048), (LIST, 32, 1024), (STRUCT, 40, 64), (STRUCT, 40, 320),
                                      (BYTES, 32, 512), (BYTES, 33, 2048)])
def test_dirty_share_at_rebuild_div(gpu, kind, L, n):
    """One dirty item below count / rebuild_div (the climb) and exactly at it (the build)."""
    at = n // DIV[kind]
    assert at >= 2
    m = Model(32)
    t = m.add(kind, L, off=0, capacity=n)
    m.assign(t, _rand(n, L, 70))
    rng = np.random.default_rng(n + L)
    for k in (at - 1, at, at - 1, at + 1):
        idx = np.sort(rng.choice(n, k, replace=False))
        m.update(t, idx[::-1], _rand(k, L, 71 + k))
        m.check(f"{k} dirty of {n}", items=(k == at))


def test_assign_shorter_with_changes_pending(gpu):
    m = Model(64)
    a, b = m.add(BYTES, 32, off=0), m.add(STRUCT, 40, off=32)
    m.assign(a, _rand(50, 32, 80))
    m.assign(b, _rand(50, 40, 81))
    m.check("assigned")
    for t, L in ((a, 32), (b, 40)):
        m.update(t, [49, 3], _rand(2, L, 82))
        m.append(t, _rand(5, L, 83))
    m.assign(a, _rand(7, 32, 84))  # drops a's pending changes; b's stay
    assert m.s.count(a) == 7 and m.s.count(b) == 55
    einval(m.s.update, a, [7], _rand(1, 32, 85))
    m.check("shorter list", items=True)
    m.assign(b, _rand(0, 40, 86))
    m.check("emptied", items=True)


def test_tree_outside_the_container(gpu):
    m = Model(40)
    a, b = m.add(LIST, 8, off=4), m.add(BYTES, 32)  # b: MK_NO_CONTAINER
    m.assign(a, _rand(10, 8, 90))
    m.assign(b, _rand(10, 32, 91))
    m.check("assigned")
    before = m.s.root()
    m.update(b, [3], _rand(1, 32, 92))
    assert m.s.root() == before  # b is no field of the message
    m.check("b changed", items=True)
    only = Model(40)
    t = only.add(LIST, 8)
    only.assign(t, _rand(5, 8, 93))
    einval(only.s.root)  # a container no tree takes part in
    assert only.s.tree_root(t) == only.want_tree_root(t)


def test_sixteen_trees_and_no_more(gpu):
    m = Model(16 * 32 + 8)
    shapes = [(LIST, 8), (STRUCT, 40), (BYTES, 32), (LIST, 5), (BYTES, 33), (STRUCT, 72), (STRUCT, 24), (LIST, 32)]
    for i in range(16):
        kind, L = shapes[i % 8]
        m.add(kind, L, off=8 + 32 * i)
    einval(m.s.add, LIST, 8)  # the 17th
    einval(m.s.add, LIST, 8, container_off=0)
    assert len(m.s) == 16
    m.put(0, b"\x01\x02\x03\x04\x05\x06\x07\x08")
    for i in range(16):
        m.assign(i, _rand(3 + 11 * i, shapes[i % 8][1], 100 + i))
    m.check("sixteen assigned")
    for i in range(16):
        m.update(i, [2, 0], _rand(2, shapes[i % 8][1], 120 + i))
        m.append(i, _rand(1 + i % 3, shapes[i % 8][1], 140 + i))
    m.check("sixteen updated", items=True)


def test_overlapping_roots_refused(gpu):
    s = TreeSet(100)
    s.add(LIST, 8, container_off=32)
    for off in (4, 32, 60):
        einval(s.add, LIST, 8, container_off=off)
    s.add(LIST, 8, container_off=0)
    s.add(LIST, 8, container_off=64)
    assert len(s) == 3


def test_varbytes_length_checked_at_update(gpu):
    m = Model(32)
    t = m.add(STRUCT, 24, off=0)
    m.assign(t, _rand(9, 24, 150))
    m.check("assigned")
    bad = _rand(2, 24, 151)
    bad[1, 0] = 13  # a 13-byte string in a 12-byte slot
    einval(m.s.update, t, [0, 1], bad)
    einval(m.s.append, t, bad)
    einval(m.s.assign, t, bad)
    assert m.s.count(t) == 9
    m.check("after the refused records", items=True)


def test_seeded_walk(gpu):
    seed = int(os.environ.get("MK_TREE_SET_SEED", "1"))
    rng = np.random.default_rng(seed)
    shapes = [(LIST, 8), (LIST, 5), (BYTES, 32), (BYTES, 33), (STRUCT, 40), (STRUCT, 24)]
    m = Model(6 * 32 + 12)
    for i, (kind, L) in enumerate(shapes):
        m.add(kind, L, off=None if i == 3 else 12 + 32 * i, capacity=int(rng.integers(0, 40)))
    salt = [1000]

    def rows(k, L):
        salt[0] += 1
        return _rand(k, L, salt[0])

    nroots = 0
    for step in range(200):
        t = int(rng.integers(0, 6))
        kind, L, cur, _ = m.trees[t]
        op = rng.choice(["update", "update", "append", "append", "assign", "put", "root", "root"])
        what = f"seed {seed}, step {step}: {op} on tree {t}"
        if op == "update" and len(cur):
            k = int(rng.integers(1, 6))
            m.update(t, rng.integers(0, len(cur), k), rows(k, L))
        elif op == "append" and len(cur) < 300:
            m.append(t, rows(int(rng.integers(1, 1 + min(40, 300 - len(cur)))), L))
        elif op == "assign" and rng.integers(0, 3) == 0:
            m.assign(t, rows(int(rng.integers(0, 301)), L))
        elif op == "put":
            off = int(rng.integers(0, 12))
            m.put(off, bytes(rows(1, 12 - off)[0]))
        elif op == "root":
            nroots += 1
            assert m.s.root() == m.want_root(), what
            assert m.s.tree_root(t) == m.want_tree_root(t), what
    assert nroots > 20
    m.check(f"seed {seed}: the end of the walk", items=True)
