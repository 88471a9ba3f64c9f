"""The three resident-tree handles of prysm_amd.listtree (ListTree,
StructListTree, BytesListTree: what a cgo caller holds as mk_list_tree,
mk_struct_list_tree, mk_bytes_list_tree) through one test body, at the sizes
where a handle can go wrong: a list that grows from nothing across every
capacity doubling and the one-chunk boundary (no levels below it), and a list
of 2 * DIV + 1 items, where a small change climbs and a large one rebuilds
(DIV: the kind's MK_*_TREE_REBUILD_DIV).

The host model is a list of row numbers into a pool of rows made once per
kind; the pool's level-0 entries are the CPU oracle's (the items themselves,
O.struct_roots or the reflective oracle's struct hash for a layout with a
variable-length field, O.elem_digests) and the root is O.merkle_hash_flat over
them.  After every step: len, the root, the whole list read back."""
import numpy as np
import pytest

from prysm_amd import _lib

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000000 + 4300
GROWTH = [1, 1, 2, 1, 3, 9, 16, 35]  # n = 1, 2, 4, 5, 8, 17, 33, 68


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


class Kind:
    """One handle kind at one item length: how to make the handle, the pool of
    rows and their level-0 entries (both read-only)."""

    def __init__(self, name, L, div, make, read, pool, pool0, var_off=None, var_cap=0):
        self.name, self.L, self.div, self.make, self.read = name, L, div, make, read
        self.pool = np.ascontiguousarray(pool, dtype=np.uint8).reshape(-1, L)
        self.pool0 = self.pool if pool0 is None else np.ascontiguousarray(pool0, dtype=np.uint8).reshape(-1, 32)
        self.len0 = L if pool0 is None else 32
        self.var_off, self.var_cap = var_off, var_cap  # a variable-length field's slot: offset, capacity
        assert len(self.pool) == len(self.pool0) >= pool_rows(div)
        self.pool.setflags(write=False)
        self.pool0.setflags(write=False)


def pool_rows(div):
    return 4 * div + 120  # phase B: 4 DIV + 13 rows, phase A: 87


def _rand(nbytes, salt):
    from oracle import oracle as O

    return O.splitmix_bytes((nbytes + 7) // 8 * 8, SEED + salt)[:nbytes].copy()


def _list_kind(L):
    from prysm_amd.listtree import ListTree

    div = _lib.LIST_TREE_REBUILD_DIV
    return Kind(f"list-{L}", L, div, lambda cap: ListTree(L, capacity=cap), "items",
                _rand(pool_rows(div) * L, L), None)


def _bytes_kind(L):
    from oracle import oracle as O
    from prysm_amd.listtree import BytesListTree

    div = _lib.BYTES_TREE_REBUILD_DIV
    pool = _rand(pool_rows(div) * L, 1000 + L)
    return Kind(f"bytes-{L}", L, div, lambda cap: BytesListTree(L, capacity=cap), "elems", pool,
                O.elem_digests(pool, pool_rows(div), L))


def _validator_kind():
    from oracle import oracle as O
    from prysm_amd import registry as R
    from prysm_amd.listtree import StructListTree

    div, m = _lib.STRUCT_TREE_REBUILD_DIV, pool_rows(_lib.STRUCT_TREE_REBUILD_DIV)
    pool = R.synthetic_registry(m, SEED + 1).records.view(np.uint8).reshape(m, 160)
    return Kind("struct-validator", 160, div, lambda cap: StructListTree(160, R.VALIDATOR_FIELDS, capacity=cap),
                "records", pool, O.struct_roots(pool, m, 160, R.VALIDATOR_FIELDS))


def _attestation_kind():
    """PendingAttestationRecords with bitfields of 16..47 bytes in 48-byte
    slots, packed by state.pack_attestations; O.struct_roots knows flat layouts
    only, so each record's root is the reflective oracle's."""
    from oracle import ssz_ref as OS
    from prysm_amd import state as ST
    from prysm_amd.listtree import StructListTree
    from tests.ssz_types import to_ref_type

    div, m = _lib.STRUCT_TREE_REBUILD_DIV, pool_rows(_lib.STRUCT_TREE_REBUILD_DIV)
    st = ST.synthetic_state(0, SEED + 2, n_attestations=m, n_batched=0, n_votes=0, lists_len=1, shards=1)
    pool, fields = ST.pack_attestations(st.attestations, 48)
    assert fields == ST.PENDING_ATTESTATION_FIELDS and pool.shape[1] == ST.pending_attestation_record_len(48)
    ref = to_ref_type(ST.PENDING_ATTESTATION_SSZ)
    pool0 = np.stack([np.frombuffer(OS.tree_hash(ref, v), np.uint8) for v in st.as_value()["LatestAttestations"]])
    var = next(f for f in fields if f[0] == _lib.MK_FIELD_VARBYTES)
    return Kind("struct-attestation", pool.shape[1], div,
                lambda cap: StructListTree(pool.shape[1], fields, capacity=cap), "records", pool, pool0,
                var_off=var[1], var_cap=var[2])


KINDS = {
    "list-8": lambda: _list_kind(8), "list-32": lambda: _list_kind(32), "list-200": lambda: _list_kind(200),
    "bytes-32": lambda: _bytes_kind(32), "bytes-5": lambda: _bytes_kind(5),
    "struct-validator": _validator_kind, "struct-attestation": _attestation_kind,
}


class Run:
    """A handle and its model: `cur`, the pool row of every list item."""

    def __init__(self, kind, cap):
        self.k, self.t, self.cur, self.next = kind, kind.make(cap), [], 0

    def take(self, n):
        """The next n unused pool rows."""
        rows = list(range(self.next, self.next + n))
        self.next += n
        assert self.next <= len(self.k.pool)
        return rows

    def check(self, what, sub=None):
        from oracle import oracle as O

        k, n = self.k, len(self.cur)
        cur = np.asarray(self.cur, dtype=np.int64)
        assert len(self.t) == n, what
        assert self.t.root() == O.merkle_hash_flat(k.pool0[cur].reshape(-1), n, k.len0), f"{what}: root"
        read = getattr(self.t, k.read)
        got = read()
        assert got.shape == (n, k.L) and np.array_equal(got, k.pool[cur]), f"{what}: read-back"
        if sub:
            first, cnt = sub
            assert np.array_equal(read(first, cnt), k.pool[cur[first:first + cnt]]), f"{what}: items {sub}"

    def assign(self, n, what):
        rows = self.take(n)
        self.t.assign(self.k.pool[rows])
        self.cur = rows
        self.check(what)

    def append(self, n, what):
        rows = self.take(n)
        self.t.append(self.k.pool[rows])
        self.cur = self.cur + rows
        self.check(what)

    def update(self, idx, what, sub=None):
        rows = self.take(len(idx))
        self.t.update(idx, self.k.pool[rows])
        for i, r in zip(idx, rows):  # in sequence: the last value of a repeated index wins
            self.cur[i] = r
        self.check(what, sub)

    def refused(self, call, what):
        with pytest.raises(_lib.MerkleError) as e:
            call()
        assert e.value.code == _lib.MK_EINVAL, what
        self.check(f"after the refused {what}")


@pytest.mark.parametrize("name", list(KINDS))
def test_handle_sizes(gpu, name):
    k = KINDS[name]()
    # ---- phase A: a tiny list, every step rebuilds --------------------------------------------
    a = Run(k, 0)
    a.check("new")  # the root of the empty list
    for step in GROWTH:
        a.append(step, f"append {step}")
        n = len(a.cur)
        a.update([n - 1], f"update the last of {n}")
    assert len(a.cur) == 68
    a.assign(3, "assign 3 (the count shrinks)")
    a.assign(0, "assign 0")
    # ---- phase B: the climb ---------------------------------------------------------------------
    div = k.div
    b = Run(k, 4 * div)
    b.assign(2 * div + 1, "assign 2 DIV + 1")
    n = len(b.cur)
    b.update([n // 2], "one index (a climb)", sub=(n // 2 - 1, 3))
    b.update([7, 3, n - 1, 3, 0, 7, 3], "unsorted, repeated indices")
    # refusals: nothing changes
    two = k.pool[b.take(2)]
    b.refused(lambda: b.t.update([1, n], two), "update of index n")
    if k.var_off is not None:
        bad = two.copy()
        bad[1, k.var_off:k.var_off + 4] = np.frombuffer((k.var_cap + 1).to_bytes(4, "little"), np.uint8)
        b.refused(lambda: b.t.update([1, 2], bad), "update with an oversized length")
        b.refused(lambda: b.t.append(bad), "append with an oversized length")
        b.refused(lambda: b.t.assign(bad), "assign with an oversized length")
    b.append(1, "append 1 (a climb, within the capacity)")
    b.append(2 * div, "append 2 DIV (past the capacity: grow, move, rebuild)")
    assert len(b.cur) == 4 * div + 2
    b.update([len(b.cur) - 1], "one index on the rebuilt levels")
