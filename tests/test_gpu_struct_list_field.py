"""List fields inside flat records (MK_FIELD_LIST) on the GPU: every item kind
at every count where the chunking or the odd-level rule changes, neighbouring
records of mixed counts, the workgroup sizes' edges, slot garbage, the device
clamp, placements, the host refusals, the resident tree and a tree set.  Every
root is compared with the restatement in tests/struct_list_ref.py or with the
oracle's typed TreeHash (oracle/ssz_ref.py), never with the library itself."""
import random

import numpy as np
import pytest

from oracle import oracle as O
from oracle import ssz_ref
from prysm_amd import _lib
from prysm_amd import state as ST
from tests import struct_list_ref as SL
from tests.test_struct_list_field_host import DEPOSIT_T, SLASHING_T, rand_deposit, rand_vote

pytestmark = pytest.mark.gpu

U8, U16, U64, BOOL, BY = ("uint", 8), ("uint", 16), ("uint", 64), ("bool",), ("bytes",)
ITEMS = {  # name -> (item type, items per chunk)
    "uint64": (U64, 16),
    "bool": (BOOL, 128),
    "bytes32": (("bytearray", 32), 4),
    "bytes48": (("bytearray", 48), 4),
    "struct2": (("struct", "t.Pair", [("B", U16), ("A", U64)]), 4),
    "struct_var": (("struct", "t.Var", [("N", U64), ("D", BY), ("T", U8)]), 4),
}
VAR_CAP = 20  # the slot of struct_var's []byte


def counts_of(ipc):
    return [0, 1, ipc - 1, ipc, ipc + 1, 2 * ipc, 2 * ipc + 1, 5 * ipc, 6 * ipc]


def rand_of(t, rng, count=None):
    k = t[0]
    if k == "bool":
        return rng.getrandbits(1)
    if k == "uint":
        return rng.getrandbits(t[1])
    if k == "bytearray":
        return bytes(rng.getrandbits(8) for _ in range(t[1]))
    if k == "bytes":
        return bytes(rng.getrandbits(8) for _ in range(rng.randint(0, VAR_CAP)))
    if k == "struct":
        return {name: rand_of(ft, rng, count) for name, ft in t[2]}
    if k == "slice":
        return [rand_of(t[1], rng) for _ in range(count)]
    raise ValueError(t)


def n_caps(t):
    """Capacities flatten() needs for one item type: its []byte fields."""
    return [VAR_CAP] * str(t).count("'bytes'")


class Case:
    """Records of a struct {Head uint64; Items []item; Tail uint16}, record i's
    list holding counts[i % len(counts)] items."""

    def __init__(self, name, n, counts, cap, seed=5, where="middle"):
        item, _ = ITEMS[name]
        lst = ("Items", ("slice", item))
        body = {"first": [lst, ("Head", U64), ("Tail", U16)], "middle": [("Head", U64), lst, ("Tail", U16)],
                "last": [("Head", U64), ("Tail", U16), lst]}[where]
        self.t = ("struct", "t.Rec", body)
        self.fields, self.R, pack = SL.flatten(self.t, [cap] + n_caps(item))
        rng = random.Random(seed)
        self.counts = [counts[i % len(counts)] for i in range(n)]
        self.vals = [rand_of(self.t, rng, c) for c in self.counts]
        self.rec = np.frombuffer(b"".join(pack(v) for v in self.vals), dtype=np.uint8).reshape(n, self.R).copy()
        self.roots = SL.record_roots(self.rec, self.fields)


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def dev_roots(gpu, rec, fields):
    """Struct roots on the device entry point; the bytes around the records
    and behind the roots are canaries."""
    import torch

    from prysm_amd import device as D

    n, R = rec.shape
    flat = np.ascontiguousarray(rec).reshape(-1)
    buf = torch.full((16 + flat.size + 64,), 0xA5, dtype=torch.uint8, device=gpu)
    view = buf[4:4 + flat.size]  # a base that is only 4-byte aligned
    view.copy_(torch.from_numpy(flat.copy()).to(gpu))
    out = torch.full((32 * n + 32,), 0x5A, dtype=torch.uint8, device=gpu)
    D.struct_roots(view, n, R, fields, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[32 * n:] == 0x5A).all()
    return got[:32 * n].reshape(n, 32)


@pytest.mark.parametrize("name", list(ITEMS))
def test_item_kinds_and_counts(gpu, name):
    """65 neighbouring records whose counts cycle through every boundary (so
    the lanes of a wave diverge), typed cross-check on a few."""
    ipc = ITEMS[name][1]
    cap = 6 * ipc + 3
    c = Case(name, 65, counts_of(ipc) + [cap], cap)
    assert lib_accepts(c.fields)
    for i in (0, 3, 9, 64):
        assert bytes(c.roots[i]) == ssz_ref.tree_hash(c.t, c.vals[i])
    got = dev_roots(gpu, c.rec, c.fields)
    bad = [(i, c.counts[i]) for i in range(65) if not np.array_equal(got[i], c.roots[i])]
    assert not bad, (name, bad)


def lib_accepts(fields):
    from tests.test_struct_list_field_host import _f

    return _lib.load().mk_ssz_struct_msg_len(_f(fields), len(fields)) > 0


def test_kind_is_accepted(gpu):
    """MK_FIELD_LIST was an unknown kind before this layout existed."""
    assert lib_accepts([(_lib.MK_FIELD_LIST, 0, 4), (_lib.MK_FIELD_RAW, 8, 8)])
    rec = np.zeros((1, 36), dtype=np.uint8)
    rec[0, 0] = 2
    rec[0, 4:20] = np.arange(16)
    want = O.keccak256(O.merkle_hash([bytes(range(8)), bytes(range(8, 16))]))
    assert bytes(ST.struct_roots_packed(rec, [(_lib.MK_FIELD_LIST, 0, 4), (_lib.MK_FIELD_RAW, 8, 8)])[0]) == want


def test_256_chunks(gpu):
    """The largest list the parser takes: 4096 uint64 in 256 chunks, 8 stack levels."""
    cap = 16 * 256
    c = Case("uint64", 5, [cap, 0, cap - 1, cap // 2 + 1, 3 * 16 * 16 + 5], cap)
    assert np.array_equal(dev_roots(gpu, c.rec, c.fields), c.roots)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 257])
def test_record_counts_at_128_threads(gpu, n):
    """Spare lanes and more than one workgroup.  A list of one chunk beside a
    42-byte message needs 300 B of column: the 128-thread instantiation."""
    c = Case("uint64", n, [7, 0, 16, 1, 15], 16, seed=n)
    assert np.array_equal(dev_roots(gpu, c.rec, c.fields), c.roots)


def test_record_counts_at_64_threads(gpu):
    """The vote layout's column takes the 64-thread instantiation: 1, 63, 64, 65 and 257 records."""
    rng = random.Random(21)
    votes = [rand_vote(rng, rng.choice([0, 1, 15, 16, 17, 32, 33, 40])) for _ in range(257)]
    rec, fields = ST.pack_slashable_votes(votes, 40, 8)
    want = SL.record_roots(rec, fields)
    for n in (1, 63, 64, 65, 257):
        assert np.array_equal(dev_roots(gpu, rec[:n], fields), want[:n]), n


def test_slot_garbage_is_ignored(gpu):
    c = Case("bytes32", 65, counts_of(4), 27)
    off = next(o for k, o, _ in c.fields if k == _lib.MK_FIELD_LIST)
    dirty = c.rec.copy()
    for i, cnt in enumerate(c.counts):
        dirty[i, off + 4 + 32 * cnt:off + 4 + 32 * 27] = 0xA5
    assert np.array_equal(dev_roots(gpu, dirty, c.fields), c.roots)


def test_device_clamps_a_count(gpu):
    """count = cap + 7 on the device entry point hashes as cap; the host entry points refuse it."""
    cap = 20
    c = Case("uint64", 3, [cap, 5, cap], cap)
    off = next(o for k, o, _ in c.fields if k == _lib.MK_FIELD_LIST)
    rec = c.rec.copy()
    rec[2, off:off + 4] = np.frombuffer((cap + 7).to_bytes(4, "little"), np.uint8)
    assert np.array_equal(dev_roots(gpu, rec, c.fields), c.roots)
    for fn in (ST.struct_roots_packed, ST.struct_list_root_packed):
        with pytest.raises(_lib.MerkleError) as e:
            fn(rec, c.fields)
        assert e.value.code == _lib.MK_EINVAL
    assert np.array_equal(ST.struct_roots_packed(c.rec, c.fields), c.roots)
    assert ST.struct_list_root_packed(c.rec, c.fields) == SL.list_root(c.rec, c.fields)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_placement(gpu, where):
    c = Case("struct2", 65, counts_of(4), 27, where=where)
    assert np.array_equal(dev_roots(gpu, c.rec, c.fields), c.roots)


def test_two_lists_in_one_record(gpu):
    t = ("struct", "t.Two", [("A", ("slice", U64)), ("M", U16), ("B", ("slice", ("bytearray", 32)))])
    fields, R, pack = SL.flatten(t, [40, 9])
    rng = random.Random(8)
    vals = [{"A": rand_of(("slice", U64), rng, rng.choice([0, 1, 16, 17, 33, 40])), "M": rng.getrandbits(16),
             "B": rand_of(("slice", ("bytearray", 32)), rng, rng.choice([0, 3, 4, 5, 8, 9]))} for _ in range(65)]
    rec = np.frombuffer(b"".join(pack(v) for v in vals), dtype=np.uint8).reshape(65, R)
    want = SL.record_roots(rec, fields)
    assert bytes(want[7]) == ssz_ref.tree_hash(t, vals[7])
    assert np.array_equal(dev_roots(gpu, rec, fields), want)


def test_list_inside_a_nested_struct(gpu):
    """AttesterSlashing: two SlashableVotes by value, each with its index list."""
    rng = random.Random(9)
    cs = [0, 1, 15, 16, 17, 32, 33, 48, 20]
    sl = [{"SlashableVote_1": rand_vote(rng, cs[i % 9]), "SlashableVote_2": rand_vote(rng, cs[(i * 4 + 1) % 9])}
          for i in range(65)]
    rec, fields = ST.pack_attester_slashings(sl, 48, 8)
    want = SL.record_roots(rec, fields)
    for i in (0, 5, 64):
        assert bytes(want[i]) == ssz_ref.tree_hash(SLASHING_T, sl[i])
    assert np.array_equal(dev_roots(gpu, rec, fields), want)
    assert ST.struct_list_root_packed(rec, fields) == ssz_ref.tree_hash(("slice", ("ptr", SLASHING_T)), sl)


def _deposits(n, seed):
    rng = random.Random(seed)
    deps = [rand_deposit(rng, rng.choice([0, 1, 3, 4, 5, 8, 9, 20, 24, 31, 32])) for _ in range(n)]
    rec, fields = ST.pack_deposits(deps, 64)
    return deps, rec, fields


def test_resident_tree_of_deposits(gpu):
    from prysm_amd.listtree import StructListTree, verify_branches

    deps, rec, fields = _deposits(320, 31)
    R = rec.shape[1]
    cur = rec[:300].copy()
    tree = StructListTree(R, fields, capacity=512)
    tree.assign(cur)
    assert len(tree) == 300 and tree.root() == SL.list_root(cur, fields)
    assert tree.root() == ssz_ref.tree_hash(("slice", ("ptr", DEPOSIT_T)), deps[:300])
    # a count above the capacity: refused by assign / update / append, nothing changes
    bad = rec[300:303].copy()
    bad[1, 0:4] = np.frombuffer((33).to_bytes(4, "little"), np.uint8)
    before = tree.root()
    for call in (lambda: tree.update([1, 2, 3], bad), lambda: tree.append(bad), lambda: tree.assign(bad)):
        with pytest.raises(_lib.MerkleError) as e:
            call()
        assert e.value.code == _lib.MK_EINVAL
        assert len(tree) == 300 and tree.root() == before
    idx = [299, 0, 130]
    cur[idx] = rec[300:303]
    tree.update(idx, rec[300:303])
    assert tree.root() == SL.list_root(cur, fields)
    cur = np.concatenate([cur, rec[303:308]])
    tree.append(rec[303:308])
    assert len(tree) == 305 and tree.root() == SL.list_root(cur, fields)
    gone = list(range(1, 305, 3))
    tree.erase(gone)
    cur = np.delete(cur, gone, axis=0)
    assert len(tree) == len(cur) and tree.root() == SL.list_root(cur, fields)
    assert tree.audit()[0] == 0
    twin = tree.clone()
    assert twin.root() == tree.root()
    one = cur[77:78].copy()
    one[0, 4 + 32 * 2 + 5] ^= 0x40  # a byte of branch node 2
    one[0, 0:4] = np.frombuffer((9).to_bytes(4, "little"), np.uint8)
    twin.update([77], one)
    cur2 = cur.copy()
    cur2[77] = one[0]
    assert twin.root() == SL.list_root(cur2, fields) and tree.root() == SL.list_root(cur, fields)
    d, total, na, nb = tree.diff(twin)
    assert list(d) == [77] and total == 1 and na == nb == len(cur)
    pick = [0, 77, len(cur) - 1, 5]
    values, br = tree.branches(pick)
    assert np.array_equal(values, SL.record_roots(cur[pick], fields))
    assert verify_branches(values, pick, len(cur), 32, br, tree.root()).all()


def test_tree_set_with_a_list_layout(gpu):
    from prysm_amd.listtree import TreeSet

    _, rec, fields = _deposits(70, 32)
    bal = np.arange(100, dtype="<u8")
    s = TreeSet(container_len=72)
    a = s.add(_lib.MK_TREE_STRUCT, rec.shape[1], fields=fields, container_off=0)
    b = s.add(_lib.MK_TREE_LIST, 8, container_off=32)
    s.put(64, (7).to_bytes(8, "little"))
    s.assign(a, rec[:64])
    s.assign(b, bal)

    def want(r, v):
        return O.keccak256(SL.list_root(r, fields) + O.merkle_hash([x.tobytes() for x in v]) + (7).to_bytes(8, "little"))
    assert s.root() == want(rec[:64], bal)
    s.append(a, rec[64:70])
    s.update(a, [3], rec[0:1])
    cur = rec[:70].copy()
    cur[3] = rec[0]
    assert s.root() == want(cur, bal)
