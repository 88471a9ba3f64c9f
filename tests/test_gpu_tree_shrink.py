"""Shrinking the resident trees on the device: truncate and
stable erase of ListTree, StructListTree and BytesListTree, and the device
entries mk_dev_ssz_*_tree_erase under a hipGraph and on two streams.

The host model is a Python list of row numbers into a pool of rows made once
per kind (as tests/test_gpu_tree_handles.py): the pool's level-0 entries are
the CPU oracle's (the items themselves, O.struct_roots or the reflective
oracle's struct hash for the nested attestation layout, O.elem_digests) and a
root is O.merkle_hash_flat over the entries of the list after the same
deletion.  Everything is compared bit for bit.

Per kind and value length, at every starting count around the chunk and level
boundaries (and 4 099: more than one workgroup of the compaction, a climb that
merges dirty paths, and -- by the kind's rebuild divisor -- the level rebuild
for a removal near the front), every removal pattern is followed by:
  the root, the count and the whole list read back;
  a one-value update next to the new end, whose climb reads the moved level-0
  entries and the nodes over them as clean siblings;
  an append back past the old count (no stale node to the right of the new
  end leaks), then a second shrink and a second append."""
import numpy as np
import pytest

from prysm_amd import _lib

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000000 + 5100
POOL = 521  # rows per kind (a prime: row (37 i + c) % POOL differs between neighbours)
COUNTS = [1, 2, 4, 5, 8, 9, 16, 17, 33, 257, 1025, 4099]


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def _rand(nbytes, salt):
    from oracle import oracle as O

    return O.splitmix_bytes((nbytes + 7) // 8 * 8, SEED + salt)[:nbytes].copy()


class Kind:
    def __init__(self, name, tree_kind, L, make, read, pool, pool0, fields=None):
        self.name, self.tree_kind, self.L, self.make, self.read, self.fields = name, tree_kind, L, make, read, fields
        self.pool = np.ascontiguousarray(pool, dtype=np.uint8).reshape(POOL, L)
        self.pool0 = self.pool if pool0 is None else np.ascontiguousarray(pool0, dtype=np.uint8).reshape(POOL, 32)
        self.len0 = L if pool0 is None else 32
        self.per = max(128 // self.len0, 1)  # level-0 entries per chunk
        self.pool.setflags(write=False)
        self.pool0.setflags(write=False)

    def root(self, rows):
        from oracle import oracle as O

        rows = np.asarray(rows, dtype=np.int64)
        return O.merkle_hash_flat(self.pool0[rows].reshape(-1), len(rows), self.len0)


def _list_kind(L):
    from prysm_amd.listtree import ListTree

    return Kind(f"list-{L}", _lib.MK_TREE_LIST, L, lambda cap: ListTree(L, capacity=cap), "items",
                _rand(POOL * L, L), None)


def _bytes_kind(L):
    from oracle import oracle as O
    from prysm_amd.listtree import BytesListTree

    pool = _rand(POOL * L, 1000 + L)
    return Kind(f"bytes-{L}", _lib.MK_TREE_BYTES, L, lambda cap: BytesListTree(L, capacity=cap), "elems", pool,
                O.elem_digests(pool, POOL, L))


def _validator_kind():
    from oracle import oracle as O
    from prysm_amd import registry as R
    from prysm_amd.listtree import StructListTree

    pool = R.synthetic_registry(POOL, SEED + 1).records.view(np.uint8).reshape(POOL, 160)
    return Kind("struct-validator", _lib.MK_TREE_STRUCT, 160,
                lambda cap: StructListTree(160, R.VALIDATOR_FIELDS, capacity=cap), "records", pool,
                O.struct_roots(pool, POOL, 160, R.VALIDATOR_FIELDS), fields=R.VALIDATOR_FIELDS)


def _attestation_kind():
    """The nested PendingAttestationRecord layout of state.pending_attestation_fields(48)."""
    from oracle import ssz_ref as OS
    from prysm_amd import state as ST
    from prysm_amd.listtree import StructListTree
    from tests.ssz_types import to_ref_type

    st = ST.synthetic_state(0, SEED + 2, n_attestations=POOL, n_batched=0, n_votes=0, lists_len=1, shards=1)
    pool, fields = ST.pack_attestations(st.attestations, 48)
    assert fields == ST.pending_attestation_fields(48)
    ref = to_ref_type(ST.PENDING_ATTESTATION_SSZ)
    pool0 = np.stack([np.frombuffer(OS.tree_hash(ref, v), np.uint8) for v in st.as_value()["LatestAttestations"]])
    L = pool.shape[1]
    return Kind("struct-attestation", _lib.MK_TREE_STRUCT, L, lambda cap: StructListTree(L, fields, capacity=cap),
                "records", pool, pool0, fields=fields)


KINDS = {
    "list-1": lambda: _list_kind(1), "list-5": lambda: _list_kind(5), "list-8": lambda: _list_kind(8),
    "list-32": lambda: _list_kind(32), "list-33": lambda: _list_kind(33), "list-48": lambda: _list_kind(48),
    "struct-validator": _validator_kind, "struct-attestation": _attestation_kind,
    "bytes-32": lambda: _bytes_kind(32), "bytes-20": lambda: _bytes_kind(20),
}
_made = {}


def kind_of(name):
    if name not in _made:
        _made[name] = KINDS[name]()
    return _made[name]


def rows(n, c=0):
    return [(37 * i + 11 * c) % POOL for i in range(n)]


def patterns(n, per):
    """(name, removed indices or None, truncate length or None) at starting count n."""
    nch = -(-n // per)
    lose = 1 << ((nch - 1).bit_length() - 1) if nch >= 2 else 0  # the largest power of two of chunks below nch
    b = 2 * per * max(1, (n // (2 * per)) // 2)                  # a level-1 (hence a chunk) boundary inside the list
    run = [i for i in range(b - 2, b + 2) if 0 <= i < n]
    other = list(range(0, n, 2))
    return [
        ("the first value", [0], None),
        ("the last value", [n - 1], None),
        ("one in the middle", [n // 2], None),
        ("every other value, unsorted with a repeat", other[::-1] + other[:1], None),
        ("a prefix", list(range(max(1, n // 3))), None),
        ("a run across a chunk and a level-1 boundary", run or [n - 1], None),
        ("a run near the end", [i for i in range(n - 3 * per - 1, n - 2 * per) if 0 <= i < n] or [0], None),
        ("all but one", [i for i in range(n) if i != n // 2], None),
        ("everything", list(range(n)), None),
        ("a truncate that loses levels", None, lose * per if lose else n - 1),
        ("a truncate to one chunk", None, min(per, n - 1)),
        ("a truncate to 0", None, 0),
    ]


class Run:
    def __init__(self, kind):
        self.k, self.t, self.cur = kind, kind.make(0), []

    def check(self, what):
        k, n = self.k, len(self.cur)
        assert len(self.t) == n, f"{what}: count"
        assert self.t.root() == k.root(self.cur), f"{what}: root"
        got = getattr(self.t, k.read)()
        assert got.shape == (n, k.L) and np.array_equal(got, k.pool[np.asarray(self.cur, dtype=np.int64)]), \
            f"{what}: read-back"

    def shrink(self, rm, trunc, what):
        if rm is not None:
            self.t.erase(rm)
            gone = set(rm)
            self.cur = [r for i, r in enumerate(self.cur) if i not in gone]  # the reference's filter loop
        else:
            self.t.truncate(trunc)
            self.cur = self.cur[:trunc]
        self.check(what)


@pytest.mark.parametrize("name", list(KINDS))
def test_shrink_patterns(gpu, name):
    k = kind_of(name)
    r = Run(k)
    r.check("new")
    for n in COUNTS:
        for c, (pat, rm, trunc) in enumerate(patterns(n, k.per)):
            what = f"{name} n={n} {pat}"
            r.t.assign(k.pool[rows(n, c)])
            r.cur = rows(n, c)
            r.shrink(rm, trunc, what)
            m = len(r.cur)
            if m:  # a climb that reads what moved as clean siblings
                i = m - 2 if m >= 2 else 0
                r.t.update([i], k.pool[[(c + 3) % POOL]])
                r.cur[i] = (c + 3) % POOL
                r.check(f"{what}, then update [{i}]")
            grow = [(91 * j + c) % POOL for j in range(n - m + 3)]  # back past the old count
            r.t.append(k.pool[grow])
            r.cur += grow
            r.check(f"{what}, then append {len(grow)}")
            m = len(r.cur)
            if c % 2:
                r.shrink([m // 3, m - 1, 1], None, f"{what}, a second erase")
            else:
                r.shrink(None, m - m // 4 - 1, f"{what}, a second truncate")
            r.t.append(k.pool[grow[:2]])
            r.cur += grow[:2]
            r.check(f"{what}, the second append")


@pytest.mark.parametrize("name", ["list-8", "struct-validator", "bytes-32"])
def test_refused_shrinks_change_nothing(gpu, name):
    k = kind_of(name)
    r = Run(k)
    r.t.assign(k.pool[rows(37)])
    r.cur = rows(37)
    for call, what in ((lambda: r.t.erase([3, 37]), "erase of index count"),
                       (lambda: r.t.erase([1 << 40]), "erase of a huge index"),
                       (lambda: r.t.truncate(38), "truncate beyond the count")):
        with pytest.raises(_lib.MerkleError) as e:
            call()
        assert e.value.code == _lib.MK_EINVAL, what
        r.check(f"after the refused {what}")
    r.t.truncate(37)  # no-ops
    r.t.erase([])
    r.check("after the no-ops")
    r.t.erase([36, 35, 36])  # a suffix by index: nothing moves
    r.cur = r.cur[:35]
    r.check("a suffix by index")


# ---- the device entries: a replayed graph, two streams -------------------------------------------
class DevTree:
    """A tree of `kind` built by the device build entry in torch buffers of the caller."""

    def __init__(self, gpu, kind, n, cap):
        import torch

        from prysm_amd import device as D

        self.k, self.n, self.cap, self.gpu = kind, n, cap, gpu
        self.cur = rows(n)
        L = kind.L
        self.items = torch.zeros(cap * L + 16, dtype=torch.uint8, device=gpu)
        self.items[: n * L] = torch.from_numpy(kind.pool[self.cur].reshape(-1).copy()).to(gpu)
        self.level0 = None if kind.tree_kind == _lib.MK_TREE_LIST else torch.zeros(32 * cap, dtype=torch.uint8, device=gpu)
        self.lv = torch.zeros(max(D.list_tree_levels_bytes(cap, kind.len0), 16), dtype=torch.uint8, device=gpu)
        self.root = torch.zeros(32, dtype=torch.uint8, device=gpu)
        if kind.tree_kind == _lib.MK_TREE_LIST:
            D.list_tree_build(self.items, n, cap, L, self.lv, self.root)
        elif kind.tree_kind == _lib.MK_TREE_STRUCT:
            D.struct_list_tree_build(self.items, n, cap, L, kind.fields, self.level0, self.lv, self.root)
        else:
            D.bytes_list_tree_build(self.items, n, cap, L, self.level0, self.lv, self.root)

    def erase(self, rm, k_rm, n_new, first, ws):
        from prysm_amd import device as D

        D.tree_erase(self.k.tree_kind, self.items, self.n, n_new, self.cap, self.k.L, self.lv, self.root, rm, k_rm,
                     first, level0=self.level0, spec=self.k.fields, ws=ws)

    def check(self, cur, what):
        import torch

        torch.cuda.synchronize()
        k, n = self.k, len(cur)
        assert bytes(self.root.cpu().numpy()) == k.root(cur), f"{what}: root"
        got = self.items[: n * k.L].cpu().numpy().reshape(n, k.L)
        assert np.array_equal(got, k.pool[np.asarray(cur, dtype=np.int64)]), f"{what}: items"
        if self.level0 is not None:
            got0 = self.level0[: 32 * n].cpu().numpy().reshape(n, 32)
            assert np.array_equal(got0, k.pool0[np.asarray(cur, dtype=np.int64)]), f"{what}: level 0 moved with the values"


@pytest.mark.parametrize("name", ["list-8", "struct-attestation", "bytes-20"])
def test_graph_erase(gpu, name):
    """The erase entry captured once and replayed on a rebuilt tree with another removal list of the same
    shape gives that list's root; a captured truncate likewise."""
    import torch

    from prysm_amd import device as D

    k = kind_of(name)
    n, k_rm, first = 1025, 40, 100
    t = DevTree(gpu, k, n, n)
    d_rm = torch.zeros(k_rm, dtype=torch.int64, device=gpu)
    ws = torch.empty(D.tree_erase_workspace_bytes(k.tree_kind, n - k_rm - first, k.L) + 16, dtype=torch.uint8, device=gpu)
    ws = ws[(-ws.data_ptr()) % 16:]
    saved = (t.items.clone(), None if t.level0 is None else t.level0.clone(), t.lv.clone())
    rng = np.random.default_rng(9)
    rm = np.sort(rng.choice(np.arange(first, n), k_rm, replace=False)).astype(np.int64)
    d_rm.copy_(torch.from_numpy(rm))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # compact, copy back, memset, climb: a single linear chain
        t.erase(d_rm, k_rm, n - k_rm, first, ws)
    for rep in range(2):
        rm = np.sort(rng.choice(np.arange(first, n), k_rm, replace=False)).astype(np.int64)
        d_rm.copy_(torch.from_numpy(rm))
        t.items.copy_(saved[0])
        if t.level0 is not None:
            t.level0.copy_(saved[1])
        t.lv.copy_(saved[2])
        g.replay()
        gone = set(rm.tolist())
        t.check([r for i, r in enumerate(rows(n)) if i not in gone], f"{name} replay {rep}")
    # the truncate form, captured
    t.items.copy_(saved[0])
    if t.level0 is not None:
        t.level0.copy_(saved[1])
    t.lv.copy_(saved[2])
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        t.erase(None, 0, 600, 0, ws)
    g2.replay()
    t.check(rows(n)[:600], f"{name} truncate replay")


def test_two_streams(gpu):
    """Two trees shrunk on two streams, a workspace each."""
    import torch

    from prysm_amd import device as D

    names, ns, ks = ["bytes-32", "struct-validator"], [4099, 1025], [700, 3]
    trees = [DevTree(gpu, kind_of(names[i]), ns[i], ns[i]) for i in range(2)]
    rng = np.random.default_rng(21)
    rms = [np.sort(rng.choice(ns[i], ks[i], replace=False)).astype(np.int64) for i in range(2)]
    d_rm = [torch.from_numpy(rms[i]).to(gpu) for i in range(2)]
    wss = [torch.empty(D.tree_erase_workspace_bytes(trees[i].k.tree_kind, ns[i] - ks[i] - int(rms[i][0]), trees[i].k.L),
                       dtype=torch.uint8, device=gpu) for i in range(2)]
    streams = [torch.cuda.Stream(gpu) for _ in range(2)]
    torch.cuda.synchronize()
    for i in range(2):
        with torch.cuda.stream(streams[i]):
            trees[i].erase(d_rm[i], ks[i], ns[i] - ks[i], int(rms[i][0]), wss[i])
    for i in range(2):
        gone = set(rms[i].tolist())
        trees[i].check([r for j, r in enumerate(rows(ns[i])) if j not in gone], f"tree {i}")
