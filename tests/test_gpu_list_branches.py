"""Merkle proofs out of the resident list trees and their batched verifier
(DESIGN.md §5l): the records of ListTree, StructListTree and BytesListTree and
of the device entry mk_dev_ssz_list_tree_branches compared byte for byte -- the
zero fill included -- with the plain-Python rule (tests/list_branch_ref.py)
over the CPU oracle's level-0 entries, and the verdicts of
mk_verify_list_branches / mk_dev_verify_list_branches with the rule's.

Per kind: every count around the chunk, window and level boundaries with the
capacity equal to the count and larger; every index of the short lists, else
the first, the last, the last item of the last full window and 13 random ones.
Then the same after a truncate, a scattered erase (stale nodes lie to the right
of the new end), an append that outgrows the capacity and an update; the four
corruptions; both root strides; an index >= n in the device form; and the two
device entries in one hipGraph replayed while the list changes."""
import numpy as np
import pytest

from prysm_amd import _lib
from tests import list_branch_ref as R

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000000 + 5200
POOL = 521  # rows per kind (a prime: row (37 i + c) % POOL differs between neighbours)


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
    """A pool of rows and their level-0 entries by the CPU oracle; a list is row numbers into it."""

    def __init__(self, name, L, make, pool, pool0):
        self.name, self.L, self.make = name, L, make
        self.pool = np.ascontiguousarray(pool, dtype=np.uint8).reshape(POOL, L)
        self.pool0 = self.pool if pool0 is None else np.ascontiguousarray(pool0, dtype=np.uint8).reshape(POOL, 32)
        self.s = L if pool0 is None else 32  # bytes of a level-0 entry: what a proof proves
        self.p = 128 // self.s
        self.pool.setflags(write=False)
        self.pool0.setflags(write=False)

    def level0(self, rows):
        return self.pool0[np.asarray(rows, dtype=np.int64)].reshape(-1).tobytes()


def _list_kind(L):
    from prysm_amd.listtree import ListTree

    return Kind(f"list-{L}", L, lambda cap: ListTree(L, capacity=cap), _rand(POOL * L, L), None)


def _bytes_kind(L):
    from oracle import oracle as O
    from prysm_amd.listtree import BytesListTree

    pool = _rand(POOL * L, 1000 + L)
    return Kind(f"bytes-{L}", L, lambda cap: BytesListTree(L, capacity=cap), pool, O.elem_digests(pool, POOL, L))


def _validator_kind():
    from oracle import oracle as O
    from prysm_amd import registry as RG
    from prysm_amd.listtree import StructListTree

    pool = RG.synthetic_registry(POOL, SEED + 1).records.view(np.uint8).reshape(POOL, 160)
    return Kind("struct-validator", 160, lambda cap: StructListTree(160, RG.VALIDATOR_FIELDS, capacity=cap), pool,
                O.struct_roots(pool, POOL, 160, RG.VALIDATOR_FIELDS))


KINDS = {
    "list-1": lambda: _list_kind(1), "list-8": lambda: _list_kind(8), "list-32": lambda: _list_kind(32),
    "list-48": lambda: _list_kind(48), "list-100": lambda: _list_kind(100), "list-128": lambda: _list_kind(128),
    "struct-validator": _validator_kind, "bytes-32": lambda: _bytes_kind(32), "bytes-20": lambda: _bytes_kind(20),
}
_made = {}


def kind_of(name):
    if name not in _made:
        _made[name] = KINDS[name]()
    return _made[name]


def rows(n, c=0):
    return [(37 * i + 11 * c) % POOL for i in range(n)]


def counts(p):
    return [1, p, p + 1, 2 * p, 2 * p + 1, 4 * p, 4 * p + 1, 5 * p, 37 * p + 3, 1025 * p + 1]


def picks(n, p, salt=0):
    """Every index of a short list; else first, last, the last item of the last full window, 13 random."""
    if n <= 5 * p:
        return list(range(n))
    rng = np.random.default_rng(n * 7919 + salt)
    last_full = (n // (2 * p)) * 2 * p - 1
    return [0, n - 1, last_full] + [int(x) for x in rng.integers(0, n, 13)]


def expect(K, lst, idx):
    """(level-0 bytes, n, the records of idx by the rule, the list root by the rule)"""
    data, n = K.level0(lst), len(lst)
    lv = R.levels(data, n, K.s)
    recs = b"".join(R.prove(data, n, K.s, i, lv) for i in idx)
    return data, n, recs, R.list_root(data, n, K.s)


def check_tree(K, tree, lst, idx, what):
    """The handle's proofs of idx equal the rule's byte for byte, its values are the level-0
    entries, and the GPU verifier accepts every one against root()."""
    from prysm_amd.listtree import verify_branches

    data, n, recs, root = expect(K, lst, idx)
    assert len(tree) == n and tree.root() == root, what
    values, br = tree.branches(idx)
    assert br.shape == (len(idx), R.stride(n, K.s)), what
    assert br.tobytes() == recs, what
    want_vals = b"".join(data[i * K.s:(i + 1) * K.s] for i in idx)
    assert values.tobytes() == want_vals, what
    ok = verify_branches(values, idx, n, K.s, br, root)
    assert ok.dtype == bool and ok.all(), (what, ok)
    return values, br, root


@pytest.mark.parametrize("name", list(KINDS))
def test_proofs_at_every_boundary(gpu, name):
    K = kind_of(name)
    for n in counts(K.p):
        for cap in (n, n + max(3, n // 3)):
            tree = K.make(cap)
            lst = rows(n, cap)
            tree.assign(K.pool[lst])
            # any order, a repeat
            idx = picks(n, K.p)[::-1] + [n - 1]
            check_tree(K, tree, lst, idx, (name, n, cap))


@pytest.mark.parametrize("name", ["list-8", "list-100", "struct-validator", "bytes-32"])
def test_proofs_after_the_list_changed(gpu, name):
    """Truncate, scattered erase, an append past the capacity and an update: the records are the
    shorter (longer, changed) list's.  After the shrinks stale nodes lie to the right of the new end."""
    K = kind_of(name)
    p = K.p
    n0 = 37 * p + 3
    tree = K.make(n0)
    lst = rows(n0, 3)
    tree.assign(K.pool[lst])
    check_tree(K, tree, lst, picks(n0, p), (name, "assign"))
    n1 = 19 * p + 1
    tree.truncate(n1)
    lst = lst[:n1]
    check_tree(K, tree, lst, picks(n1, p, 1) + list(range(n1 - p - 1, n1)), (name, "truncate"))
    rm = sorted({1, p, 2 * p + 1, 7 * p, 7 * p + 1, 11 * p + 2, n1 - 2} & set(range(n1)))
    tree.erase(rm)
    lst = [r for i, r in enumerate(lst) if i not in set(rm)]
    check_tree(K, tree, lst, picks(len(lst), p, 2) + list(range(len(lst) - p - 1, len(lst))), (name, "erase"))
    more = rows(60 * p + 5, 9)  # outgrows the capacity of n0
    tree.append(K.pool[more])
    lst = lst + more
    assert len(lst) > n0
    check_tree(K, tree, lst, picks(len(lst), p, 3), (name, "append"))
    upd = [0, 2 * p, len(lst) - 1]
    new = [(r + 101) % POOL for r in (lst[i] for i in upd)]
    tree.update(upd, K.pool[new])
    for i, r in zip(upd, new):
        lst[i] = r
    check_tree(K, tree, lst, upd + picks(len(lst), p, 4), (name, "update"))
    tree.truncate(1)  # down to no levels at all
    check_tree(K, tree, lst[:1], [0], (name, "one"))


def test_handle_rejects_a_bad_index_and_takes_none(gpu):
    K = kind_of("list-32")
    tree = K.make(16)
    tree.assign(K.pool[rows(9)])
    with pytest.raises(_lib.MerkleError) as ei:
        tree.branches([0, 9])
    assert ei.value.code == _lib.MK_EINVAL
    values, br = tree.branches([])
    assert values.shape == (0, 32) and br.shape == (0, R.stride(9, 32))
    from prysm_amd.listtree import ListTree

    big = ListTree(160, capacity=4)  # an item above 128 bytes has no proof record
    big.assign(_rand(3 * 160, 77))
    with pytest.raises(_lib.MerkleError) as ei:
        big.branches([0])
    assert ei.value.code == _lib.MK_EINVAL


def corrupt(K, data, n, idx, values, br):
    """The four corruptions (and the two harmless ones) of proofs idx: (values, indices, records, want)
    with want the rule's verdicts against the honest root."""
    s, p = K.s, K.p
    root = R.list_root(data, n, s)
    _, cb, nchunks, total, D = R.shape(n, s)
    stride = R.stride(n, s)
    V, I, B = [], [], []
    for g, i in enumerate(idx):
        val, rec = values[g].tobytes(), br[g].tobytes()
        j = (i // p) // 2 if nchunks >= 2 else 0
        wl = min(total, (2 * j + 2) * cb) - 2 * j * cb if nchunks >= 2 else total
        V.append(val), I.append(i), B.append(rec)                       # honest
        bad = bytearray(val)
        bad[(3 * g) % s] ^= 0x04
        V.append(bytes(bad)), I.append(i), B.append(rec)                # a flipped value bit
        for d in range(1, D):                                           # a flipped bit of every sibling
            r2 = bytearray(rec)
            r2[256 + 32 * (d - 1) + (5 * d) % 32] ^= 0x80
            V.append(val), I.append(i), B.append(bytes(r2))
        V.append(val), I.append((i + p) % n), B.append(rec)             # a wrong index
        V.append(val), I.append(n + g), B.append(rec)                   # an index beyond the list
        r3 = bytearray(rec)                                             # past the window's end: not read
        for b in range(wl, 256):
            r3[b] = 0xA5
        V.append(val), I.append(i), B.append(bytes(r3))
    want = [R.verify(v, i, n, s, b, root) for v, i, b in zip(V, I, B)]
    assert all(len(b) == stride for b in B)
    return V, I, B, want, root


@pytest.mark.parametrize("name", ["list-1", "list-48", "list-100", "struct-validator"])
def test_verifier_rejects_corruptions(gpu, name):
    from prysm_amd.listtree import verify_branches

    K = kind_of(name)
    for n in (2 * K.p + 1, 5 * K.p, 37 * K.p + 3):
        lst = rows(n, 5)
        tree = K.make(n)
        tree.assign(K.pool[lst])
        idx = [0, n // 2, n - 1, (n // (2 * K.p)) * 2 * K.p - 1]
        values, br = tree.branches(idx)
        data = K.level0(lst)
        V, I, B, want, root = corrupt(K, data, n, idx, values, br)
        assert tree.root() == root
        assert want.count(True) >= 2 * len(idx) and want.count(False) >= 2 * len(idx)
        vals = np.frombuffer(b"".join(V), dtype=np.uint8)
        recs = np.frombuffer(b"".join(B), dtype=np.uint8)
        got = verify_branches(vals, I, n, K.s, recs, root)
        assert got.tolist() == want, (name, n)
        # one root per proof: the honest root for the even proofs, another for the odd ones
        other = bytes(32)
        roots = b"".join(root if g % 2 == 0 else other for g in range(len(I)))
        got = verify_branches(vals, I, n, K.s, recs, np.frombuffer(roots, dtype=np.uint8))
        assert got.tolist() == [w and g % 2 == 0 for g, w in enumerate(want)], (name, n)
        # a wrong n: the honest proofs against n + 1 and n - 1 items
        for m in (n + 1, n - 1):
            keep = [g for g, i in enumerate(idx) if i < m]
            hv = np.concatenate([values[g] for g in keep])
            hb = b"".join(br[g].tobytes().ljust(R.stride(m, K.s), b"\0")[:R.stride(m, K.s)] for g in keep)
            sm = R.stride(m, K.s)
            want_m = [R.verify(values[g].tobytes(), idx[g], m, K.s, hb[t * sm:(t + 1) * sm], root)
                      for t, g in enumerate(keep)]
            got = verify_branches(hv, [idx[g] for g in keep], m, K.s, np.frombuffer(hb, dtype=np.uint8), root)
            assert got.tolist() == want_m and not any(want_m), (name, n, m)


def _dev_tree(gpu, K, lst, cap):
    """A list tree built by the device entry over K's level-0 entries: (level0, levels, root) tensors."""
    import torch

    from prysm_amd import device as D

    n = len(lst)
    level0 = torch.zeros(cap * K.s + 16, dtype=torch.uint8, device=gpu)
    level0[:n * K.s] = torch.from_numpy(np.frombuffer(K.level0(lst), dtype=np.uint8).copy()).to(gpu)
    levels = torch.full((max(D.list_tree_levels_bytes(cap, K.s), 16),), 0xEE, dtype=torch.uint8, device=gpu)
    root = torch.zeros(32, dtype=torch.uint8, device=gpu)
    D.list_tree_build(level0, n, cap, K.s, levels, root=root)
    return level0, levels, root


@pytest.mark.parametrize("name", ["list-8", "list-100", "list-128", "bytes-32"])
def test_device_form(gpu, name):
    """mk_dev_ssz_list_tree_branches over level 0 and the levels as the device entries lay them out
    (for a bytes tree: its digests, item_len 32), an index >= n among the indices: a zero record and
    ok == 0; mk_dev_verify_list_branches with one root and with one root per proof."""
    import torch

    from prysm_amd import device as D

    K = kind_of(name)
    for n in (1, K.p + 1, 4 * K.p + 1, 37 * K.p + 3, 1025 * K.p + 1):
        cap = n + 5
        lst = rows(n, 7)
        level0, levels, root = _dev_tree(gpu, K, lst, cap)
        idx = picks(n, K.p, 5) + [n, n + 1, 1 << 40]
        data, _, recs, want_root = expect(K, lst, idx)
        d_idx = torch.tensor(idx, dtype=torch.int64, device=gpu)
        out = torch.full((R.stride(n, K.s) * len(idx),), 0xA5, dtype=torch.uint8, device=gpu)
        assert D.list_tree_branches(level0, n, cap, K.s, levels, d_idx, out=out) is out
        torch.cuda.synchronize()
        assert bytes(root.cpu().numpy()) == want_root
        assert out.cpu().numpy().tobytes() == recs, (name, n)
        assert recs[-3 * R.stride(n, K.s):] == bytes(3 * R.stride(n, K.s))
        vals = b"".join(data[i * K.s:(i + 1) * K.s] if i < n else bytes(K.s) for i in idx)
        d_vals = torch.from_numpy(np.frombuffer(vals, dtype=np.uint8).copy()).to(gpu)
        want = [i < n for i in idx]
        ok = D.verify_list_branches(d_vals, d_idx, len(idx), n, K.s, out, root)
        assert ok.cpu().numpy().tolist() == [int(w) for w in want], (name, n)
        roots = torch.zeros(32 * len(idx), dtype=torch.uint8, device=gpu)
        roots.view(len(idx), 32)[::2] = root
        ok = D.verify_list_branches(d_vals, d_idx, len(idx), n, K.s, out, roots, root_stride=32)
        assert ok.cpu().numpy().tolist() == [int(w and g % 2 == 0) for g, w in enumerate(want)], (name, n)


def test_device_form_in_a_graph(gpu):
    """Both device entries captured into one hipGraph and replayed three times; between replays the
    list changes (updates by mk_dev_ssz_list_tree_update outside the graph, into the same buffers) and
    the indices are rewritten: records and verdicts follow."""
    import torch

    from prysm_amd import device as D

    K = kind_of("list-48")
    s, cap = K.s, 64 * K.p
    n = 37 * K.p + 3
    lst = rows(n, 1)
    level0, levels, root = _dev_tree(gpu, K, lst, cap)
    k = 9
    d_idx = torch.zeros(k, dtype=torch.int64, device=gpu)
    d_vals = torch.zeros(k * s, dtype=torch.uint8, device=gpu)
    out = torch.zeros(R.stride(n, s) * k, dtype=torch.uint8, device=gpu)
    ok = torch.zeros(k, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.list_tree_branches(level0, n, cap, s, levels, d_idx, out=out)
        D.verify_list_branches(d_vals, d_idx, k, n, s, out, root, out=ok)
    for turn in range(3):
        if turn:  # items change in place (n is baked into the graph): the tree is brought up to date outside it
            upd = sorted({turn, 2 * K.p + turn, n - 1 - turn})
            new = [(lst[i] + 50 + turn) % POOL for i in upd]
            vals = torch.from_numpy(K.pool0[new].reshape(-1).copy()).to(gpu)
            D.list_tree_update(level0, n, n, cap, s, levels, root,
                               idx=torch.tensor(upd, dtype=torch.int64, device=gpu), k_idx=len(upd), values=vals)
            for i, r in zip(upd, new):
                lst[i] = r
        idx = picks(n, K.p, 10 + turn)[:k - 1] + [n + turn]
        data, _, recs, want_root = expect(K, lst, idx)
        d_idx.copy_(torch.tensor(idx, dtype=torch.int64))
        hv = b"".join(data[i * s:(i + 1) * s] if i < n else bytes(s) for i in idx)
        hv = bytearray(hv)
        hv[s * 2] ^= 1  # proof 2 carries a wrong value
        d_vals.copy_(torch.from_numpy(np.frombuffer(bytes(hv), dtype=np.uint8).copy()))
        out.fill_(0xA5)
        ok.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        assert bytes(root.cpu().numpy()) == want_root, turn
        assert out.cpu().numpy().tobytes() == recs, turn
        assert ok.cpu().numpy().tolist() == [int(i < n and q != 2) for q, i in enumerate(idx)], turn
