"""mk_dev_ssz_trees_journal / mk_dev_ssz_trees_restore (k_trees_journal,
k_trees_restore): journal, then mk_dev_ssz_trees_update, then
restore, for the three kinds.  Every buffer of a tree and the journal -- exactly
mk_ssz_trees_journal_bytes long -- lie in a tests/guarded_arena.py arena, so a
write past the journal or past any tree buffer is caught.  After the restore
every byte the layout contract specifies for n_old values must equal a copy
taken before the journal ran: the values, level 0, the nodes within the old
counts on every old level, the root, and with a container the message and its
root -- the bytes themselves, not only the root.  The update in between is
checked against the oracle, and the same update run again after the restore
must give the same root.  (device_levels / split_levels are
test_gpu_list_tree.py's.)"""
import numpy as np
import pytest

from prysm_amd import _lib
from prysm_amd import registry as R
from prysm_amd import state as ST

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000000 + 5150
LIST, STRUCT, BYTES = _lib.MK_TREE_LIST, _lib.MK_TREE_STRUCT, _lib.MK_TREE_BYTES
SPECS = {160: R.VALIDATOR_FIELDS, 40: ST.CROSSLINK_FIELDS}


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def _rand(nbytes, salt):
    from oracle import oracle as O

    return O.splitmix_bytes((nbytes + 7) // 8 * 8, SEED + salt)[:nbytes].copy()


def _per(kind, L):
    leaf = L if kind == LIST else 32
    return 128 // leaf if leaf < 128 else 1


def oracle_root(kind, L, rows):
    from oracle import oracle as O

    n = len(rows)
    flat = np.ascontiguousarray(rows).reshape(-1)
    if kind == LIST:
        return O.merkle_hash_flat(flat, n, L)
    if kind == BYTES:
        lv0 = O.elem_digests(flat, n, L) if n else np.zeros((0, 32), np.uint8)
    else:
        lv0 = O.struct_roots(np.ascontiguousarray(rows), n, L, SPECS[L]) if n else np.zeros((0, 32), np.uint8)
    return O.merkle_hash_flat(np.ascontiguousarray(lv0).reshape(-1), n, 32)


class Tree:
    """A device tree of ``rows`` built by its kind's own build entry, every buffer in a guarded arena."""

    def __init__(self, gpu, kind, L, shift, rows, cap):
        import torch

        from prysm_amd import device as D
        from tests.guarded_arena import GuardedArena

        self.kind, self.L, self.cap, self.n, self.gpu = kind, L, cap, len(rows), gpu
        self.len0 = L if kind == LIST else 32
        self.spec = SPECS[L] if kind == STRUCT else None
        regs = [("items", max(cap * L, 8), 16, shift), ("levels", max(D.list_tree_levels_bytes(cap, self.len0), 32), 16, 0),
                ("root", 32, 16, 0)]
        if kind != LIST:
            regs.append(("level0", max(32 * cap, 32), 16, 0))
        self.arena = GuardedArena(gpu, regs)
        self.items, self.lv, self.root = self.arena.view("items"), self.arena.view("levels"), self.arena.view("root")
        self.level0 = self.arena.view("level0") if kind != LIST else None
        self.rows = np.ascontiguousarray(rows).copy()
        if self.n:
            self.items[:self.n * L].copy_(torch.from_numpy(self.rows.reshape(-1)))
        if kind == LIST:
            D.list_tree_build(self.items, self.n, cap, L, self.lv, self.root)
        elif kind == STRUCT:
            D.struct_list_tree_build(self.items, self.n, cap, L, self.spec, self.level0, self.lv, self.root)
        else:
            D.bytes_list_tree_build(self.items, self.n, cap, L, self.level0, self.lv, self.root)
        torch.cuda.synchronize()

    def args(self, idx=(), vals=None, n_app=0, off=None, lists=True):
        """The mk_tree_update of a change: ``idx`` listed indices, ``n_app`` appended values, ``vals`` the new
        values of both.  lists False: as the restore may get it, without the index list and the values."""
        import torch

        from prysm_amd import device as D

        k = len(idx)
        d_idx = torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(self.gpu) if k and lists else None
        d_vals = torch.from_numpy(np.ascontiguousarray(vals).reshape(-1)).to(self.gpu) if lists and k + n_app else None
        return D.TreeArgs(self.kind, self.items, self.n, self.n + n_app, self.cap, self.L, self.lv, self.root,
                          level0=self.level0, idx=d_idx, k_idx=k, values=d_vals, spec=self.spec, container_off=off)

    def after(self, idx, vals, n_app):
        """The rows after the change (an index >= n is ignored)."""
        rows = self.rows.copy()
        for j, i in enumerate(idx):
            if i < self.n:
                rows[i] = vals[j]
        return np.concatenate([rows, vals[len(idx):len(idx) + n_app]]) if n_app else rows

    def snap(self):
        """Every byte the layout contract specifies for the n values, as host copies."""
        from tests.test_gpu_list_tree import split_levels

        n = self.n
        out = {"items": self.items[:n * self.L].cpu().numpy().copy(), "root": self.root.cpu().numpy().copy()}
        if self.level0 is not None:
            out["level0"] = self.level0[:32 * n].cpu().numpy().copy()
        for d, lv in enumerate(split_levels(self.lv.cpu().numpy(), n, self.cap, self.len0), 1):
            out[f"level {d}"] = lv.copy()
        return out


def assert_same(got, want, what):
    assert got.keys() == want.keys(), f"{what}: {sorted(got)} against {sorted(want)}"
    for name in want:
        bad = np.flatnonzero(got[name].reshape(-1) != want[name].reshape(-1))
        assert bad.size == 0, f"{what}: {name} differs at byte {bad[:4]} of {want[name].size} ({bad.size} bytes)"


def journal_arena(gpu, nbytes):
    from tests.guarded_arena import GuardedArena

    a = GuardedArena(gpu, [("journal", nbytes, 16, 0)])
    a.poison("journal", 0x3C)
    return a


def changes(kind, L, n_old, salt):
    """The issue's change sets that this n_old admits: (name, idx, n_app)."""
    p = _per(kind, L)
    nch = -(-n_old // p)
    full = 1
    while full < max(nch, 1):
        full *= 2
    grow = full * p - n_old + 1 if nch > 1 else p - n_old + 1  # one value into the first chunk of a new level
    out = [("k_idx = 0, nothing appended", [], 0), ("an index >= n_old", [n_old // 2, n_old, n_old + 5][0 if n_old else 1:], 0)]
    if n_old == 0:
        out.append(("an append from n_old = 0", [], p + 1))
    if n_old >= 1:
        out += [("one index", [n_old // 2], 0), ("the last item and an append", [n_old - 1], 1),
                ("an append that adds a level", [], grow)]
    if n_old >= 2:
        out += [("two adjacent indices", [0, 1] if n_old < 4 * p else [2 * p, 2 * p + 1], 0),
                ("first and last", [0, n_old - 1], 0)]
    return out


def cycle(gpu, t, idx, n_app, salt, what):
    """journal, update, restore of one change of tree ``t``; the tree is afterwards what it was before."""
    import torch

    from prysm_amd import device as D

    vals = _rand((len(idx) + n_app) * t.L, salt).reshape(-1, t.L)
    before = t.snap()
    a = t.args(idx, vals, n_app)
    nbytes = D.trees_journal_bytes([a])
    assert nbytes >= 32 and nbytes % 16 == 0, f"{what}: journal of {nbytes} bytes"
    jr = journal_arena(gpu, nbytes)
    D.trees_journal([a], jr.view("journal"))
    D.trees_update([a])
    torch.cuda.synchronize()
    want_root = oracle_root(t.kind, t.L, t.after(idx, vals, n_app))
    assert bytes(t.root.cpu().numpy()) == want_root, f"{what}: the update between journal and restore"
    D.trees_restore([t.args(idx, None, n_app, lists=False)], jr.view("journal"))
    torch.cuda.synchronize()
    jr.check_guards(f"{what}: ")
    t.arena.check_guards(f"{what}: ")
    assert_same(t.snap(), before, f"{what}: after the restore")
    # the restored tree takes the same update again
    D.trees_update([a])
    torch.cuda.synchronize()
    assert bytes(t.root.cpu().numpy()) == want_root, f"{what}: the same update after the restore"
    D.trees_restore([a], jr.view("journal"))
    torch.cuda.synchronize()
    assert_same(t.snap(), before, f"{what}: after the second restore")


KINDS = [(LIST, 8, 8), (LIST, 32, 0), (LIST, 48, 0), (LIST, 160, 4), (BYTES, 32, 0), (BYTES, 48, 1), (STRUCT, 160, 0),
         (STRUCT, 40, 4)]


@pytest.mark.parametrize("kind,L,shift", KINDS, ids=[f"{'?LSB'[k]}{L}" for k, L, _ in KINDS])
def test_journal_update_restore(gpu, kind, L, shift):
    p = _per(kind, L)
    ran = 0
    for n_old in (0, 1, p, p + 1, 8 * p, 8 * p + 1, 1000):
        sets = changes(kind, L, n_old, 0)
        cap = n_old + max(n_app for _, _, n_app in sets) + 3
        t = Tree(gpu, kind, L, shift, _rand(n_old * L, 7 * n_old + L).reshape(n_old, L), cap)
        assert bytes(t.root.cpu().numpy()) == oracle_root(kind, L, t.rows)
        for s, (name, idx, n_app) in enumerate(sets):
            cycle(gpu, t, idx, n_app, 1000 * n_old + 10 * s + L, f"kind {kind}, {L} B, n_old {n_old}, {name}")
            ran += 1
    # 3 change sets for n_old 0, 5 for n_old 1 (when one value is less than two: p > 1 makes n_old = p >= 2), 7 beyond
    assert ran == 3 + 5 + 7 * 5 - (2 if p == 1 else 0), ran


def _three(gpu):
    """A list, a bytes list and a struct list under one container, and one change to each."""
    shapes = [(LIST, 8, 8, 1000, 1030), (BYTES, 48, 1, 37, 64), (STRUCT, 40, 4, 1024, 1024)]
    trees = [Tree(gpu, k, L, sh, _rand(n * L, 900 + i).reshape(n, L), cap) for i, (k, L, sh, n, cap) in enumerate(shapes)]
    return trees, [8, 40, 72]


def _container(gpu, msg):
    import torch

    from tests.guarded_arena import GuardedArena

    a = GuardedArena(gpu, [("msg", len(msg), 4, 0), ("croot", 32, 4, 0)])
    a.view("msg").copy_(torch.from_numpy(msg))
    a.view("croot").zero_()
    return a


def test_three_trees_and_the_container(gpu):
    import torch

    from oracle import oracle as O
    from prysm_amd import device as D

    trees, offs = _three(gpu)
    msg = _rand(107, 950)  # not a multiple of 4: the last piece of the message goes in bytes
    c = _container(gpu, msg)
    cm, cr = c.view("msg"), c.view("croot")
    none = [t.args(off=o) for t, o in zip(trees, offs)]
    D.trees_update(none, cm, 107, cr)  # the roots into the message, the container root
    torch.cuda.synchronize()
    before = [t.snap() for t in trees]
    msg0, root0 = cm.cpu().numpy().copy(), cr.cpu().numpy().copy()
    assert bytes(root0) == O.keccak256(bytes(msg0))
    sets = [([5, 999], 7), ([36], 2), ([0, 1023], 0)]
    vals = [_rand((len(i) + a) * t.L, 960 + j).reshape(-1, t.L) for j, (t, (i, a)) in enumerate(zip(trees, sets))]
    args = [t.args(i, v, a, off=o) for t, (i, a), v, o in zip(trees, sets, vals, offs)]
    nbytes = D.trees_journal_bytes(args, 107)
    assert nbytes == sum(D.trees_journal_bytes([a]) for a in args) + 112 + 32
    jr = journal_arena(gpu, nbytes)
    D.trees_journal(args, jr.view("journal"), cm, 107, cr)
    cm[100:107].copy_(torch.from_numpy(_rand(7, 970)))  # another field of the struct changes with the slot
    D.trees_update(args, cm, 107, cr)
    torch.cuda.synchronize()
    want = cm.cpu().numpy().copy()
    for t, (i, a), v, o in zip(trees, sets, vals, offs):
        r = oracle_root(t.kind, t.L, t.after(i, v, a))
        assert bytes(t.root.cpu().numpy()) == r
        assert bytes(want[o:o + 32]) == r
    assert bytes(cr.cpu().numpy()) == O.keccak256(bytes(want)) != bytes(root0)
    D.trees_restore([t.args(i, None, a, off=o, lists=False) for t, (i, a), o in zip(trees, sets, offs)],
                    jr.view("journal"), cm, 107, cr)
    torch.cuda.synchronize()
    for a in [jr, c] + [t.arena for t in trees]:
        a.check_guards("three trees: ")
    for j, t in enumerate(trees):
        assert_same(t.snap(), before[j], f"tree {j} after the restore")
    assert np.array_equal(cm.cpu().numpy(), msg0), "the container message"
    assert np.array_equal(cr.cpu().numpy(), root0), "the container root"


def test_two_records_newest_first(gpu):
    """The second update overwrites nodes the first one wrote (index 17 and 18 share every ancestor; the
    append of the second grows the tree over the first one's right edge): undone newest first, the tree is
    what it was; after the first restore alone it is what the first update left."""
    import torch

    from prysm_amd import device as D

    for kind, L, shift in ((LIST, 8, 8), (STRUCT, 160, 0), (BYTES, 48, 1)):
        p = _per(kind, L)
        n0 = 16 * p  # a power-of-two chunk count: the second record's append adds a level
        t = Tree(gpu, kind, L, shift, _rand(n0 * L, 1200 + L).reshape(n0, L), 2 * n0 + 8)
        s0 = t.snap()
        v1 = _rand(3 * L, 1210 + L).reshape(3, L)
        a1 = t.args([17, n0 - 1], v1, 1)
        j1 = journal_arena(gpu, D.trees_journal_bytes([a1]))
        D.trees_journal([a1], j1.view("journal"))
        D.trees_update([a1])
        torch.cuda.synchronize()
        t.rows, t.n = t.after([17, n0 - 1], v1, 1), n0 + 1
        s1 = t.snap()
        v2 = _rand(4 * L, 1220 + L).reshape(4, L)
        a2 = t.args([18, n0], v2, 2)
        j2 = journal_arena(gpu, D.trees_journal_bytes([a2]))
        D.trees_journal([a2], j2.view("journal"))
        D.trees_update([a2])
        torch.cuda.synchronize()
        assert bytes(t.root.cpu().numpy()) == oracle_root(kind, L, t.after([18, n0], v2, 2))
        D.trees_restore([a2], j2.view("journal"))
        torch.cuda.synchronize()
        assert_same(t.snap(), s1, f"kind {kind}: after the newer record")
        D.trees_restore([a1], j1.view("journal"))
        torch.cuda.synchronize()
        t.n = n0
        assert_same(t.snap(), s0, f"kind {kind}: after both records")
        for a in (j1, j2, t.arena):
            a.check_guards(f"kind {kind}: ")


def test_graph_replayed_twice(gpu):
    """journal + update captured into one hipGraph, restore into another; replayed in turn, twice."""
    import torch

    from oracle import oracle as O
    from prysm_amd import device as D

    trees, offs = _three(gpu)
    msg = _rand(104, 1300)
    c = _container(gpu, msg)
    cm, cr = c.view("msg"), c.view("croot")
    D.trees_update([t.args(off=o) for t, o in zip(trees, offs)], cm, 104, cr)
    torch.cuda.synchronize()
    before = [t.snap() for t in trees]
    msg0, root0 = cm.cpu().numpy().copy(), cr.cpu().numpy().copy()
    sets = [([5, 999], 7), ([36], 2), ([0, 1023], 0)]
    vals = [_rand((len(i) + a) * t.L, 1310 + j).reshape(-1, t.L) for j, (t, (i, a)) in enumerate(zip(trees, sets))]
    args = [t.args(i, v, a, off=o) for t, (i, a), v, o in zip(trees, sets, vals, offs)]
    jr = journal_arena(gpu, D.trees_journal_bytes(args, 104))
    ws = torch.empty(D.trees_update_workspace_bytes(args), dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    fwd, back = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(fwd):
        D.trees_journal(args, jr.view("journal"), cm, 104, cr)
        D.trees_update(args, cm, 104, cr, ws)
    with torch.cuda.graph(back):
        D.trees_restore(args, jr.view("journal"), cm, 104, cr)
    want = [oracle_root(t.kind, t.L, t.after(i, v, a)) for t, (i, a), v in zip(trees, sets, vals)]
    for rep in range(2):
        fwd.replay()
        torch.cuda.synchronize()
        m = cm.cpu().numpy()
        for t, r, o in zip(trees, want, offs):
            assert bytes(t.root.cpu().numpy()) == r == bytes(m[o:o + 32]), f"replay {rep}: the update"
        assert bytes(cr.cpu().numpy()) == O.keccak256(bytes(m))
        back.replay()
        torch.cuda.synchronize()
        for j, t in enumerate(trees):
            assert_same(t.snap(), before[j], f"replay {rep}: tree {j} after the restore")
        assert np.array_equal(cm.cpu().numpy(), msg0) and np.array_equal(cr.cpu().numpy(), root0), f"replay {rep}"
    for a in [jr, c] + [t.arena for t in trees]:
        a.check_guards("graph: ")


def test_refusals(gpu):
    """A short journal is MK_ENOMEM, a misaligned one MK_EINVAL; nothing is written."""
    import torch

    from prysm_amd import device as D

    t = Tree(gpu, LIST, 32, 0, _rand(100 * 32, 1400).reshape(100, 32), 128)
    a = t.args([3], _rand(32, 1401).reshape(1, 32), 0)
    nbytes = D.trees_journal_bytes([a])
    jr = journal_arena(gpu, nbytes)
    for call in (D.trees_journal, D.trees_restore):
        with pytest.raises(_lib.MerkleError) as e:
            call([a], jr.view("journal")[:nbytes - 16])
        assert e.value.code == _lib.MK_ENOMEM
        with pytest.raises(_lib.MerkleError) as e:
            call([a], jr.view("journal")[8:])
        assert e.value.code == _lib.MK_EINVAL
    torch.cuda.synchronize()
    jr.assert_poison("journal", 0x3C)
    jr.check_guards()
