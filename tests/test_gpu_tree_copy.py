"""Resident trees copied on the device: the device entry
mk_dev_ssz_trees_copy between the layouts of two capacities, and clone /
copy_from / reserve / capacity of ListTree, StructListTree and BytesListTree.

The kinds, their pools of rows and the oracle are those of
tests/test_gpu_tree_shrink.py (a root is O.merkle_hash_flat over the level-0
entries of the listed rows: the items themselves, O.struct_roots or the
reflective oracle's struct hash, O.elem_digests), with the longer item lengths
of this file added.  Everything is compared bit for bit.

Device entry: a tree built by its kind's build entry at cap_src is copied into
buffers prefilled with 0xA5.  Every live extent (the values, level 0, the
ceil(nchunks / 2^d) nodes of each stored level at the offset cap_dst gives, the
root) must equal the source's, and every other byte must still be 0xA5.  Then a
one-value update and, where cap_dst has room, a one-value append run on the
destination at cap_dst: their roots are the oracle's only if every clean
sibling lies where the new layout puts it."""
import ctypes

import numpy as np
import pytest

from prysm_amd import _lib
from tests.test_gpu_tree_shrink import (POOL, Kind, _attestation_kind, _bytes_kind, _list_kind, _rand,  # noqa: F401
                                        _validator_kind, rows)

pytestmark = pytest.mark.gpu

FILL = 0xA5
COUNTS = [0, 1, 2, 4, 5, 8, 9, 16, 17, 33, 257, 1025, 4099]
KINDS = {
    "list-1": lambda: _list_kind(1), "list-8": lambda: _list_kind(8), "list-32": lambda: _list_kind(32),
    "list-48": lambda: _list_kind(48), "list-100": lambda: _list_kind(100), "list-128": lambda: _list_kind(128),
    "list-200": lambda: _list_kind(200),
    "bytes-32": lambda: _bytes_kind(32), "bytes-48": lambda: _bytes_kind(48),
    "struct-validator": _validator_kind, "struct-attestation": _attestation_kind,
}
_made = {}


def kind_of(name):
    if name not in _made:
        _made[name] = KINDS[name]()
    return _made[name]


def pairs(n):
    """(cap_src, cap_dst) for a list of n values."""
    return [(n, n), (n, n + 1), (n, 2 * n + 3), (2 * n + 3, n), (4099, 8200)]


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def levels_of(k, n, cap):
    """[(first node, live nodes)] of levels 1 .. D of n values in the layout of `cap` values."""
    c, cc, off, out = -(-n // k.per), -(-cap // k.per), 0, []
    while c > 1:
        c, cc = (c + 1) // 2, (cc + 1) // 2
        out.append((off, c))
        off += cc
    return out


class Bufs:
    """The four buffers of a tree of `kind` with room for `cap` values, every byte `fill`; the values at a
    byte offset `shift` of their allocation (a device-form buffer need not be aligned)."""

    def __init__(self, gpu, kind, cap, fill=0, shift=0):
        import torch

        from prysm_amd import device as D

        self.k, self.cap = kind, cap
        self.items_all = torch.full((cap * kind.L + 32 + shift,), fill, dtype=torch.uint8, device=gpu)
        self.items = self.items_all[shift:]
        self.level0 = None if kind.tree_kind == _lib.MK_TREE_LIST else \
            torch.full((32 * cap + 16,), fill, dtype=torch.uint8, device=gpu)
        self.lv = torch.full((max(D.list_tree_levels_bytes(cap, kind.len0), 16),), fill, dtype=torch.uint8, device=gpu)
        self.root = torch.full((32,), fill, dtype=torch.uint8, device=gpu)

    def build(self, cur):
        import torch

        from prysm_amd import device as D

        k, n = self.k, len(cur)
        if n:
            self.items[: n * k.L] = torch.from_numpy(k.pool[np.asarray(cur, dtype=np.int64)].reshape(-1).copy()).to(
                self.items.device)
        if k.tree_kind == _lib.MK_TREE_LIST:
            D.list_tree_build(self.items, n, self.cap, k.L, self.lv, self.root)
        elif k.tree_kind == _lib.MK_TREE_STRUCT:
            D.struct_list_tree_build(self.items, n, self.cap, k.L, k.fields, self.level0, self.lv, self.root)
        else:
            D.bytes_list_tree_build(self.items, n, self.cap, k.L, self.level0, self.lv, self.root)
        return self

    def update(self, n_old, n_new, idx, values):
        """One call of the kind's update entry at this capacity (idx: a list of indices, values: rows)."""
        import torch

        from prysm_amd import device as D

        k, dev = self.k, self.items.device
        d_idx = torch.tensor(idx, dtype=torch.int64, device=dev) if idx else None
        vals = torch.from_numpy(np.ascontiguousarray(values).reshape(-1).copy()).to(dev)
        if k.tree_kind == _lib.MK_TREE_LIST:
            D.list_tree_update(self.items, n_old, n_new, self.cap, k.L, self.lv, self.root, d_idx, len(idx), vals)
        elif k.tree_kind == _lib.MK_TREE_STRUCT:
            D.struct_list_tree_update(self.items, n_old, n_new, self.cap, k.L, k.fields, self.level0, self.lv, self.root,
                                      d_idx, len(idx), vals)
        else:
            D.bytes_list_tree_update(self.items, n_old, n_new, self.cap, k.L, self.level0, self.lv, self.root, d_idx,
                                     len(idx), vals)

    def host(self):
        return (self.items_all.cpu().numpy(), None if self.level0 is None else self.level0.cpu().numpy(),
                self.lv.cpu().numpy(), self.root.cpu().numpy())


def desc(src, dst, n):
    from prysm_amd import device as D

    return D.TreeCopyArgs(src.k.tree_kind, src.k.L, n, src.cap, dst.cap, src.items, src.lv, src.root, dst.items,
                          dst.lv, dst.root, src_level0=src.level0, dst_level0=dst.level0)


def check_copy(src, dst, n, what, shift_src=0, shift_dst=0):
    """Every live extent of dst equals src's, every other byte of dst's buffers is still FILL."""
    k = src.k
    s_items, s_l0, s_lv, s_root = src.host()
    d_items, d_l0, d_lv, d_root = dst.host()
    want = np.full_like(d_items, FILL)
    want[shift_dst: shift_dst + n * k.L] = s_items[shift_src: shift_src + n * k.L]
    assert np.array_equal(d_items, want), f"{what}: the values, or a byte beside them"
    if d_l0 is not None:
        want = np.full_like(d_l0, FILL)
        want[: 32 * n] = s_l0[: 32 * n]
        assert np.array_equal(d_l0, want), f"{what}: level 0, or a byte beside it"
    want = np.full_like(d_lv, FILL)
    for (so, cnt), (do, cnt2) in zip(levels_of(k, n, src.cap), levels_of(k, n, dst.cap)):
        assert cnt == cnt2
        want[32 * do: 32 * (do + cnt)] = s_lv[32 * so: 32 * (so + cnt)]
    assert np.array_equal(d_lv, want), f"{what}: a level's live nodes, or a node outside them"
    assert np.array_equal(d_root, s_root), f"{what}: the root"


def check_climbs(dst, cur, what, salt=0):
    """A one-value update and (with room) a one-value append on dst at its capacity give the oracle's roots."""
    import torch

    k, n = dst.k, len(cur)
    cur = list(cur)
    if n:
        i = n - 2 if n >= 2 else 0
        r = (salt + 3) % POOL
        dst.update(n, n, [i], k.pool[[r]])
        cur[i] = r
        torch.cuda.synchronize()
        assert bytes(dst.root.cpu().numpy()) == k.root(cur), f"{what}: the root after an update of [{i}]"
    if n < dst.cap:
        r = (salt + 7) % POOL
        dst.update(n, n + 1, [], k.pool[[r]])
        cur.append(r)
        torch.cuda.synchronize()
        assert bytes(dst.root.cpu().numpy()) == k.root(cur), f"{what}: the root after an append"
    return cur


@pytest.mark.parametrize("name", list(KINDS))
def test_copy_between_layouts(gpu, name):
    from prysm_amd import device as D

    k = kind_of(name)
    for n in COUNTS:
        built = {}
        for c, (cap_src, cap_dst) in enumerate(pairs(n)):
            if n > min(cap_src, cap_dst):
                continue  # (4099, 8200) holds every n of COUNTS; nothing else is skipped
            what = f"{name} n={n} {cap_src}->{cap_dst}"
            cur = rows(n, 1)
            if cap_src not in built:
                built[cap_src] = Bufs(gpu, k, cap_src).build(cur)
            src = built[cap_src]
            assert bytes(src.root.cpu().numpy()) == k.root(cur), f"{what}: the build"
            dst = Bufs(gpu, k, cap_dst, FILL)
            D.trees_copy([desc(src, dst, n)])
            check_copy(src, dst, n, what)
            check_climbs(dst, cur, what, salt=c)


@pytest.mark.parametrize("name,n", [("list-1", 4099), ("list-8", 1025), ("list-100", 257), ("list-200", 33)])
@pytest.mark.parametrize("shifts", [(8, 0), (0, 8), (4, 12), (1, 3), (16, 16), (2, 2)])
def test_unaligned_values(gpu, name, n, shifts):
    """A value buffer at any byte alignment, and a list whose n * item_len is no multiple of 16: pieces of
    8, 4 or 1 bytes, the last one short, and not a byte beside the values written."""
    from prysm_amd import device as D

    k = kind_of(name)
    cur = rows(n, 2)
    src = Bufs(gpu, k, n + 5, shift=shifts[0]).build(cur)
    dst = Bufs(gpu, k, 2 * n + 3, FILL, shift=shifts[1])
    D.trees_copy([desc(src, dst, n)])
    check_copy(src, dst, n, f"{name} shifts {shifts}", *shifts)
    check_climbs(dst, cur, f"{name} shifts {shifts}")


@pytest.mark.parametrize("name", ["list-8", "struct-validator", "bytes-32"])
def test_truncated_source_leaves_its_stale_nodes_behind(gpu, name):
    from prysm_amd import device as D

    k = kind_of(name)
    n0, n = 4099, 1025
    src = Bufs(gpu, k, n0).build(rows(n0))
    D.tree_erase(k.tree_kind, src.items, n0, n, n0, k.L, src.lv, src.root, level0=src.level0, spec=k.fields)
    cur = rows(n0)[:n]
    assert bytes(src.root.cpu().numpy()) == k.root(cur)
    dst = Bufs(gpu, k, 2 * n + 3, FILL)
    D.trees_copy([desc(src, dst, n)])
    check_copy(src, dst, n, f"{name} truncated")  # the stale values, level-0 entries and nodes stayed behind
    check_climbs(dst, cur, f"{name} truncated")


def test_three_trees_and_the_extra_in_one_call(gpu):
    import torch

    from prysm_amd import device as D

    shapes = [("list-48", 257, 300, 257), ("struct-validator", 1025, 1025, 2053), ("bytes-32", 33, 69, 40)]
    srcs, dsts, curs = [], [], []
    for j, (name, n, cap_src, cap_dst) in enumerate(shapes):
        curs.append(rows(n, j))
        srcs.append(Bufs(gpu, kind_of(name), cap_src).build(curs[-1]))
        dsts.append(Bufs(gpu, kind_of(name), cap_dst, FILL))
    extra_src = torch.arange(32, dtype=torch.uint8, device=gpu)
    extra_dst = torch.full((32,), FILL, dtype=torch.uint8, device=gpu)
    D.trees_copy([desc(s, d, len(c)) for s, d, c in zip(srcs, dsts, curs)], extra_src, extra_dst)
    for (name, n, _, _), s, d, c in zip(shapes, srcs, dsts, curs):
        check_copy(s, d, n, f"{name} of three")
        check_climbs(d, c, f"{name} of three")
    assert torch.equal(extra_dst, extra_src)
    # the extra alone, and nothing at all
    extra_dst.fill_(FILL)
    D.trees_copy([], extra_src, extra_dst)
    assert torch.equal(extra_dst, extra_src)
    _lib.invoke("mk_dev_ssz_trees_copy", None, 0, None, None, None)


def test_graph_copy(gpu):
    """One call captured (a single kernel node) and replayed twice, the source rebuilt in between."""
    import torch

    from prysm_amd import device as D

    k = kind_of("struct-attestation")
    n = 1025
    src = Bufs(gpu, k, n + 1).build(rows(n))
    dst = Bufs(gpu, k, 2 * n + 3, FILL)
    d = desc(src, dst, n)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.trees_copy([d])
    for rep in range(2):
        cur = rows(n, 5 + rep)
        src.build(cur)
        for t in (dst.items_all, dst.level0, dst.lv, dst.root):
            t.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        check_copy(src, dst, n, f"replay {rep}")
        check_climbs(dst, cur, f"replay {rep}")


def test_refused_calls_launch_nothing(gpu):
    """Every MK_EINVAL of the entry: the code, and the destination still holds 0xA5."""
    import torch

    from prysm_amd import device as D

    k = kind_of("bytes-32")
    n = 257
    src = Bufs(gpu, k, n + 3).build(rows(n))
    dst = Bufs(gpu, k, 2 * n + 3, FILL)
    kl = kind_of("list-8")
    lsrc = Bufs(gpu, kl, n).build(rows(n))
    ldst = Bufs(gpu, kl, n, FILL)

    def refused(what, trees, extra=(None, None), text=None):
        with pytest.raises(_lib.MerkleError) as e:
            D.trees_copy(trees, *extra)
        assert e.value.code == _lib.MK_EINVAL, what
        if text:
            assert text in str(e.value), f"{what}: {e.value}"
        torch.cuda.synchronize()
        for b in (dst, ldst):
            for t in (b.items_all, b.level0, b.lv, b.root):
                assert t is None or bool((t == FILL).all()), f"{what}: the destination was written"

    def edit(d, **kw):
        d = desc(*d)
        for key, v in kw.items():
            if key in ("src", "dst"):
                cur = list(getattr(d, key))
                for i, x in v.items():
                    cur[i] = x
                setattr(d, key, tuple(cur))
            else:
                setattr(d, key, v)
        return d

    B, Lst = (src, dst, n), (lsrc, ldst, n)
    ITEMS, LEVEL0, LEVELS, ROOT = 0, 1, 2, 3
    refused("null destination root", [edit(B, dst={ROOT: None})], text="null pointer")
    refused("null source root", [edit(B, src={ROOT: None})], text="null pointer")
    refused("null values", [edit(B, dst={ITEMS: None})], text="null pointer")
    refused("null level 0", [edit(B, src={LEVEL0: None})], text="null pointer")
    refused("null levels", [edit(B, dst={LEVELS: None})], text="null level array")
    refused("a level 0 for a list tree", [edit(Lst, dst={LEVEL0: dst.level0}, src={LEVEL0: src.level0})], text="list tree")
    refused("misaligned levels", [edit(B, dst={LEVELS: dst.items_all[8:]})], text="misaligned")
    refused("misaligned source levels", [edit(B, src={LEVELS: src.items_all[4:]})], text="misaligned")
    refused("misaligned level 0", [edit(B, dst={LEVEL0: dst.level0[8:]})], text="misaligned")
    refused("misaligned root", [edit(B, dst={ROOT: dst.items[8:]})], text="misaligned")
    refused("item_len == 0", [edit(Lst, item_len=0)], text="item_len == 0")
    refused("item_len above 2^30", [edit(Lst, item_len=(1 << 30) + 1, n=0, src={LEVELS: None}, dst={LEVELS: None})], text="2^30")
    refused("an unknown kind", [edit(B, kind=7)], text="unknown kind")
    refused("n above the source's capacity", [edit(Lst, n=n + 1, dst_capacity=n + 9)], text="capacity")
    refused("n above the destination's capacity", [edit(Lst, src_capacity=n + 9, n=n + 1)], text="capacity")
    refused("17 trees", [desc(*Lst)] * 17, text="17 trees")
    refused("a misaligned extra", [desc(*B)], extra=(src.root, dst.items[8:]), text="extra")
    refused("the values onto themselves", [edit(B, dst={ITEMS: src.items})], text="overlaps")
    refused("the source's levels as the destination's", [edit(B, dst_capacity=n + 3, dst={LEVELS: src.lv})],
            text="overlaps")
    refused("a destination root that is another tree's source", [desc(*B), edit(Lst, dst={ROOT: src.root})],
            text="overlaps")
    refused("the extra onto a source root", [desc(*B)], extra=(lsrc.root, src.root), text="overlaps")
    # a one-sided extra (the wrapper refuses it itself: straight to the entry)
    arr = (_lib.TreeCopy * 1)()
    with pytest.raises(_lib.MerkleError) as e:
        _lib.invoke("mk_dev_ssz_trees_copy", arr, 0, None, ctypes.c_void_p(dst.root.data_ptr()), None)
    assert e.value.code == _lib.MK_EINVAL
    assert bool((dst.root == FILL).all())
    # and the same descriptors, unedited, go through
    D.trees_copy([desc(*B), desc(*Lst)])
    check_copy(src, dst, n, "after the refused calls")
    check_copy(lsrc, ldst, n, "after the refused calls (list)")


# ---- the handles ---------------------------------------------------------------------------------
HANDLE_KINDS = ["list-8", "list-100", "struct-validator", "struct-attestation", "bytes-32", "bytes-48"]


class Model:
    def __init__(self, kind, tree, cur):
        self.k, self.t, self.cur = kind, tree, list(cur)

    def check(self, what):
        k, n = self.k, len(self.cur)
        assert len(self.t) == n, f"{what}: count"
        assert self.t.root() == k.root(self.cur), f"{what}: root"
        got = getattr(self.t, k.read)()
        assert got.shape == (n, k.L) and np.array_equal(got, k.pool[np.asarray(self.cur, dtype=np.int64)]), \
            f"{what}: read-back"

    def update(self, i, r):
        self.t.update([i], self.k.pool[[r]])
        self.cur[i] = r

    def append(self, rs):
        self.t.append(self.k.pool[rs])
        self.cur += list(rs)


def filled(k, n, cap, c=0):
    t = k.make(cap)
    t.assign(k.pool[rows(n, c)])
    return Model(k, t, rows(n, c))


@pytest.mark.parametrize("name", HANDLE_KINDS)
def test_clone_then_diverge(gpu, name):
    from prysm_amd.listtree import verify_branches

    k = kind_of(name)
    a = filled(k, 1025, 1100)
    b = Model(k, a.t.clone(), a.cur)
    assert type(b.t) is type(a.t) and b.t.capacity == a.t.capacity == 1100
    assert b.t.root() == a.t.root()
    b.check("the clone")
    b.update(1023, 7)       # next to the end of the clone
    a.append([11, 12, 13])  # and the source grows
    b.check("the clone after its update")
    a.check("the source after its append")  # neither saw the other's change
    b.t.truncate(600)
    b.cur = b.cur[:600]
    b.check("the clone truncated")
    b.append([(5 * j + 1) % POOL for j in range(450)])
    b.check("the clone re-appended")
    a.check("the source, untouched by all that")
    idx = [0, 5, 599, len(b.cur) - 1]
    vals, br = b.t.branches(idx)
    assert verify_branches(vals, idx, len(b.cur), k.len0, br, b.t.root()).all()
    e = filled(k, 0, 0)
    z = Model(k, e.t.clone(), [])
    z.check("a clone of the empty tree")
    z.append([1, 2, 3, 4, 5])
    z.check("... grown")


@pytest.mark.parametrize("name", HANDLE_KINDS)
def test_copy_from(gpu, name):
    k = kind_of(name)
    a = filled(k, 1025, 1200)
    big = filled(k, 7, 5000, 3)
    big.t.copy_from(a.t)
    big.cur = list(a.cur)
    assert big.t.capacity == 5000
    big.check("into a larger handle")
    big.update(1024, 9)
    big.append([21, 22])
    big.check("... then an update and an append in its own layout")
    fit = filled(k, 1030, 1030, 4)  # smaller than the source's capacity, and the values fit
    fit.t.copy_from(a.t)
    fit.cur = list(a.cur)
    assert fit.t.capacity == 1030
    fit.check("into a smaller handle that fits")
    fit.update(3, 9)
    fit.append([31])
    fit.check("... then an update and an append")
    tiny = filled(k, 9, 10, 5)
    tiny.t.copy_from(a.t)
    tiny.cur = list(a.cur)
    assert tiny.t.capacity == a.t.capacity == 1200  # it grew to the source's
    tiny.check("into a handle that was too small")
    tiny.update(1000, 9)
    tiny.append([41, 42, 43])
    tiny.check("... then an update and an append")
    a.t.copy_from(a.t)
    a.check("onto itself, and after being copied three times")


def test_copy_from_a_mismatch_changes_nothing(gpu):
    from prysm_amd.listtree import ListTree

    k8, kv, ka, kb = kind_of("list-8"), kind_of("struct-validator"), kind_of("struct-attestation"), kind_of("bytes-32")
    a8, av, aa, ab = filled(k8, 33, 40), filled(kv, 33, 40), filled(ka, 33, 40), filled(kb, 33, 40)
    t16 = ListTree(16, capacity=40)
    t16.assign(np.arange(16 * 5, dtype=np.uint8))
    r16 = t16.root()
    for dst, src, what in ((t16, a8.t, "another item length"), (a8.t, ab.t, "another kind"),
                           (av.t, aa.t, "another record layout"), (ab.t, a8.t, "another kind")):
        with pytest.raises(_lib.MerkleError) as e:
            dst.copy_from(src)
        assert e.value.code == _lib.MK_EINVAL, what
    assert t16.root() == r16 and len(t16) == 5
    # the C entry itself refuses a handle of another kind or length (no Python check in the way)
    for dst, src in ((a8.t, ab.t), (ab.t, av.t), (t16, a8.t)):
        with pytest.raises(_lib.MerkleError) as e:
            _lib.invoke(f"mk_{dst._prefix}_copy", dst._handle, src._handle)
        assert e.value.code == _lib.MK_EINVAL
    for m in (a8, av, aa, ab):
        m.check("after the refused copies")


@pytest.mark.parametrize("name", HANDLE_KINDS)
def test_reserve(gpu, name):
    k = kind_of(name)
    a = filled(k, 1025, 1025)
    cap, root = a.t.capacity, a.t.root()
    assert cap == 1025
    a.t.reserve(cap - 5)  # no-ops
    a.t.reserve(cap)
    assert a.t.capacity == cap
    a.t.reserve(2 * cap + 3)
    assert a.t.capacity == 2 * cap + 3 and a.t.root() == root
    a.check("reserved: nothing changed")
    a.update(1024, 2)
    a.check("an update in the new layout")
    a.append([(3 * j + 2) % POOL for j in range(2 * cap + 3 - 1025)])  # up to the new capacity: no rebuild by growth
    assert a.t.capacity == 2 * cap + 3
    a.check("appended up to the new capacity")
