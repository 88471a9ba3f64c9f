"""The device-resident tree of a list of byte strings
(mk_dev_ssz_bytes_list_tree_build / _update, mk_bytes_list_tree): the element
buffer, EVERY stored element digest, EVERY stored node of every level and the
root against the oracle -- digests[i] = Keccak(le32(elem_len) || e_i)
(O.elem_digests), then the level-by-level restatement of
tests/test_gpu_list_tree.py over the oracle's Keccak -- after builds, in-place
updates, appends, a random sequence, two trees on two streams and a replayed
hipGraph.  The root is also held against the one-shot
mk_ssz_tree_hash_bytes_list and the reflective oracle/ssz_ref.tree_hash of
Slice(Bytes).  An update is k_list_tree_scatter (with d_values),
k_bytes_tree_digest and k_list_tree_update."""
import numpy as np
import pytest

from prysm_amd import _lib
from tests.test_gpu_list_tree import device_levels, oracle_tree

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000000 + 2400
# MK_BYTES_TREE_REBUILD_DIV (prysm_amd/csrc/bytes_tree_api.cpp): the handle rebuilds from count / DIV dirty elements
REBUILD_DIV = 256
# (elem_len, byte offset of the element buffer from a 16-B aligned address): 32-B elements
# at an aligned base take the one-permutation digest, everything else the general sponge
KINDS = {"32": (32, 0), "32+4": (32, 4), "132": (132, 0)}


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def _rand(nbytes, salt):
    from oracle import oracle as O

    return O.splitmix_bytes((nbytes + 7) // 8 * 8, SEED + salt)[:nbytes].copy()


class Model:
    """The host model: `cap` elements and their oracle digests."""

    def __init__(self, elem_len, cap, salt):
        from oracle import oracle as O

        self.L = elem_len
        self.el = _rand(max(cap, 1) * elem_len, salt).reshape(-1, elem_len)[:cap]
        self.dig = O.elem_digests(self.el.reshape(-1), cap, elem_len, nthreads=16)

    def copy(self):
        m = Model.__new__(Model)
        m.L, m.el, m.dig = self.L, self.el.copy(), self.dig.copy()
        return m

    def set(self, idx, vals):
        from oracle import oracle as O

        idx = np.asarray(idx, dtype=np.int64)
        if idx.size:
            vals = np.ascontiguousarray(vals, dtype=np.uint8).reshape(idx.size, self.L)
            self.el[idx] = vals
            self.dig[idx] = O.elem_digests(vals.reshape(-1), idx.size, self.L, nthreads=16)

    def root(self, n):
        from oracle import oracle as O

        return O.merkle_hash_flat(self.dig[:n].reshape(-1), n, 32)


class Tree:
    """A device bytes tree built from the first n elements of a model; the
    element buffer starts `off` bytes past a 16-B aligned address."""

    def __init__(self, gpu, model, n, cap, off=0):
        import torch

        from prysm_amd import device as D

        self.n, self.cap, self.L = n, cap, model.L
        self.base = torch.zeros(max(cap * self.L, 8) + 16, dtype=torch.uint8, device=gpu)
        assert self.base.data_ptr() % 16 == 0
        self.elems = self.base[off:off + max(cap * self.L, 8)]
        self.elems[:n * self.L].copy_(torch.from_numpy(np.ascontiguousarray(model.el[:n]).reshape(-1)))
        self.dig = torch.zeros(max(32 * cap, 32), dtype=torch.uint8, device=gpu)
        self.lv = torch.zeros(max(D.list_tree_levels_bytes(cap, 32), 32), dtype=torch.uint8, device=gpu)
        self.root = torch.zeros(32, dtype=torch.uint8, device=gpu)
        D.bytes_list_tree_build(self.elems, n, cap, self.L, self.dig, self.lv, self.root)

    def update(self, model, idx=(), values=None, n_new=None, scatter=True, ws=None):
        """values: (len(idx) + appended, L) uint8 host array, already applied
        to `model`.  scatter=False: the caller writes the new elements itself
        (here: the model's first n_new elements, uploaded whole on the same
        stream) and passes d_values == NULL."""
        import torch

        from prysm_amd import device as D

        gpu = self.elems.device
        n_new = self.n if n_new is None else n_new
        idx = np.asarray(idx, dtype=np.int64)
        d_idx = torch.from_numpy(idx).to(gpu) if idx.size else None
        d_vals = None
        if values is not None and np.asarray(values).size:
            if scatter:
                d_vals = torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint8).reshape(-1)).to(gpu)
            else:
                self.elems[:n_new * self.L].copy_(
                    torch.from_numpy(np.ascontiguousarray(model.el[:n_new]).reshape(-1)))
        D.bytes_list_tree_update(self.elems, self.n, n_new, self.cap, self.L, self.dig, self.lv, self.root, d_idx,
                                 idx.size, d_vals, ws=ws)
        self.n = n_new


def check_tree(tree, model, what, one_shot=False):
    """Elements, every digest, every level and the root against the oracle."""
    import torch

    torch.cuda.synchronize()
    n, L = tree.n, tree.L
    assert np.array_equal(tree.elems[:n * L].cpu().numpy(), model.el[:n].reshape(-1)), f"{what}: elements"
    got_dig = tree.dig[:32 * n].cpu().numpy().reshape(n, 32)
    bad = np.flatnonzero((got_dig != model.dig[:n]).any(axis=1))
    assert bad.size == 0, f"{what}: digests {bad[:8]} of {n}"
    levels, root = oracle_tree(model.dig[:n].reshape(-1), n, 32)
    assert root == model.root(n)
    assert bytes(tree.root.cpu().numpy()) == root, f"{what}: root"
    got = device_levels(tree.lv, n, tree.cap, 32)
    assert len(got) == len(levels)
    for d, (g, w) in enumerate(zip(got, levels), 1):
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, f"{what}: level {d} nodes {bad[:8]} of {len(w)}"
    if one_shot:  # the one-shot library root and the reflective restatement of the same list
        from oracle import ssz_ref as OS
        from prysm_amd import ssz

        assert ssz.tree_hash_bytes_list(model.el[:n].reshape(-1), n, L) == root, f"{what}: one-shot root"
        if n <= 1000:
            assert OS.tree_hash(("slice", ("bytes",)), [bytes(e) for e in model.el[:n]]) == root, what


# ---- build: digests, every level, the root ----------------------------------------------------
BUILD_SIZES = [0, 1, 4, 5, 8, 9, 1000, (1 << 16) + 3]  # around one chunk, one window; odd levels; many blocks
# 4 + elem_len around the 136-B rate: the pad inside the block (131), at its end (132), in a
# second block (133); 300: three blocks
BUILD_KINDS = [(1, 0), (32, 0), (32, 4), (48, 0), (131, 0), (132, 0), (133, 0), (300, 0)]


@pytest.mark.parametrize("elem_len,off", BUILD_KINDS, ids=[f"{L}+{o}" for L, o in BUILD_KINDS])
def test_build_every_level(gpu, elem_len, off):
    m = Model(elem_len, BUILD_SIZES[-1], elem_len)
    for n in BUILD_SIZES:
        for cap in (n, n + 1000):
            check_tree(Tree(gpu, m, n, cap, off), m, f"L={elem_len}+{off} n={n} cap={cap}", one_shot=cap == n)


# ---- update in place --------------------------------------------------------------------------
def dirty_sets(n, rng):
    return [
        ("one element", [n // 3]),
        ("the first and the last", [0, n - 1]),
        ("all 8 of one window", list(range(40, 48))),
        ("7 of 8 in one window and 1 in the next", list(range(48, 55)) + [57]),
        ("every 8th element", list(range(5, n, 8))),
        ("a random 5 %", sorted(rng.choice(n, max(n // 20, 1), replace=False).tolist())),
        ("every element", list(range(n))),
    ]


@pytest.mark.parametrize("n", [1000, (1 << 16) + 3])
@pytest.mark.parametrize("kind", list(KINDS))
def test_update_in_place(gpu, kind, n):
    L, off = KINDS[kind]
    m = Model(L, n, 100 + n)
    t = Tree(gpu, m, n, n, off)
    check_tree(t, m, "build")
    rng = np.random.default_rng(n)
    step = 0
    for scatter in (True, False):
        for name, idx in dirty_sets(n, rng):
            step += 1
            vals = _rand(len(idx) * L, 1000 * step + n).reshape(-1, L)
            m.set(idx, vals)
            t.update(m, idx, vals, scatter=scatter)
            check_tree(t, m, f"{kind} {name}, d_values={scatter}")
    t.update(m)  # nothing changed: the root is written again
    t.root.zero_()
    t.update(m)
    check_tree(t, m, "no-op")


# ---- append through update --------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_append_through_update(gpu, kind):
    L, off = KINDS[kind]
    cap = 1021 + 4096 + 100
    m0 = Model(L, cap, 300)
    for n_old in (0, 3, 4, 7, 1021):  # inside a chunk, at its edge, inside a window, an odd chunk count
        for k in (1, 5, 4096):        # across a chunk, a window and several levels
            for with_idx in (False, True):  # with_idx: in-place changes and an append in one call
                if with_idx and (n_old < 7 or k == 4096):
                    continue
                for scatter in (True, False):
                    m = m0.copy()
                    t = Tree(gpu, m, n_old, cap, off)
                    idx = sorted({0, n_old // 2, n_old - 1}) if with_idx else []
                    n_new = n_old + k
                    vals = _rand((len(idx) + k) * L, 7 * n_new + n_old).reshape(-1, L)
                    m.set(idx, vals[:len(idx)])
                    m.set(list(range(n_old, n_new)), vals[len(idx):])
                    t.update(m, idx, vals, n_new=n_new, scatter=scatter)
                    check_tree(t, m, f"{kind} {n_old}->{n_new} idx={with_idx} d_values={scatter}")


# ---- an index >= n_old ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_out_of_range_index_is_ignored(gpu, kind):
    import torch

    L, off = KINDS[kind]
    n = 4001
    m = Model(L, n, 900)
    t = Tree(gpu, m, n, n + 100, off)
    assert not torch.any(t.elems[n * L:]) and not torch.any(t.dig[32 * n:])
    vals = _rand(4 * L, 901).reshape(4, L)
    m.set([5, 9], vals[:2])
    t.update(m, [5, 9, n + 7, n + 50], vals)  # elements n + 7, n + 50 lie inside the capacity: they stay untouched
    check_tree(t, m, "out-of-range index")
    assert not torch.any(t.elems[n * L:]), "elements past the list were written"
    assert not torch.any(t.dig[32 * n:]), "digests past the list were written"
    t.root.zero_()
    t.update(m, [n + 1])  # pre-written form (nothing to write): the same root, nothing moves
    check_tree(t, m, "only an out-of-range index")
    assert not torch.any(t.dig[32 * n:])
    # with an append in the same call: the bytes past n_new stay as they were
    app = _rand(3 * L, 902).reshape(3, L)
    m2 = Model.__new__(Model)
    m2.L, m2.el, m2.dig = L, np.concatenate([m.el, np.zeros((3, L), np.uint8)]), np.concatenate(
        [m.dig, np.zeros((3, 32), np.uint8)])
    v = _rand(2 * L, 903).reshape(2, L)
    m2.set([17], v[:1])
    m2.set([n, n + 1, n + 2], app)
    t.update(m2, [17, n + 60], np.concatenate([v, app]), n_new=n + 3)
    check_tree(t, m2, "out-of-range index beside an append")
    assert not torch.any(t.elems[(n + 3) * L:]) and not torch.any(t.dig[32 * (n + 3):])


# ---- a random sequence ------------------------------------------------------------------------
def test_random_sequence(gpu):
    import torch

    cap, n = 5000, 1500
    m = Model(32, cap, 400)
    t = Tree(gpu, m, n, cap)
    rng = np.random.default_rng(12345)
    for step in range(30):
        kind = step % 3  # update, append, no-op
        idx = sorted(rng.choice(n, int(rng.integers(1, 200)), replace=False).tolist()) if kind == 0 else []
        n_new = min(n + int(rng.integers(1, 400)), cap) if kind == 1 else n
        vals = _rand((len(idx) + n_new - n) * 32, 5000 + step).reshape(-1, 32)
        m.set(idx, vals[:len(idx)])
        m.set(list(range(n, n_new)), vals[len(idx):])
        t.root.zero_()
        t.update(m, idx, vals, n_new=n_new, scatter=bool(step & 1))
        n = n_new
        torch.cuda.synchronize()
        assert bytes(t.root.cpu().numpy()) == m.root(n), step
    check_tree(t, m, "after 30 steps")


# ---- two trees on two streams -----------------------------------------------------------------
def test_two_streams(gpu):
    import torch

    from prysm_amd import device as D

    sizes, ks, steps = [(1 << 16) + 3, 1000], [3000, 5], [3, 24]  # a wide update beside a loop of small ones
    models = [Model(32, sizes[i], 500 + i) for i in range(2)]
    trees = [Tree(gpu, models[i], sizes[i], sizes[i]) for i in range(2)]
    rng = np.random.default_rng(77)
    work = [[], []]  # per tree and step: (d_idx, d_vals), uploaded before the streams start
    for i in range(2):
        for s in range(steps[i]):
            idx = np.sort(rng.choice(sizes[i], ks[i], replace=False)).astype(np.int64)
            vals = _rand(ks[i] * 32, 6000 + 100 * i + s).reshape(ks[i], 32)
            models[i].set(idx, vals)
            work[i].append((torch.from_numpy(idx).to(gpu), torch.from_numpy(vals.reshape(-1)).to(gpu)))
    wss = [torch.empty(D.bytes_list_tree_update_workspace_bytes(ks[i], 32), dtype=torch.uint8, device=gpu)
           for i in range(2)]
    streams = [torch.cuda.Stream(gpu) for _ in range(2)]
    torch.cuda.synchronize()
    for s in range(max(steps)):
        for i in range(2):
            if s < steps[i]:
                with torch.cuda.stream(streams[i]):
                    tr, n = trees[i], sizes[i]
                    D.bytes_list_tree_update(tr.elems, n, n, n, 32, tr.dig, tr.lv, tr.root, work[i][s][0], ks[i],
                                             work[i][s][1], ws=wss[i])
    for i in range(2):
        check_tree(trees[i], models[i], f"tree {i}")


# ---- a replayed graph -------------------------------------------------------------------------
def test_graph_update(gpu):
    import torch

    from prysm_amd import device as D

    n, k = 40_003, 64
    m = Model(32, n, 600)
    t = Tree(gpu, m, n, n)
    d_idx = torch.zeros(k, dtype=torch.int64, device=gpu)
    d_vals = torch.zeros(k * 32, dtype=torch.uint8, device=gpu)
    ws = torch.empty(D.bytes_list_tree_update_workspace_bytes(k, 32), dtype=torch.uint8, device=gpu)
    rng = np.random.default_rng(5)
    idx = np.sort(rng.choice(n, k, replace=False)).astype(np.int64)
    d_idx.copy_(torch.from_numpy(idx))
    d_vals.copy_(torch.from_numpy(np.ascontiguousarray(m.el[idx]).reshape(-1)))  # the elements as they are
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # scatter, digests, memset, climb: a single linear chain
        D.bytes_list_tree_update(t.elems, n, n, n, 32, t.dig, t.lv, t.root, d_idx, k, d_vals, ws=ws)
    for rep in range(2):
        idx = np.sort(rng.choice(n, k, replace=False)).astype(np.int64)
        vals = _rand(k * 32, 700 + rep).reshape(k, 32)
        m.set(idx, vals)
        d_idx.copy_(torch.from_numpy(idx))
        d_vals.copy_(torch.from_numpy(vals.reshape(-1)))
        g.replay()
        check_tree(t, m, f"after replay {rep}")


# ---- the handle -------------------------------------------------------------------------------
@pytest.mark.parametrize("elem_len", [32, 132])
def test_handle_against_oracle(gpu, elem_len):
    from prysm_amd.listtree import BytesListTree

    L = elem_len
    m = Model(L, 40_000, 800)
    t = BytesListTree(L, capacity=12_000)
    assert len(t) == 0 and t.root() == m.root(0)  # merkleHash([])
    n = 10_241
    t.assign(m.el[:n])
    assert len(t) == n and t.root() == m.root(n)
    # unsorted indices with repeats: the last value of an index wins
    idx = np.array([700, 3, n - 1, 3, 1999, 700, 0, 3], dtype=np.uint64)
    vals = _rand(idx.size * L, 810).reshape(-1, L)
    for i, v in zip(idx, vals):
        m.set([int(i)], v)
    t.update(idx, vals)
    assert t.root() == m.root(n)
    assert np.array_equal(t.elems(), m.el[:n])
    assert np.array_equal(t.elems(1998, 3), m.el[1998:2001])
    # an index >= count is refused and changes nothing
    with pytest.raises(_lib.MerkleError) as e:
        t.update([1, n], _rand(2 * L, 811).reshape(2, L))
    assert e.value.code == _lib.MK_EINVAL
    assert t.root() == m.root(n) and np.array_equal(t.elems(0, 2), m.el[:2])
    # just below the rebuild share (the climb), just above it and far above it (rebuilds)
    for k in (n // REBUILD_DIV - 1, n // REBUILD_DIV + 1, 1, n // 3):
        idx = np.random.default_rng(k).choice(n, k, replace=False)
        vals = _rand(k * L, 820 + k).reshape(-1, L)
        m.set(idx, vals)
        t.update(idx, vals)
        assert t.root() == m.root(n), k
    # appends: a few (the climb), many (a rebuild), then past the capacity (grow + rebuild)
    for k in (7, 1500, 20_000):
        t.append(m.el[n:n + k])
        n += k
        assert len(t) == n and t.root() == m.root(n), k
    t.update([n - 1], m.el[0:1])  # a small one climbs the rebuilt levels
    m.set([n - 1], m.el[0:1].copy())
    assert t.root() == m.root(n)
    assert np.array_equal(t.elems(), m.el[:n])
