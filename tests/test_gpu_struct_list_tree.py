"""The device-resident registry tree (mk_dev_ssz_struct_list_tree_build /
_update, mk_struct_list_tree, registry.ResidentState): the record buffer, the
struct roots, EVERY stored node of every level and the root against the
oracle -- O.struct_roots, then the level-by-level restatement of
tests/test_gpu_list_tree.py over the oracle's Keccak, then O.merkle_hash_flat
-- after builds, in-place updates, appends, a random sequence, two trees on
two streams and a replayed hipGraph.  V is the validator layout, G a layout
whose struct roots take the two-launch form (a 96-B bytes field, a 2-byte
scalar); an update is k_struct_tree_gather (records pre-written), the
struct-roots launch, k_list_tree_scatter and k_list_tree_update."""
import numpy as np
import pytest

from prysm_amd import _lib
from tests.test_gpu_list_tree import device_levels, oracle_tree

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000000 + 2300
B, R = _lib.MK_FIELD_BYTES, _lib.MK_FIELD_RAW
V = (160, [(B, 0, 48), (B, 48, 32), (B, 80, 32)] + [(R, 112 + 8 * k, 8) for k in range(6)])
G = (108, [(B, 0, 96), (R, 96, 8), (R, 104, 2)])  # not a k_struct_fused layout
LAYOUTS = {"V": V, "G": G}
# MK_STRUCT_TREE_REBUILD_DIV (prysm_amd/csrc/struct_tree_api.cpp): the handle rebuilds from count / DIV dirty records
REBUILD_DIV = 32


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
    """The host model: `cap` records and their oracle struct roots."""

    def __init__(self, layout, cap, salt):
        from oracle import oracle as O

        self.R, self.spec = layout
        self.rec = _rand(max(cap, 1) * self.R, salt).reshape(-1, self.R)[:cap]
        self.roots = O.struct_roots(self.rec.reshape(-1), cap, self.R, self.spec)

    def set(self, idx, vals):
        from oracle import oracle as O

        idx = np.asarray(idx, dtype=np.int64)
        if idx.size:
            vals = np.ascontiguousarray(vals, dtype=np.uint8).reshape(idx.size, self.R)
            self.rec[idx] = vals
            self.roots[idx] = O.struct_roots(vals.reshape(-1), idx.size, self.R, self.spec)

    def root(self, n):
        from oracle import oracle as O

        return O.merkle_hash_flat(self.roots[:n].reshape(-1), n, 32)


class Tree:
    """A device registry tree built from the first n records of a model."""

    def __init__(self, gpu, model, n, cap):
        import torch

        from prysm_amd import device as D

        self.n, self.cap, self.R, self.spec = n, cap, model.R, model.spec
        self.recs = torch.zeros(max(cap * self.R, 8), dtype=torch.uint8, device=gpu)
        self.recs[:n * self.R] = torch.from_numpy(np.ascontiguousarray(model.rec[:n]).reshape(-1)).to(gpu)
        self.roots = torch.zeros(max(32 * cap, 32), dtype=torch.uint8, device=gpu)
        self.lv = torch.zeros(max(D.list_tree_levels_bytes(cap, 32), 32), dtype=torch.uint8, device=gpu)
        self.root = torch.zeros(32, dtype=torch.uint8, device=gpu)
        D.struct_list_tree_build(self.recs, n, cap, self.R, self.spec, self.roots, self.lv, self.root)

    def update(self, idx=(), values=None, n_new=None, scatter=True, ws=None):
        """values: (len(idx) + appended, R) uint8 host array."""
        import torch

        from prysm_amd import device as D

        gpu = self.recs.device
        n_new = self.n if n_new is None else n_new
        idx = np.asarray(idx, dtype=np.int64)
        vals = np.ascontiguousarray(values, dtype=np.uint8).reshape(-1, self.R) if values is not None else None
        d_idx = torch.from_numpy(idx).to(gpu) if idx.size else None
        d_vals = None
        if vals is not None and vals.size:
            if scatter:
                d_vals = torch.from_numpy(vals.reshape(-1)).to(gpu)
            else:  # the caller writes the new records itself, on the same stream
                v = torch.from_numpy(vals).to(gpu)
                if idx.size:
                    self.recs[:self.n * self.R].view(self.n, self.R)[d_idx] = v[:idx.size]
                if n_new > self.n:
                    self.recs[self.n * self.R:n_new * self.R] = v[idx.size:].reshape(-1)
        D.struct_list_tree_update(self.recs, self.n, n_new, self.cap, self.R, self.spec, self.roots, self.lv,
                                  self.root, d_idx, idx.size, d_vals, ws=ws)
        self.n = n_new


def check_tree(tree, model, what):
    """Records, struct roots, every level and the root against the oracle."""
    import torch

    torch.cuda.synchronize()
    n, R_ = tree.n, tree.R
    assert np.array_equal(tree.recs[:n * R_].cpu().numpy(), model.rec[:n].reshape(-1)), f"{what}: records"
    got_roots = tree.roots[:32 * n].cpu().numpy().reshape(n, 32)
    bad = np.flatnonzero((got_roots != model.roots[:n]).any(axis=1))
    assert bad.size == 0, f"{what}: struct roots {bad[:8]} of {n}"
    levels, root = oracle_tree(model.roots[:n].reshape(-1), n, 32)
    assert root == model.root(n)
    assert bytes(tree.root.cpu().numpy()) == root, f"{what}: root"
    got = device_levels(tree.lv, n, tree.cap, 32)
    assert len(got) == len(levels)
    for d, (g, w) in enumerate(zip(got, levels), 1):
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, f"{what}: level {d} nodes {bad[:8]} of {len(w)}"


# ---- build: roots, every level, the root ------------------------------------------------------
BUILD_SIZES = [0, 1, 4, 5, 7, 8, 9, 15, 16, 17, 1000, 4099]  # around one chunk, one window, odd levels


@pytest.mark.parametrize("layout", ["V", "G"])
def test_build_every_level(gpu, layout):
    m = Model(LAYOUTS[layout], BUILD_SIZES[-1], 1)
    for n in BUILD_SIZES:
        for cap in (n, n + n // 2 + 3):
            check_tree(Tree(gpu, m, n, cap), m, f"{layout} n={n} cap={cap}")


# ---- update in place --------------------------------------------------------------------------
def dirty_sets(n, rng):
    return [
        ("first", [0]),
        ("last record (of the ragged window)", [n - 1]),
        ("all 8 of one window", list(range(40, 48))),
        ("2 in sibling windows", [8 * 6 + 1, 8 * 7 + 2]),
        ("2 meeting at the top node", [3, n - 2]),
        ("one per window over 64 windows", [8 * (11 + i) + i % 8 for i in range(64)]),
        ("every record", list(range(n))),
        ("1 % random", sorted(rng.choice(n, max(n // 100, 1), replace=False).tolist())),
    ]


@pytest.mark.parametrize("layout,n", [("V", 1000), ("V", (1 << 16) + 3), ("G", 1000)])
def test_update_in_place(gpu, layout, n):
    m = Model(LAYOUTS[layout], n, 100 + n)
    t = Tree(gpu, m, n, n)
    check_tree(t, m, "build")
    rng = np.random.default_rng(n)
    step = 0
    for scatter in (True, False):
        for name, idx in dirty_sets(n, rng):
            step += 1
            vals = _rand(len(idx) * m.R, 1000 * step + n).reshape(-1, m.R)
            m.set(idx, vals)
            t.update(idx, vals, scatter=scatter)
            check_tree(t, m, f"{layout} {name}, d_values={scatter}")
    t.update()  # nothing changed: the root is written again
    t.root.zero_()
    t.update()
    check_tree(t, m, "no-op")


# ---- append through update --------------------------------------------------------------------
APPENDS = ([("window edge", 39, 39 + k) for k in (1, 3, 8, 9)]
           + [("chunks 8 -> 9 and up (a new level)", 32, 32 + k) for k in (1, 3, 8, 9)]
           + [("chunks 1024 -> 1025 and up", 4096, 4096 + k) for k in (1, 9)]
           + [("from 0", 0, k) for k in (1, 3, 8, 9)]
           + [("one chunk", 3, 4), ("one chunk to two", 4, 5), ("ragged window", 43, 61)])


@pytest.mark.parametrize("layout", ["V", "G"])
def test_append_through_update(gpu, layout):
    cap = 4400
    m0 = Model(LAYOUTS[layout], cap, 300)
    for name, n_old, n_new in APPENDS:
        for with_idx in (False, True):
            for scatter in (True, False):
                m = Model.__new__(Model)
                m.R, m.spec, m.rec, m.roots = m0.R, m0.spec, m0.rec.copy(), m0.roots.copy()
                t = Tree(gpu, m, n_old, cap)
                idx = sorted({0, n_old // 2, n_old - 1}) if with_idx and n_old else []
                vals = _rand((len(idx) + n_new - n_old) * m.R, 7 * n_new + n_old).reshape(-1, m.R)
                m.set(idx, vals[:len(idx)])
                m.set(list(range(n_old, n_new)), vals[len(idx):])
                t.update(idx, vals, n_new=n_new, scatter=scatter)
                check_tree(t, m, f"{layout} {name} {n_old}->{n_new} idx={with_idx} d_values={scatter}")


# ---- an index >= n_old ------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["V", "G"])
def test_out_of_range_index_is_ignored(gpu, layout):
    import torch

    n = 4001
    m = Model(LAYOUTS[layout], n, 900)
    t = Tree(gpu, m, n, n + 100)
    vals = _rand(4 * m.R, 901).reshape(4, m.R)
    m.set([5, 9], vals[:2])
    t.update([5, 9, n + 7, n + 50], vals)  # records n + 7, n + 50 lie inside the capacity: they stay untouched
    check_tree(t, m, "out-of-range index")
    assert not torch.any(t.recs[n * m.R:]), "records past the list were written"
    assert not torch.any(t.roots[32 * n:]), "roots past the list were written"
    t.root.zero_()
    t.update([n + 1])  # pre-written form (nothing to write): the same root, nothing moves
    check_tree(t, m, "only an out-of-range index")
    assert not torch.any(t.roots[32 * n:])


# ---- a random sequence ------------------------------------------------------------------------
def test_random_sequence(gpu):
    import torch

    cap, n = 1 << 15, 5000
    m = Model(V, cap, 400)
    t = Tree(gpu, m, n, cap)
    rng = np.random.default_rng(12345)
    for step in range(30):
        kind = step % 3  # update, append, no-op
        idx = sorted(rng.choice(n, int(rng.integers(1, 300)), replace=False).tolist()) if kind == 0 else []
        n_new = min(n + int(rng.integers(1, 900)), cap) if kind == 1 else n
        vals = _rand((len(idx) + n_new - n) * m.R, 5000 + step).reshape(-1, m.R)
        m.set(idx, vals[:len(idx)])
        m.set(list(range(n, n_new)), vals[len(idx):])
        t.root.zero_()
        t.update(idx, vals, n_new=n_new, scatter=bool(step & 1))
        n = n_new
        torch.cuda.synchronize()
        assert bytes(t.root.cpu().numpy()) == m.root(n), step
    check_tree(t, m, "after 30 steps")


# ---- two trees on two streams -----------------------------------------------------------------
def test_two_streams(gpu):
    import torch

    from prysm_amd import device as D

    sizes, ks, steps = [(1 << 16) + 3, 1000], [6000, 5], [3, 24]  # a wide update beside a loop of small ones
    models = [Model(V, sizes[i], 500 + i) for i in range(2)]
    trees = [Tree(gpu, models[i], sizes[i], sizes[i]) for i in range(2)]
    rng = np.random.default_rng(77)
    work = [[], []]  # per tree and step: (d_idx, d_vals), uploaded before the streams start
    for i in range(2):
        for s in range(steps[i]):
            idx = np.sort(rng.choice(sizes[i], ks[i], replace=False)).astype(np.int64)
            vals = _rand(ks[i] * 160, 6000 + 100 * i + s).reshape(ks[i], 160)
            models[i].set(idx, vals)
            work[i].append((torch.from_numpy(idx).to(gpu), torch.from_numpy(vals.reshape(-1)).to(gpu)))
    wss = [torch.empty(D.struct_list_tree_update_workspace_bytes(ks[i], V[1]), dtype=torch.uint8, device=gpu)
           for i in range(2)]
    streams = [torch.cuda.Stream(gpu) for _ in range(2)]
    torch.cuda.synchronize()
    for s in range(max(steps)):
        for i in range(2):
            if s < steps[i]:
                with torch.cuda.stream(streams[i]):
                    tr, n = trees[i], sizes[i]
                    D.struct_list_tree_update(tr.recs, n, n, n, 160, V[1], tr.roots, tr.lv, tr.root, work[i][s][0],
                                              ks[i], work[i][s][1], ws=wss[i])
    for i in range(2):
        check_tree(trees[i], models[i], f"tree {i}")


# ---- a replayed graph -------------------------------------------------------------------------
def test_graph_update(gpu):
    import torch

    from prysm_amd import device as D

    n, k = 40_003, 64
    m = Model(V, n, 600)
    t = Tree(gpu, m, n, n)
    d_idx = torch.zeros(k, dtype=torch.int64, device=gpu)
    d_vals = torch.zeros(k * 160, dtype=torch.uint8, device=gpu)
    ws = torch.empty(D.struct_list_tree_update_workspace_bytes(k, V[1]), dtype=torch.uint8, device=gpu)
    rng = np.random.default_rng(5)
    idx = np.sort(rng.choice(n, k, replace=False)).astype(np.int64)
    d_idx.copy_(torch.from_numpy(idx))
    d_vals.copy_(t.recs.view(-1, 160)[d_idx].reshape(-1))  # the capture's own run rewrites the same records
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # scatters, struct roots, memset, climb: a single linear chain
        D.struct_list_tree_update(t.recs, n, n, n, 160, V[1], t.roots, t.lv, t.root, d_idx, k, d_vals, ws=ws)
    for rep in range(3):
        idx = np.sort(rng.choice(n, k, replace=False)).astype(np.int64)
        vals = _rand(k * 160, 700 + rep).reshape(k, 160)
        m.set(idx, vals)
        d_idx.copy_(torch.from_numpy(idx))
        d_vals.copy_(torch.from_numpy(vals.reshape(-1)))
        g.replay()
        torch.cuda.synchronize()
        assert bytes(t.root.cpu().numpy()) == m.root(n), rep
    check_tree(t, m, "after 3 replays")


# ---- the handle -------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["V", "G"])
def test_handle_against_oracle(gpu, layout):
    from prysm_amd.listtree import StructListTree

    R_, spec = LAYOUTS[layout]
    m = Model(LAYOUTS[layout], 40_000, 800)
    t = StructListTree(R_, spec, capacity=12_000)
    assert len(t) == 0 and t.root() == m.root(0)  # merkleHash([])
    n = 10_241
    t.assign(m.rec[:n])
    assert len(t) == n and t.root() == m.root(n)
    # unsorted indices with repeats: the last value of an index wins
    idx = np.array([700, 3, n - 1, 3, 1999, 700, 0, 3], dtype=np.uint64)
    vals = _rand(idx.size * R_, 810).reshape(-1, R_)
    for i, v in zip(idx, vals):
        m.set([int(i)], v)
    t.update(idx, vals)
    assert t.root() == m.root(n)
    assert np.array_equal(t.records(), m.rec[:n])
    assert np.array_equal(t.records(1998, 3), m.rec[1998:2001])
    # an index >= count is refused and changes nothing
    with pytest.raises(_lib.MerkleError) as e:
        t.update([1, n], _rand(2 * R_, 811).reshape(2, R_))
    assert e.value.code == _lib.MK_EINVAL
    assert t.root() == m.root(n) and np.array_equal(t.records(0, 2), m.rec[:2])
    # just below the rebuild threshold (the climb) and just above it (a rebuild)
    for k in (n // REBUILD_DIV - 1, n // REBUILD_DIV + 1, 1, n // 3):
        idx = np.random.default_rng(k).choice(n, k, replace=False)
        vals = _rand(k * R_, 820 + k).reshape(-1, R_)
        m.set(idx, vals)
        t.update(idx, vals)
        assert t.root() == m.root(n), k
    # appends: a few (the climb), many (a rebuild), then past the capacity (grow + rebuild)
    for k in (7, 1500, 20_000):
        t.append(m.rec[n:n + k])
        n += k
        assert len(t) == n and t.root() == m.root(n), k
    t.update([n - 1], m.rec[0:1])  # a small one climbs the rebuilt levels
    m.set([n - 1], m.rec[0:1].copy())
    assert t.root() == m.root(n)
    assert np.array_equal(t.records(), m.rec[:n])


# ---- State{registry, balances} ----------------------------------------------------------------
def test_resident_state(gpu):
    from oracle import oracle as O
    from prysm_amd import registry as Rg

    n, extra = 4099, 9
    rec = Rg.synthetic_registry(n + extra, SEED + 1).records.copy()
    bal = Rg.synthetic_balances(n + extra, SEED + 2).copy()
    st = Rg.ResidentState(capacity=n)
    st.assign(rec[:n], bal[:n])
    rng = np.random.default_rng(9)
    for rnd in range(3):
        vi = rng.choice(n, 17, replace=False)
        rec[vi] = Rg.synthetic_registry(17, SEED + 10 + rnd).records
        st.update_validators(vi, rec[vi])
        bi = rng.choice(n, 40, replace=False)
        bal[bi] = rng.integers(0, 1 << 62, 40, dtype=np.uint64)
        st.update_balances(bi, bal[bi])
    st.append(rec[n:], bal[n:])
    n += extra
    assert len(st) == n
    raw = rec.view(np.uint8).reshape(n, 160)
    reg_root = O.merkle_hash_flat(O.struct_roots(raw.reshape(-1), n, 160, Rg.VALIDATOR_FIELDS).reshape(-1), n, 32)
    bal_root = O.merkle_hash_flat(np.ascontiguousarray(bal, dtype="<u8").view(np.uint8), n, 8)
    want = O.keccak256(reg_root + bal_root)
    assert st.root() == want
    assert Rg.state_root(Rg.ValidatorRegistry(rec), bal) == want
