"""mk_dev_ssz_trees_update (several resident trees in one launch,
k_trees_update) against the existing single-tree update entry points and the
oracle.  Every case is run on TWIN copies of the same built buffers: one goes
through the new call, the other through its kind's own
mk_dev_ssz_*_tree_update; the item buffer, level 0, every stored level and the
root must be equal byte for byte, and level 0 and the root must equal the
oracle's (O.merkle_hash_flat over the items, over O.struct_roots /
oracle/ssz_ref.tree_hash of every record, over O.elem_digests).  Then the
container hash, back-to-back calls, two streams and a replayed hipGraph.
(device_levels is test_gpu_list_tree.py's; random lives of mixed trees and
the container at every length class are in test_gpu_tree_fuzz.py.)"""
import numpy as np
import pytest

from prysm_amd import _lib
from prysm_amd import registry as R
from prysm_amd import state as ST

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000000 + 3100
LIST, STRUCT, BYTES = _lib.MK_TREE_LIST, _lib.MK_TREE_STRUCT, _lib.MK_TREE_BYTES


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def _rand(nbytes, salt):
    from oracle import oracle as O

    return O.splitmix_bytes((nbytes + 7) // 8 * 8, SEED + salt)[:nbytes].copy()


class Case:
    """One tree and one change to it.  ``pool``: (m, L) rows, the first n_old
    the list, the next len(idx) the new values of ``idx`` (ascending; an index
    >= n_old is ignored), the next n_app the appended rows.  ``pool0``: the
    oracle's level-0 entry (struct root, element digest) of every pool row."""

    def __init__(self, kind, L, pool, pool0, n_old, cap, idx=(), n_app=0, spec=None, off=0):
        self.kind, self.L, self.pool, self.pool0, self.spec, self.off = kind, L, pool, pool0, spec, off
        self.n_old, self.cap, self.idx, self.n_app = n_old, cap, np.asarray(idx, dtype=np.int64), n_app
        self.n_new = n_old + n_app
        k = len(self.idx)
        assert n_old + k + n_app <= len(pool) and self.n_new <= cap
        self.values = pool[n_old:n_old + k + n_app]

        def final(p):
            rows = p[:n_old].copy()
            for j, i in enumerate(self.idx):
                if i < n_old:
                    rows[i] = p[n_old + j]
            return np.concatenate([rows, p[n_old + k:n_old + k + n_app]])

        from oracle import oracle as O

        self.want_rows = final(pool)
        self.want0 = final(pool0) if kind != LIST else None
        lv0, len0 = (self.want_rows, L) if kind == LIST else (self.want0, 32)
        self.want_root = O.merkle_hash_flat(np.ascontiguousarray(lv0).reshape(-1), self.n_new, len0)


class Twin:
    """A device tree of a case, built by its kind's own build entry."""

    def __init__(self, gpu, c):
        import torch

        from prysm_amd import device as D

        self.c = c
        self.base = torch.zeros(max(c.cap * c.L, 8) + 32, dtype=torch.uint8, device=gpu)
        self.items = self.base[c.off:c.off + max(c.cap * c.L, 8)]
        self.items[:c.n_old * c.L].copy_(torch.from_numpy(np.ascontiguousarray(c.pool[:c.n_old]).reshape(-1)))
        self.level0 = torch.zeros(max(32 * c.cap, 32), dtype=torch.uint8, device=gpu) if c.kind != LIST else None
        self.lv = torch.zeros(max(D.list_tree_levels_bytes(c.cap, c.L if c.kind == LIST else 32), 32),
                              dtype=torch.uint8, device=gpu)
        self.root = torch.zeros(32, dtype=torch.uint8, device=gpu)
        if c.kind == LIST:
            D.list_tree_build(self.items, c.n_old, c.cap, c.L, self.lv, self.root)
        elif c.kind == STRUCT:
            D.struct_list_tree_build(self.items, c.n_old, c.cap, c.L, c.spec, self.level0, self.lv, self.root)
        else:
            D.bytes_list_tree_build(self.items, c.n_old, c.cap, c.L, self.level0, self.lv, self.root)
        k = len(c.idx)
        self.d_idx = torch.from_numpy(c.idx).to(gpu) if k else None
        self.d_vals = (torch.from_numpy(np.ascontiguousarray(c.values).reshape(-1)).to(gpu)
                       if len(c.values) else None)

    def args(self, container_off=None):
        from prysm_amd import device as D

        c = self.c
        return D.TreeArgs(c.kind, self.items, c.n_old, c.n_new, c.cap, c.L, self.lv, self.root, level0=self.level0,
                          idx=self.d_idx, k_idx=len(c.idx), values=self.d_vals, spec=c.spec,
                          container_off=container_off)

    def single(self):
        """The existing single-tree update entry with the same arguments."""
        from prysm_amd import device as D

        c, k = self.c, len(self.c.idx)
        if c.kind == LIST:
            D.list_tree_update(self.items, c.n_old, c.n_new, c.cap, c.L, self.lv, self.root, self.d_idx, k,
                               self.d_vals)
        elif c.kind == STRUCT:
            D.struct_list_tree_update(self.items, c.n_old, c.n_new, c.cap, c.L, c.spec, self.level0, self.lv,
                                      self.root, self.d_idx, k, self.d_vals)
        else:
            D.bytes_list_tree_update(self.items, c.n_old, c.n_new, c.cap, c.L, self.level0, self.lv, self.root,
                                     self.d_idx, k, self.d_vals)


def check_twins(a, b, what):
    """a: after the new call, b: after the single-tree entry; then a against the oracle."""
    from tests.test_gpu_list_tree import device_levels

    c = a.c
    assert np.array_equal(a.base.cpu().numpy(), b.base.cpu().numpy()), f"{what}: items differ"
    assert np.array_equal(a.items[:c.n_new * c.L].cpu().numpy(), c.want_rows.reshape(-1)), f"{what}: items"
    if c.kind != LIST:
        assert np.array_equal(a.level0.cpu().numpy(), b.level0.cpu().numpy()), f"{what}: level 0 differs"
        got0 = a.level0[:32 * c.n_new].cpu().numpy().reshape(c.n_new, 32)
        bad = np.flatnonzero((got0 != c.want0).any(axis=1))
        assert bad.size == 0, f"{what}: level 0 entries {bad[:8]} against the oracle"
    len0 = c.L if c.kind == LIST else 32
    la, lb = device_levels(a.lv, c.n_new, c.cap, len0), device_levels(b.lv, c.n_new, c.cap, len0)
    assert len(la) == len(lb)
    for d, (x, y) in enumerate(zip(la, lb), 1):
        bad = np.flatnonzero((x != y).any(axis=1))
        assert bad.size == 0, f"{what}: level {d} nodes {bad[:8]} differ"
    assert np.array_equal(a.lv.cpu().numpy(), b.lv.cpu().numpy()), f"{what}: level array differs"
    ra, rb = bytes(a.root.cpu().numpy()), bytes(b.root.cpu().numpy())
    assert ra == rb, f"{what}: roots differ"
    assert ra == c.want_root, f"{what}: root against the oracle"


# ---- the cases: built once, shared, never changed -------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    from oracle import oracle as O
    from oracle import ssz_ref as OS
    from tests.ssz_types import to_ref_type

    out = {}

    def lst(name, L, n_old, cap, idx=(), n_app=0, salt=0):
        m = n_old + len(idx) + n_app
        out[name] = Case(LIST, L, _rand(max(m, 1) * L, salt).reshape(-1, L)[:m], None, n_old, cap, idx, n_app)

    def byt(name, L, n_old, cap, idx=(), n_app=0, salt=0, off=0):
        m = n_old + len(idx) + n_app
        pool = _rand(m * L, salt).reshape(m, L)
        out[name] = Case(BYTES, L, pool, O.elem_digests(pool.reshape(-1), m, L), n_old, cap, idx, n_app, off=off)

    lst("L8 k1", 8, 1000, 1024, [517], salt=1)
    lst("L8 k3 app5", 8, 1000, 1024, [0, 511, 999], 5, salt=2)
    lst("L8 k0", 8, 1000, 1024, salt=3)
    lst("L8 ignored", 8, 1000, 1024, [10, 1000, 5000], salt=4)
    lst("L32 n5", 32, 5, 8, [4], salt=5)
    lst("L32 n3", 32, 3, 8, [1], salt=6)
    lst("L32 n0", 32, 0, 8, salt=7)
    lst("L200 n3", 200, 3, 4, [2], salt=8)
    lst("L32 all64", 32, 64, 64, list(range(64)), salt=9)
    lst("L32 run", 32, 64, 64, [6, 7, 8, 9], salt=10)
    byt("B32 8192", 32, 8192, 8192, [4242], salt=11)
    byt("B48 odd", 48, 37, 64, [3, 36], 1, salt=12, off=1)
    byt("B32 n3", 32, 3, 4, [2], salt=13)
    byt("B32 ignored", 32, 100, 128, [7, 100], salt=14)
    # validator records: 4099, 7 dirty ones with two adjacent pairs
    m = 4099 + 7
    pool = R.synthetic_registry(m, SEED + 20).records.view(np.uint8).reshape(m, 160)
    out["S validator"] = Case(STRUCT, 160, pool, O.struct_roots(pool, m, 160, R.VALIDATOR_FIELDS), 4099, 4099,
                              [0, 17, 18, 1023, 2048, 4097, 4098], spec=R.VALIDATOR_FIELDS)
    st = ST.synthetic_state(0, SEED + 21, n_attestations=12, n_batched=0, n_votes=6, lists_len=1100, shards=1024)
    val = st.as_value()
    # crosslinks: 1024 + 2 new values (the pool continues with two more records)
    cr = np.concatenate([ST.pack_crosslinks(st.crosslink_epochs, st.crosslink_roots),
                         _rand(2 * 40, 22).reshape(2, 40)])
    out["S crosslink"] = Case(STRUCT, 40, cr, O.struct_roots(cr, len(cr), 40, ST.CROSSLINK_FIELDS), 1024, 1024,
                              [5, 1000], spec=ST.CROSSLINK_FIELDS)
    out["S crosslink ignored"] = Case(STRUCT, 40, cr, out["S crosslink"].pool0, 50, 64, [3, 77],
                                      spec=ST.CROSSLINK_FIELDS)
    # nested layouts: the oracle's reflective hasher roots every record
    att, _ = ST.pack_attestations(st.attestations, 48)
    att0 = np.stack([np.frombuffer(OS.tree_hash(to_ref_type(ST.PENDING_ATTESTATION_SSZ), v), np.uint8)
                     for v in val["LatestAttestations"]])
    out["S attestation 9+3"] = Case(STRUCT, att.shape[1], att, att0, 9, 16, n_app=3,
                                    spec=ST.PENDING_ATTESTATION_FIELDS)
    out["S attestation 3+9"] = Case(STRUCT, att.shape[1], att, att0, 3, 16, n_app=9,
                                    spec=ST.PENDING_ATTESTATION_FIELDS)
    vo = ST.pack_eth1_votes(st.eth1_votes, st.eth1_vote_counts)
    vo0 = np.stack([np.frombuffer(OS.tree_hash(to_ref_type(ST.ETH1_VOTE_SSZ), v), np.uint8)
                    for v in val["Eth1DataVotes"]])
    out["S vote n4"] = Case(STRUCT, 72, vo, vo0, 4, 4, [1, 3], spec=ST.ETH1_VOTE_FIELDS)
    return out


def run_call(gpu, cs, what, **kw):
    """One mk_dev_ssz_trees_update over the cases ``cs`` against the single-tree entries on their twins."""
    import torch

    from prysm_amd import device as D

    a, b = [Twin(gpu, c) for c in cs], [Twin(gpu, c) for c in cs]
    D.trees_update([t.args() for t in a], **kw)
    for t in b:
        t.single()
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(a, b)):
        check_twins(x, y, f"{what}, tree {i}")
    return a


ALL = ["L8 k1", "L8 k3 app5", "L8 k0", "L8 ignored", "L32 n5", "L32 n3", "L32 n0", "L200 n3", "L32 all64", "L32 run",
       "B32 8192", "B48 odd", "B32 n3", "B32 ignored", "S validator", "S crosslink", "S crosslink ignored",
       "S attestation 9+3", "S attestation 3+9", "S vote n4"]


@pytest.mark.parametrize("name", ALL)
def test_one_tree(gpu, cases, name):
    assert set(ALL) == set(cases)
    run_call(gpu, [cases[name]], name)


@pytest.mark.parametrize("ntrees,seed", [(10, 1), (10, 2), (16, 3), (16, 4)])
def test_many_trees_shuffled(gpu, cases, ntrees, seed):
    rng = np.random.default_rng(seed)
    names = [ALL[i] for i in rng.permutation(len(ALL))[:ntrees]]
    run_call(gpu, [cases[n] for n in names], f"{ntrees} trees {names}")


def test_every_case_in_two_calls_of_ten(gpu, cases):
    rng = np.random.default_rng(9)
    order = [ALL[i] for i in rng.permutation(len(ALL))]
    for part in (order[:10], order[10:]):
        run_call(gpu, [cases[n] for n in part], f"{part}")


# ---- the container --------------------------------------------------------------------------------
TEN = ["S validator", "L8 k3 app5", "B32 8192", "S crosslink", "B48 odd", "B32 n3", "L8 k1", "S attestation 3+9",
       "L32 n0", "S vote n4"]
OFFS = [0, 40, 72, 232, 264, 296, 328, 360, 392, 456]  # the state's own (prysm_amd.state.CONTAINER_OFF)


@pytest.mark.parametrize("mode", ["all ten", "some outside", "nothing dirty"])
def test_container_root(gpu, cases, mode):
    import torch

    from oracle import oracle as O
    from prysm_amd import device as D

    cs = [cases[n] for n in TEN]
    if mode == "nothing dirty":  # the same lists with no index, no value, no append
        cs = [Case(c.kind, c.L, c.pool, c.pool0, c.n_old, c.cap, spec=c.spec, off=c.off) for c in cs]
    offs = [None if mode == "some outside" and i in (1, 4, 9) else o for i, o in enumerate(OFFS)]
    msg = _rand(536, 40)
    a, b = [Twin(gpu, c) for c in cs], [Twin(gpu, c) for c in cs]
    container = torch.from_numpy(np.concatenate([msg, np.full(8, 0xA5, np.uint8)])).to(gpu)
    croot = torch.full((40,), 0x5A, dtype=torch.uint8, device=gpu)
    D.trees_update([t.args(o) for t, o in zip(a, offs)], container, 536, croot)
    for t in b:
        t.single()
    torch.cuda.synchronize()
    want = msg.copy()
    for i, (x, y, o) in enumerate(zip(a, b, offs)):
        check_twins(x, y, f"{mode}, tree {i}")
        if o is not None:
            want[o:o + 32] = np.frombuffer(cs[i].want_root, np.uint8)
    got = container.cpu().numpy()
    assert np.array_equal(got[:536], want), "the container message"
    assert (got[536:] == 0xA5).all(), "bytes behind the container"
    got = croot.cpu().numpy()
    assert bytes(got[:32]) == O.keccak256(bytes(want)), "the container root"
    assert (got[32:] == 0x5A).all()


def test_no_container_writes_nothing(gpu, cases):
    import torch

    from prysm_amd import _lib as L
    from prysm_amd import device as D

    cs = [cases[n] for n in TEN[:3]]
    a = [Twin(gpu, c) for c in cs]
    container = torch.full((544,), 0xA5, dtype=torch.uint8, device=gpu)
    croot = torch.full((32,), 0x5A, dtype=torch.uint8, device=gpu)
    # container_len == 0: the wrapper passes NULL; call the entry itself with the canary buffers
    arr, _keep = D._tree_table([t.args() for t in a])
    ws = torch.empty(D.trees_update_workspace_bytes([t.args() for t in a]), dtype=torch.uint8, device=gpu)
    L.invoke("mk_dev_ssz_trees_update", arr, len(a), container.data_ptr(), 0, croot.data_ptr(), ws.data_ptr(),
             ws.numel(), torch.cuda.current_stream(gpu).cuda_stream, device=0)
    torch.cuda.synchronize()
    assert (croot.cpu().numpy() == 0x5A).all() and (container.cpu().numpy() == 0xA5).all()
    for t in a:
        assert bytes(t.root.cpu().numpy()) == t.c.want_root


# ---- 20 calls back to back, one stream, one workspace, no sync -------------------------------------
def _steps(gpu, nsteps, salt, stream=None):
    """Three trees (a list, a bytes list, a struct list) and ``nsteps`` changes
    to each: the enqueue closure of every step and the roots the oracle wants
    after it."""
    import torch

    from oracle import oracle as O
    from prysm_amd import device as D

    rng = np.random.default_rng(salt)
    shapes = [(LIST, 8, 1000, None), (BYTES, 32, 8192, None), (STRUCT, 40, 1024, ST.CROSSLINK_FIELDS)]
    rows = [_rand(n * L, salt + 10 * i).reshape(n, L) for i, (_, L, n, _) in enumerate(shapes)]
    twins = [Twin(gpu, Case(kind, L, r, np.zeros((n, 32), np.uint8), n, n, spec=spec))
             for (kind, L, n, spec), r in zip(shapes, rows)]
    offs = [0, 40, 72]
    msg = _rand(104, salt + 5)
    container = torch.from_numpy(msg.copy()).to(gpu)
    trees0 = [t.args(o) for t, o in zip(twins, offs)]
    ws = torch.empty(2 * D.trees_update_workspace_bytes(trees0) + 4096, dtype=torch.uint8, device=gpu)
    calls, wants, keep = [], [], []
    for s in range(nsteps):
        trees, want = [], msg.copy()
        roots = torch.zeros(3 * 32 + 32, dtype=torch.uint8, device=gpu)
        for i, ((kind, L, n, spec), t) in enumerate(zip(shapes, twins)):
            k = int(rng.integers(1, 4))
            idx = np.sort(rng.choice(n, k, replace=False)).astype(np.int64)
            vals = _rand(k * L, salt + 100 * s + i).reshape(k, L)
            rows[i][idx] = vals
            d_idx, d_vals = torch.from_numpy(idx).to(gpu), torch.from_numpy(vals.reshape(-1)).to(gpu)
            keep.append((d_idx, d_vals))
            trees.append(D.TreeArgs(kind, t.items, n, n, n, L, t.lv, roots[32 * i:32 * i + 32], level0=t.level0,
                                    idx=d_idx, k_idx=k, values=d_vals, spec=spec, container_off=offs[i]))
            if kind == LIST:
                r = O.merkle_hash_flat(rows[i].reshape(-1), n, L)
            elif kind == BYTES:
                r = O.merkle_hash_flat(O.elem_digests(rows[i].reshape(-1), n, L).reshape(-1), n, 32)
            else:
                r = O.merkle_hash_flat(O.struct_roots(rows[i], n, L, spec).reshape(-1), n, 32)
            want[offs[i]:offs[i] + 32] = np.frombuffer(r, np.uint8)
        wants.append((roots, want.copy(), O.keccak256(bytes(want))))
        calls.append(lambda trees=trees, roots=roots: D.trees_update(trees, container, 104, roots[96:], ws))
    return calls, wants, keep


def _check_steps(wants, what):
    for s, (roots, want, croot) in enumerate(wants):
        got = roots.cpu().numpy()
        for i, o in enumerate((0, 40, 72)):
            assert np.array_equal(got[32 * i:32 * i + 32], want[o:o + 32]), f"{what}: call {s}, tree {i}"
        assert bytes(got[96:]) == croot, f"{what}: call {s}, container root"


def test_twenty_calls_back_to_back(gpu):
    import torch

    calls, wants, _keep = _steps(gpu, 20, 500)
    torch.cuda.synchronize()
    for c in calls:
        c()
    torch.cuda.synchronize()
    _check_steps(wants, "back to back")


def test_two_streams(gpu):
    import torch

    work = [_steps(gpu, 6, 600 + 50 * i) for i in range(2)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(gpu) for _ in range(2)]
    for s in range(6):
        for i in range(2):
            with torch.cuda.stream(streams[i]):
                work[i][0][s]()
    torch.cuda.synchronize()
    for i in range(2):
        _check_steps(work[i][1], f"stream {i}")


# ---- a replayed graph -----------------------------------------------------------------------------
def test_graph_replay(gpu, cases):
    import torch

    from oracle import oracle as O
    from prysm_amd import device as D

    shapes = [(LIST, 8, 1000, None), (BYTES, 32, 8192, None), (STRUCT, 40, 1024, ST.CROSSLINK_FIELDS),
              (BYTES, 32, 3, None)]
    k = 3
    rows = [_rand(n * L, 700 + i).reshape(n, L) for i, (_, L, n, _) in enumerate(shapes)]
    twins = [Twin(gpu, Case(kind, L, r, np.zeros((n, 32), np.uint8), n, n, spec=spec))
             for (kind, L, n, spec), r in zip(shapes, rows)]
    offs = [0, 40, 72, 104]
    msg = _rand(136, 710)
    container = torch.from_numpy(msg.copy()).to(gpu)
    croot = torch.zeros(32, dtype=torch.uint8, device=gpu)
    d_idx = [torch.zeros(k, dtype=torch.int64, device=gpu) for _ in shapes]
    d_vals = [torch.zeros(k * L, dtype=torch.uint8, device=gpu) for _, L, _, _ in shapes]
    for i, (_, L, n, _) in enumerate(shapes):  # the capture run writes the items as they are
        idx = np.arange(k, dtype=np.int64)
        d_idx[i].copy_(torch.from_numpy(idx))
        d_vals[i].copy_(torch.from_numpy(np.ascontiguousarray(rows[i][idx]).reshape(-1)))
    trees = [D.TreeArgs(kind, t.items, n, n, n, L, t.lv, t.root, level0=t.level0, idx=d_idx[i], k_idx=k,
                        values=d_vals[i], spec=spec, container_off=offs[i])
             for i, ((kind, L, n, spec), t) in enumerate(zip(shapes, twins))]
    ws = torch.empty(D.trees_update_workspace_bytes(trees), dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # memset, every stage 0, the one climb: a linear chain
        D.trees_update(trees, container, 136, croot, ws)
    rng = np.random.default_rng(11)
    for rep in range(3):
        want = msg.copy()
        for i, (kind, L, n, spec) in enumerate(shapes):
            idx = np.sort(rng.choice(n, k, replace=False)).astype(np.int64)
            vals = _rand(k * L, 720 + 10 * rep + i).reshape(k, L)
            rows[i][idx] = vals
            d_idx[i].copy_(torch.from_numpy(idx))
            d_vals[i].copy_(torch.from_numpy(vals.reshape(-1)))
            if kind == LIST:
                r = O.merkle_hash_flat(rows[i].reshape(-1), n, L)
            elif kind == BYTES:
                r = O.merkle_hash_flat(O.elem_digests(rows[i].reshape(-1), n, L).reshape(-1), n, 32)
            else:
                r = O.merkle_hash_flat(O.struct_roots(rows[i], n, L, spec).reshape(-1), n, 32)
            want[offs[i]:offs[i] + 32] = np.frombuffer(r, np.uint8)
        g.replay()
        torch.cuda.synchronize()
        for i, t in enumerate(twins):
            assert np.array_equal(t.root.cpu().numpy(), want[offs[i]:offs[i] + 32]), f"replay {rep}, tree {i}"
            assert np.array_equal(t.items[:rows[i].size].cpu().numpy(), rows[i].reshape(-1)), f"replay {rep}: items"
        assert bytes(croot.cpu().numpy()) == O.keccak256(bytes(want)), f"replay {rep}: container root"
