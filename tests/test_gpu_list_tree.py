"""The device-resident list tree (mk_dev_ssz_list_tree_build / _update):
the root and EVERY stored node of every level against a restatement of the
definition (include/prysm_merkle.h) over the oracle's
Keccak, after builds, in-place updates, appends, a random sequence, two trees
on two streams and a replayed hipGraph.  oracle_tree, split_levels /
device_levels and compare_tree / check_tree live here and are shared with
test_gpu_trees_update.py, test_gpu_tree_fuzz.py and test_tree_fuzz_host.py
(compare_tree is check_tree's comparison over host arrays)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000000 + 2100


@pytest.fixture(scope="module")
def gpu():
    import torch

    from prysm_amd import _lib

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def _per(L):
    return 128 // L if L < 128 else 1


def _chunks(n, L):
    return -(-n // _per(L))


def oracle_tree(buf, n, L):
    """(levels, root): levels[d - 1] is the (c_d, 32) array of level d >= 1."""
    from oracle import oracle as O

    buf = np.ascontiguousarray(buf, dtype=np.uint8)[:n * L]
    root = O.merkle_hash_flat(buf, n, L)
    cb, nch, total = _per(L) * L, _chunks(n, L), n * L
    levels = []
    if nch <= 1:
        return levels, root
    c1 = (nch + 1) // 2
    full = c1 - 1  # every level-1 node but the last is two whole chunks
    nodes = np.empty((c1, 32), dtype=np.uint8)
    if full:
        nodes[:full] = O.keccak256_batch(buf[:full * 2 * cb], 2 * cb)
    last = bytes(buf[full * 2 * cb:total]) + (bytes(128) if nch & 1 else b"")
    nodes[full] = O.keccak256_var([last])[0]
    levels.append(nodes)
    while len(nodes) > 1:
        c = len(nodes)
        nxt = np.empty(((c + 1) // 2, 32), dtype=np.uint8)
        if c // 2:
            nxt[:c // 2] = O.keccak256_batch(nodes[:2 * (c // 2)].reshape(-1), 64)
        if c & 1:
            nxt[c // 2] = O.keccak256_var([bytes(nodes[c - 1]) + bytes(128)])[0]
        levels.append(nxt)
        nodes = nxt
    # the restatement agrees with the oracle's own merkleHash
    assert O.keccak256(bytes(nodes[0]) + n.to_bytes(8, "little") + bytes(24)) == root
    return levels, root


def split_levels(host, n, cap, L):
    """The stored nodes of every level of a level array held in a host array."""
    out, off, capd, c = [], 0, _chunks(cap, L), _chunks(n, L)
    while c > 1:
        capd, c = (capd + 1) // 2, (c + 1) // 2
        out.append(host[32 * off:32 * (off + c)].reshape(c, 32))
        off += capd
    return out


def device_levels(lv, n, cap, L):
    return split_levels(lv.cpu().numpy(), n, cap, L)


def compare_tree(items, got, root, want_buf, n, L, what):
    """Host arrays (the item buffer, split_levels' levels, the root) against a
    fresh oracle build: the comparison of check_tree, without a device."""
    assert np.array_equal(items[:n * L], want_buf[:n * L]), f"{what}: items"
    levels, want_root = oracle_tree(want_buf, n, L)
    assert bytes(root) == want_root, f"{what}: root"
    assert len(got) == len(levels)
    for d, (g, w) in enumerate(zip(got, levels), 1):
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, f"{what}: level {d} nodes {bad[:8]} of {len(w)}"


def check_tree(tree, want_buf, what):
    """Item buffer, every level and the root against a fresh oracle build."""
    import torch

    torch.cuda.synchronize()
    n, L = tree.n, tree.L
    compare_tree(tree.items[:n * L].cpu().numpy(), device_levels(tree.lv, n, tree.cap, L),
                 tree.root.cpu().numpy(), want_buf, n, L, what)


class Tree:
    """A device list tree built from `buf` (n items of L bytes)."""

    def __init__(self, gpu, buf, n, L, cap):
        import torch

        from prysm_amd import device as D

        self.n, self.L, self.cap = n, L, cap
        self.items = torch.zeros(max(cap * L, 8), dtype=torch.uint8, device=gpu)
        self.items[:n * L] = torch.from_numpy(np.ascontiguousarray(buf[:n * L])).to(gpu)
        self.lv = torch.zeros(max(D.list_tree_levels_bytes(cap, L), 32), dtype=torch.uint8, device=gpu)
        self.root = torch.zeros(32, dtype=torch.uint8, device=gpu)
        D.list_tree_build(self.items, n, cap, L, self.lv, self.root)

    def update(self, idx=(), values=None, n_new=None, scatter=True, ws=None):
        """values: (len(idx) + appended, L) uint8 host array."""
        import torch

        from prysm_amd import device as D

        gpu = self.items.device
        n_new = self.n if n_new is None else n_new
        idx = np.asarray(idx, dtype=np.int64)
        vals = np.ascontiguousarray(values, dtype=np.uint8).reshape(-1, self.L) if values is not None else None
        d_idx = torch.from_numpy(idx).to(gpu) if idx.size else None
        d_vals = None
        if vals is not None and vals.size:
            if scatter:
                d_vals = torch.from_numpy(vals.reshape(-1)).to(gpu)
            else:  # the caller writes the new bytes itself, on the same stream
                v = torch.from_numpy(vals).to(gpu)
                if idx.size:
                    self.items[:self.n * self.L].view(self.n, self.L)[d_idx] = v[:idx.size]
                if n_new > self.n:
                    self.items[self.n * self.L:n_new * self.L] = v[idx.size:].reshape(-1)
        D.list_tree_update(self.items, self.n, n_new, self.cap, self.L, self.lv, self.root, d_idx, idx.size, d_vals,
                           ws=ws)
        self.n = n_new


def _rand(nbytes, salt):
    from oracle import oracle as O

    return O.splitmix_bytes((nbytes + 7) // 8 * 8, SEED + salt)[:nbytes].copy()


# ---- build: every level ---------------------------------------------------------------------
CHUNK_COUNTS = [0, 1, 2, 3, 4, 5, (1 << 3) + 1, (1 << 10) + 1, 1000, 4097, (1 << 16) + 3]


@pytest.mark.parametrize("L", [1, 8, 32, 48, 128, 200])
def test_build_every_level(gpu, L):
    p = _per(L)
    buf = _rand(CHUNK_COUNTS[-1] * p * L, L)
    for nch in CHUNK_COUNTS:
        ns = {nch * p}  # a full last chunk
        if nch and p > 1:
            ns.add(nch * p - (p - 1))  # a ragged one (a single item)
            ns.add(nch * p - 1)
        for n in sorted(ns):
            want = oracle_tree(buf, n, L)
            for cap in (n, n + n // 2 + 3):
                t = Tree(gpu, buf, n, L, cap)
                import torch

                torch.cuda.synchronize()
                assert bytes(t.root.cpu().numpy()) == want[1], (L, n, cap)
                got = device_levels(t.lv, n, cap, L)
                assert len(got) == len(want[0])
                for d, (g, w) in enumerate(zip(got, want[0]), 1):
                    assert np.array_equal(g, w), (L, n, cap, d)


# ---- update in place ------------------------------------------------------------------------
def dirty_sets(n, p, rng):
    run0 = p * 101
    return [
        ("first", [0]),
        ("last, ragged chunk", [n - 1]),
        ("two of one chunk", [5 * p, 5 * p + 1]),
        ("both children of a level-1 node", [6 * p, 7 * p + 1]),
        ("each half of the root", [3, n - 2]),
        ("run of 5000 from an odd chunk", list(range(run0, min(run0 + 5000, n)))),
        ("1 % random", sorted(rng.choice(n, max(n // 100, 1), replace=False).tolist())),
        ("every item", list(range(n))),
        ("none", []),
    ]


@pytest.mark.parametrize("nch,L", [(1000, 32), ((1 << 16) + 3, 32), (1000, 8), ((1 << 16) + 3, 8)])
def test_update_in_place(gpu, nch, L):
    p = _per(L)
    n = nch * p - 1  # a ragged last chunk
    buf = _rand(n * L, 100 + L + nch)
    t = Tree(gpu, buf, n, L, n)
    check_tree(t, buf, "build")
    rng = np.random.default_rng(nch * L)
    step = 0
    for scatter in (True, False):
        for name, idx in dirty_sets(n, p, rng):
            step += 1
            vals = _rand(len(idx) * L, 1000 * step + L).reshape(-1, L)
            if idx:
                buf.reshape(n, L)[np.asarray(idx)] = vals
            t.update(idx, vals, scatter=scatter)
            check_tree(t, buf, f"{name}, scatter={scatter}")


# ---- append through update ------------------------------------------------------------------
def append_cases(p):
    return [
        ("chunk boundary", 4 * p + 2 if p > 1 else 5, 5 * p + 1),
        ("pair boundary", 6 * p - 1, 6 * p + 1),
        ("taller: 8 -> 9 chunks", 8 * p, 8 * p + 1),
        ("taller: 1024 -> 1027 chunks", 1024 * p, 1026 * p + 1),
        ("one chunk to two", max(p - 1, 1), p + 1),
        ("from 0 inside a chunk", 0, 1),
        ("from 0", 0, 5 * p + 1),
        ("from a ragged chunk", 10 * p + 1 if p > 1 else 11, 13 * p + 2),
    ]


@pytest.mark.parametrize("L", [32, 8, 200])
def test_append_through_update(gpu, L):
    p = _per(L)
    cap = 1100 * p
    buf0 = _rand(cap * L, 300 + L)
    for name, n_old, n_new in append_cases(p):
        for with_idx in (False, True):
            for scatter in (True, False):
                buf = buf0.copy()
                t = Tree(gpu, buf, n_old, L, cap)
                idx = sorted({0, n_old // 2, n_old - 1}) if with_idx and n_old else []
                vals = _rand((len(idx) + n_new - n_old) * L, 7 * n_new + L).reshape(-1, L)
                if idx:
                    buf.reshape(cap, L)[np.asarray(idx)] = vals[:len(idx)]
                buf.reshape(cap, L)[n_old:n_new] = vals[len(idx):]
                t.update(idx, vals, n_new=n_new, scatter=scatter)
                check_tree(t, buf, f"{name} idx={with_idx} scatter={scatter}")


# ---- a random sequence ----------------------------------------------------------------------
def test_random_sequence(gpu):
    import torch

    from oracle import oracle as O

    L, p = 32, 4
    cap = (1 << 15) * p
    n = 50_000
    buf = _rand(cap * L, 400)
    t = Tree(gpu, buf, n, L, cap)
    rng = np.random.default_rng(12345)
    for step in range(60):
        kind = step % 3  # update, append, both
        idx = sorted(rng.choice(n, int(rng.integers(1, 300)), replace=False).tolist()) if kind != 1 else []
        n_new = min(n + int(rng.integers(1, 2000)), cap) if kind != 0 else n
        vals = _rand((len(idx) + n_new - n) * L, 5000 + step).reshape(-1, L)
        if idx:
            buf.reshape(cap, L)[np.asarray(idx)] = vals[:len(idx)]
        buf.reshape(cap, L)[n:n_new] = vals[len(idx):]
        t.update(idx, vals, n_new=n_new, scatter=bool(step & 1))
        n = n_new
        torch.cuda.synchronize()
        assert bytes(t.root.cpu().numpy()) == O.merkle_hash_flat(buf[:n * L], n, L), step
    check_tree(t, buf, "after 60 steps")


# ---- two trees on two streams ---------------------------------------------------------------
def test_two_streams(gpu):
    import torch

    from prysm_amd import device as D

    L, p, steps, k = 32, 4, 30, 500
    n = (1 << 14) * p
    bufs = [_rand(n * L, 500 + i) for i in range(2)]
    trees = [Tree(gpu, bufs[i], n, L, n) for i in range(2)]
    rng = np.random.default_rng(77)
    work = []  # per step and tree: (d_idx, d_vals), uploaded before the streams start
    for s in range(steps):
        row = []
        for i in range(2):
            idx = np.sort(rng.choice(n, k, replace=False)).astype(np.int64)
            vals = _rand(k * L, 6000 + 2 * s + i).reshape(k, L)
            bufs[i].reshape(n, L)[idx] = vals
            row.append((torch.from_numpy(idx).to(gpu), torch.from_numpy(vals.reshape(-1)).to(gpu)))
        work.append(row)
    wss = [torch.empty(D.list_tree_update_workspace_bytes(k), dtype=torch.uint8, device=gpu) for _ in range(2)]
    streams = [torch.cuda.Stream(gpu) for _ in range(2)]
    torch.cuda.synchronize()
    for s in range(steps):
        for i in range(2):
            with torch.cuda.stream(streams[i]):
                tr = trees[i]
                D.list_tree_update(tr.items, n, n, n, L, tr.lv, tr.root, work[s][i][0], k, work[s][i][1], ws=wss[i])
    for i in range(2):
        check_tree(trees[i], bufs[i], f"tree {i}")


# ---- a replayed graph -----------------------------------------------------------------------
def test_graph_update(gpu):
    import torch

    from oracle import oracle as O
    from prysm_amd import device as D

    L, n, k = 32, 40_003, 64
    buf = _rand(n * L, 600)
    t = Tree(gpu, buf, n, L, n)
    d_idx = torch.zeros(k, dtype=torch.int64, device=gpu)
    d_vals = torch.zeros(k * L, dtype=torch.uint8, device=gpu)
    ws = torch.empty(D.list_tree_update_workspace_bytes(k), dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.list_tree_update(t.items, n, n, n, L, t.lv, t.root, d_idx, k, d_vals, ws=ws)
    rng = np.random.default_rng(5)
    for rep in range(5):
        idx = np.sort(rng.choice(n, k, replace=False)).astype(np.int64)
        vals = _rand(k * L, 700 + rep).reshape(k, L)
        buf.reshape(n, L)[idx] = vals
        d_idx.copy_(torch.from_numpy(idx))
        d_vals.copy_(torch.from_numpy(vals.reshape(-1)))
        g.replay()
        torch.cuda.synchronize()
        assert bytes(t.root.cpu().numpy()) == O.merkle_hash_flat(buf, n, L), rep
    check_tree(t, buf, "after 5 replays")


# ---- bad arguments --------------------------------------------------------------------------
def _raw_update(t, n_old, n_new, cap, L, d_idx, k, d_vals, ws):
    from prysm_amd import _lib

    call = _lib.Call(-1, 0, b"")
    p = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None  # noqa: E731
    rc = _lib.load().mk_dev_ssz_list_tree_update(ctypes.byref(call), p(t.items), n_old, n_new, cap, L, p(t.lv),
                                                 p(d_idx), k, p(d_vals), p(t.root), p(ws), ws.numel(), None)
    return rc, call


def test_bad_arguments(gpu):
    import torch

    from prysm_amd import _lib
    from prysm_amd import device as D

    L, n = 32, 999
    buf = _rand(n * L, 800)
    t = Tree(gpu, buf, n, L, n)
    ws = torch.empty(D.list_tree_update_workspace_bytes(8), dtype=torch.uint8, device=gpu)
    for args in ((n, n - 1, n, L), (n, n + 1, n, L), (n, n, n, 0)):
        rc, call = _raw_update(t, *args, None, 0, None, ws)
        assert rc == _lib.MK_EINVAL and call.code == rc and call.err != b"", args
    d_idx = torch.arange(0, 2 * 1000, 2, dtype=torch.int64, device=gpu)[:400]
    rc, call = _raw_update(t, n, n, n, L, d_idx, 400, None, ws)  # 400 work items, room for 32
    assert rc == _lib.MK_ENOMEM and call.err != b""
    check_tree(t, buf, "refused calls change nothing")


def test_out_of_range_index_is_ignored(gpu):
    L, n = 32, 4001
    buf = _rand(n * L, 900)
    t = Tree(gpu, buf, n, L, n + 100)
    vals = _rand(3 * L, 901).reshape(3, L)
    buf.reshape(n, L)[[5, 9]] = vals[:2]
    t.update([5, 9, n + 7], vals)  # item n + 7 lies inside the buffer's capacity: it must stay untouched
    check_tree(t, buf, "out-of-range index")
    import torch

    assert not torch.any(t.items[n * L:]), "bytes past the list were written"
