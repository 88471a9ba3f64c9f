"""Batched Merkle branches and roots of the resident deposit trie AS OF a past
deposit count (k_trie_branches_at: mk_deposit_trie_branches,
mk_deposit_trie_root_at, mk_dev_deposit_trie_branches).

Every expected value comes from oracle.DictTrie, the literal restatement of
deposit_trie.go: run to count c, .branch(i) and .root() are what the
reference's trie answered at that moment (tests/trie_history_ref.Snapshots
keeps its map at the counts a test asks about)."""
import ctypes

import numpy as np
import pytest

from tests import trie_history_ref as H

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000000 + 0xB7A
NMAX = 4400  # the life-cycle test's trie; every other test uses a prefix


@pytest.fixture(scope="module")
def gpu():
    import torch

    from prysm_amd import _lib

    assert torch.cuda.is_available()
    _lib.init(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def deposits():
    from oracle import oracle as O

    raw = O.splitmix_bytes(NMAX * 320, SEED)
    return [bytes(raw[320 * i:320 * i + 200 + 8 * (i % 14) + (i % 7)]) for i in range(NMAX)]


def _pow2_floor(n):
    return 1 << (n.bit_length() - 1)


def _counts(n):
    p = _pow2_floor(n)
    return sorted({c for c in (0, 1, 2, n - 1, n, n // 2 + 1, p, p + 1) if 0 <= c <= n})


NS32 = (1, 2, 3, 5, 8, 9, 64, 65, 1000, 1025)


@pytest.fixture(scope="module")
def snaps32(deposits):
    """DictTrie at depth 32 over the shared deposits, kept at every count the tests below ask about."""
    want = {c for n in NS32 for c in _counts(n)} | set(LIFE_COUNTS) | {65, 1025}
    return H.Snapshots(deposits, want, 32)


LIFE_POINTS = (1000, 2100, 4300)  # capacity 1024 -> 2100 -> 4300: two growths
LIFE_COUNTS = (1, 513, 999, 1000, 1025, 2047, 2099, 2100, 2101, 4096, 4299, 4300)


def _trie(deposits, n, depth=32, capacity=0):
    from prysm_amd import trieutil as T

    t = T.DepositTrie(depth, capacity=capacity)
    for d in deposits[:n]:
        t.update_deposit_trie(d)
    return t


def _indices(n, c, depth, rng, extra=24):
    top = (1 << depth) - 1
    special = [c - 1, c, c + 1, top, 0, n - 1, n, c - 1, top]
    rnd = list(rng.integers(0, min(top, n + 3) + 1, size=extra))
    idx = [int(i) for i in special + rnd if 0 <= i <= top]
    rng.shuffle(idx)
    return idx


def _expect(snaps, c, idx, depth):
    return np.frombuffer(b"".join(snaps.branch(c, i) for i in idx), dtype=np.uint8).reshape(len(idx), depth, 32)


def test_exhaustive_depth6(gpu, deposits):
    """n = 33 at depth 6: every count 0..33, all indices 0..35 in one call each."""
    n, depth = 33, 6
    snaps = H.Snapshots(deposits, range(n + 1), depth)
    t = _trie(deposits, n, depth)
    idx = list(range(36))
    for c in range(n + 1):
        got = t.generate_merkle_branches(idx, c)
        assert got.shape == (36, depth, 32)
        assert np.array_equal(got, _expect(snaps, c, idx, depth)), c
        assert t.root_at(c) == snaps.root(c), c
        assert t.generate_merkle_branch(c, c) == [snaps.branch(c, c)[32 * d:32 * d + 32] for d in range(depth)]


@pytest.mark.parametrize("n", NS32)
def test_depth32(gpu, deposits, snaps32, n):
    """Unsorted indices with repeats, among them c - 1, c, c + 1 and 2^32 - 1."""
    rng = np.random.default_rng(n)
    t = _trie(deposits, n)
    for c in _counts(n):
        idx = _indices(n, c, 32, rng)
        got = t.generate_merkle_branches(idx, c)
        assert np.array_equal(got, _expect(snaps32, c, idx, 32)), (n, c)
        assert t.root_at(c) == snaps32.root(c), (n, c)
    assert t.root_at() == t.root() == snaps32.root(n)


def test_many_indices_grid_stride(gpu, deposits, snaps32):
    """k = 3000 at n = 1025: 750 workgroups of four waves."""
    n, rng = 1025, np.random.default_rng(3000)
    t = _trie(deposits, n)
    for c in (513, 1024):
        idx = [int(i) for i in rng.integers(0, 1100, size=2990)] + [c - 1, c, c + 1, (1 << 32) - 1, 0] * 2
        rng.shuffle(idx)
        assert len(idx) == 3000
        assert np.array_equal(t.generate_merkle_branches(idx, c), _expect(snaps32, c, idx, 32)), c


def test_chunked_handle_call(gpu, deposits, snaps32):
    """More indices than one chunk of the handle's scratch (8192): two launches, two read-backs."""
    n, c = 65, 33
    t = _trie(deposits, n)
    base = list(range(68)) + [(1 << 32) - 1]
    idx = (base * 130)[:8192 + 300]
    got = t.generate_merkle_branches(idx, c)
    want = {i: np.frombuffer(snaps32.branch(c, i), dtype=np.uint8).reshape(32, 32) for i in base}
    for j in (0, 1, 67, 68, 8191, 8192, 8193, len(idx) - 1):
        assert np.array_equal(got[j], want[idx[j]]), j
    pos = {i: np.array([j for j, v in enumerate(idx) if v == i]) for i in base}
    for i in base:
        assert (got[pos[i]] == want[i]).all(), i


def _check_past(t, snaps, counts, n, rng):
    for c in counts:
        idx = _indices(n, c, 32, rng, extra=8)
        assert np.array_equal(t.generate_merkle_branches(idx, c), _expect(snaps, c, idx, 32)), (n, c)
        assert t.root_at(c) == snaps.root(c), (n, c)


def test_handle_growth(gpu, deposits, snaps32):
    """Created with capacity 4 (the library's floor is 1024) and appended past
    two growths of the level array; three past counts at each point."""
    from prysm_amd import trieutil as T

    rng = np.random.default_rng(4)
    t = T.DepositTrie(32, capacity=4)
    done = 0
    for n in LIFE_POINTS:
        for d in deposits[done:n]:
            t.update_deposit_trie(d)
        done = n
        past = [c for c in LIFE_COUNTS if c <= n][-4:]
        _check_past(t, snaps32, past[:3] + [n], n, rng)
        assert t.root() == snaps32.root(n)


def test_after_save_logs_with_skips(gpu, deposits):
    """A save_logs batch in which some logs carry a wrong root and are skipped
    (the trie was cut back and its right edge recomputed)."""
    from oracle import oracle as O
    from prysm_amd import trieutil as T

    rng = np.random.default_rng(5)
    ref = O.DictTrie(32)
    t = T.DepositTrie(32)
    kept, roots, want = [], [], []
    for d in deposits[:20]:
        ref.update(d)
        kept.append(d)
        t.update_deposit_trie(d)
    batch = deposits[20:60]
    for j, d in enumerate(batch):
        if j in (3, 4, 17, 39):
            roots.append(bytes(32 - 1) + b"\x01")
            want.append(False)
            continue
        roots.append(ref.root())
        want.append(True)
        ref.update(d)
        kept.append(d)
    assert t.save_logs(batch, roots) == want
    n = len(kept)
    assert n == 56 and t.deposit_count == n
    snaps = H.Snapshots(kept, [19, 23, 40, n], 32)
    _check_past(t, snaps, [19, 23, 40, n], n, rng)


def test_after_mixed_appends(gpu, deposits):
    """Single appends (each flushed by a Root() read) between batched ones."""
    rng = np.random.default_rng(6)
    from prysm_amd import trieutil as T

    t = T.DepositTrie(32)
    n = 0
    for step in (1, 1, 30, 1, 200, 1, 1, 17):
        for d in deposits[n:n + step]:
            t.update_deposit_trie(d)
        n += step
        t.root()
    snaps = H.Snapshots(deposits, [2, 33, 233, n], 32)
    _check_past(t, snaps, [2, 33, 233, n], n, rng)


def test_closure_with_the_existing_verifier(gpu, deposits, snaps32):
    """Every produced branch passes the existing verify_merkle_branches against
    root_at(c); root_at(count) is Root(); a branch as of c < count does not
    verify against Root() when the two roots differ."""
    from prysm_amd import trieutil as T

    n = 65
    t = _trie(deposits, n)
    assert t.root_at(n) == t.root()
    leaves = [t.leaf(i) for i in range(n)]
    for c in (1, 33, 64, 65):
        idx = list(range(c))
        br = t.generate_merkle_branches(idx, c)
        root_c = t.root_at(c)
        lists = [[bytes(br[j, d]) for d in range(32)] for j in range(c)]
        assert all(T.verify_merkle_branches(leaves[:c], lists, 32, idx, [root_c] * c))
        if root_c != t.root():
            assert not any(T.verify_merkle_branches(leaves[:c], lists, 32, idx, [t.root()] * c))
    assert t.root_at(64) != t.root()


def test_single_form_unchanged(gpu, deposits):
    n = 65
    t = _trie(deposits, n)
    for i in range(n + 3):
        one = t.generate_merkle_branch(i)
        assert b"".join(one) == t.generate_merkle_branches([i])[0].tobytes(), i
        assert one == t.generate_merkle_branch(i, n)


def test_empty_trie_and_errors(gpu, deposits):
    from prysm_amd import _lib
    from prysm_amd import trieutil as T

    e = T.DepositTrie(32)
    assert not e.generate_merkle_branches([0, 5]).any() and e.root_at() == bytes(32) and e.root_at(0) == bytes(32)
    with pytest.raises(_lib.MerkleError):
        e.root_at(1)
    t = _trie(deposits, 9)
    out = np.full((2, 32, 32), 0xA5, dtype=np.uint8)
    with pytest.raises(_lib.MerkleError) as ei:
        t.generate_merkle_branches([0, 1], 10, out=out)
    assert ei.value.code == _lib.MK_EINVAL and (out == 0xA5).all()
    # the library's own check, under the Python one
    idx = np.array([0, 1], dtype=np.uint64)
    root = ctypes.create_string_buffer(b"\xa5" * 32, 32)
    call = _lib.Call(-1, 0, b"")
    rc = _lib.load().mk_deposit_trie_branches(ctypes.byref(call), t._handle, 10, idx.ctypes.data_as(ctypes.c_void_p), 2,
                                              out.ctypes.data_as(ctypes.c_void_p), root)
    assert rc == _lib.MK_EINVAL and b"as_of" in call.err and (out == 0xA5).all() and root.raw == b"\xa5" * 32
    rc = _lib.load().mk_deposit_trie_root_at(ctypes.byref(call), t._handle, 10, root)
    assert rc == _lib.MK_EINVAL and root.raw == b"\xa5" * 32
    # k == 0: accepted, only the root is written
    assert t.generate_merkle_branches([], 4).shape == (0, 32, 32)
    rc = _lib.load().mk_deposit_trie_branches(ctypes.byref(call), t._handle, 4, None, 0, None, root)
    assert rc == 0 and root.raw == t.root_at(4) and (out == 0xA5).all()
    assert out is t.generate_merkle_branches([3, 8], 9, out=out) and out.tobytes() == b"".join(
        b"".join(t.generate_merkle_branch(i)) for i in (3, 8))


def test_device_form_in_a_graph(gpu, deposits, snaps32):
    """mk_dev_deposit_trie_branches twice in one captured stream (a linear
    chain), replayed; the indices tensor is rewritten between replays and the
    results follow it.  An out-of-range as_of launches nothing."""
    import torch

    from prysm_amd import _lib
    from prysm_amd import device as D

    n, depth, cap = 65, 32, 100
    data, offs = [], [0]
    for d in deposits[:n]:
        data.append(d)
        offs.append(offs[-1] + len(d))
    blob = torch.from_numpy(np.frombuffer(b"".join(data), dtype=np.uint8).copy()).to(gpu)
    d_offs = torch.tensor(offs, dtype=torch.int64, device=gpu)
    lv = torch.zeros(D.deposit_trie_levels_bytes(cap, depth), dtype=torch.uint8, device=gpu)
    root = torch.zeros(32, dtype=torch.uint8, device=gpu)
    D.deposit_trie_append(lv, cap, 0, blob, n, 0, depth, root, offs=d_offs)
    k = 7
    idx = torch.zeros(k, dtype=torch.int64, device=gpu)
    out_a = torch.zeros(k * depth * 32, dtype=torch.uint8, device=gpu)
    out_b = torch.zeros(k * depth * 32, dtype=torch.uint8, device=gpu)
    root_a = torch.zeros(32, dtype=torch.uint8, device=gpu)
    root_b = torch.zeros(32, dtype=torch.uint8, device=gpu)

    def body():
        D.deposit_trie_branches(lv, cap, n, depth, 33, idx, out=out_a, root_at=root_a)
        D.deposit_trie_branches(lv, cap, n, depth, 65, idx, out=out_b, root_at=root_b)

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    for pick in ([0, 32, 33, 34, 64, 66, 5], [31, 31, 2, 65, 1, 0, (1 << 32) - 1]):
        idx.copy_(torch.tensor(pick, dtype=torch.int64))
        out_a.zero_()
        out_b.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out_a.cpu().numpy().reshape(k, depth, 32), _expect(snaps32, 33, pick, depth)), pick
        assert np.array_equal(out_b.cpu().numpy().reshape(k, depth, 32), _expect(snaps32, 65, pick, depth)), pick
        assert bytes(root_a.cpu().numpy()) == snaps32.root(33) and bytes(root_b.cpu().numpy()) == snaps32.root(65)
    out_a.fill_(0xA5)
    with pytest.raises(_lib.MerkleError) as ei:
        D.deposit_trie_branches(lv, cap, n, depth, n + 1, idx, out=out_a)
    torch.cuda.synchronize()
    assert ei.value.code == _lib.MK_EINVAL and bool((out_a == 0xA5).all())
