"""The resident deposit trie rolled back, compared, audited, cloned, copied and
grown on the device (mk_dev_deposit_trie_truncate / _fork_point / _audit /
_copy and the handle forms of prysm_amd.trieutil.DepositTrie).

Truth is the oracle: oracle.deposit_trie_levels (the level array of a deposit
sequence) and oracle.DictTrie (the literal restatement of deposit_trie.go,
through tests/trie_history_ref.Snapshots).  Nothing compares the library with
itself.  Dead nodes -- at or beyond a level's live count -- are filled with
0xFF before the calls, so a kernel that read one would compute a wrong node."""
import numpy as np
import pytest

from tests import trie_history_ref as H
from tests.guarded_arena import GuardedArena

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000000 + 0x7ADA
BIG = (1 << 17) + 3
NMAX = BIG + 8
DEP = 280
COUNTS6 = (1, 2, 3, 4, 5, 7, 8, 9, 31, 33, 63, 64)
COUNTS32 = (1, 2, 5, 1000, 1025)
CLEAN = (0, 0xFFFFFFFF, 2**64 - 1)
ROOT_LEVEL = 64


@pytest.fixture(autouse=True)
def _collect_handles():
    """A trie handle caught in a reference cycle (a frame kept by pytest.raises) is freed here, not by a
    collection in the middle of some later test's graph capture, where freeing device memory is an error."""
    yield
    import gc

    gc.collect()


@pytest.fixture(scope="module")
def gpu():
    import torch

    from prysm_amd import _lib

    assert torch.cuda.is_available()
    _lib.init(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def raw():
    """NMAX deposits of 280 bytes, and as many other ones."""
    from oracle import oracle as O

    return (np.array(O.splitmix_bytes(NMAX * DEP, SEED)), np.array(O.splitmix_bytes(NMAX * DEP, SEED + 1)))


def deps(buf, lo, hi):
    return [bytes(buf[DEP * i:DEP * (i + 1)]) for i in range(lo, hi)]


def cnt(c, d):
    return -(-c // (1 << d))


def off(cap, d):
    return sum(cnt(cap, i) for i in range(d))


def targets(count):
    """0, 1, every power of two below count, an odd value, count - 1 and count."""
    t = {0, 1, count - 1, count, (count // 2) | 1}
    p = 1
    while p < count:
        t.add(p)
        p *= 2
    return sorted(c for c in t if 0 <= c <= count)


_oracle = {}


def oracle_levels(key, seq, depth):
    """(root, [level d as an (n_d, 32) uint8 array]) of a deposit sequence; the small ones are computed once per key."""
    from oracle import oracle as O

    if key in _oracle:
        return _oracle[key]
    root, lv = O.deposit_trie_levels(seq, depth)
    res = (root, [np.frombuffer(b"".join(l), dtype=np.uint8).reshape(-1, 32) for l in lv] if seq else
           [np.zeros((0, 32), np.uint8)] * (depth + 1))
    if len(seq) <= 4096:  # the large ones are used once
        _oracle[key] = res
    return res


def live(host, cap, count, depth):
    """The live nodes of a downloaded level array, level by level."""
    return [host[32 * off(cap, d):32 * (off(cap, d) + cnt(count, d))].reshape(-1, 32) for d in range(depth + 1)]


def dead_mask(cap, count, depth):
    m = np.zeros(32 * off(cap, depth + 1), dtype=bool)
    for d in range(depth + 1):
        m[32 * (off(cap, d) + cnt(count, d)):32 * off(cap, d + 1)] = True
    return m


def branch_of(levels, index, depth):
    out = []
    for d in range(depth):
        s = (index >> d) ^ 1
        out.append(bytes(levels[d][s]) if s < len(levels[d]) else bytes(32))
    return b"".join(out)


class DevTrie:
    """A device-form trie inside a guarded arena."""

    def __init__(self, gpu, cap, depth, extra=0):
        from prysm_amd import device as D

        self.D, self.gpu, self.cap, self.depth, self.count = D, gpu, cap, depth, 0
        self.nbytes = D.deposit_trie_levels_bytes(cap, depth)
        self.arena = GuardedArena(gpu, [("levels", self.nbytes, 256, 0), ("root", 32, 256, 0), ("out", 64, 256, 0)])
        self.levels, self.root, self.out = (self.arena.view(n) for n in ("levels", "root", "out"))

    def append(self, buf, lo, hi):
        import torch

        if hi > lo:
            data = torch.from_numpy(buf[DEP * lo:DEP * hi]).to(self.gpu)
            self.D.deposit_trie_append(self.levels, self.cap, self.count, data, hi - lo, DEP, self.depth, self.root)
            self.count += hi - lo
        return self

    def poison_dead(self):
        import torch

        self.levels[torch.from_numpy(dead_mask(self.cap, self.count, self.depth)).to(self.gpu)] = 0xFF

    def host(self):
        return self.levels.cpu().numpy()

    def audit(self):
        return self.D.audit_reports(self.D.deposit_trie_audit(self.levels, self.cap, self.count, self.depth,
                                                              self.root))[0]

    def truncate(self, c):
        self.D.deposit_trie_truncate(self.levels, self.cap, self.count, c, self.depth, self.root)
        self.count = c

    def branches(self, as_of, idx):
        import torch

        t = torch.tensor(idx, dtype=torch.int64, device=self.gpu)
        root_at = torch.empty(32, dtype=torch.uint8, device=self.gpu)
        out = self.D.deposit_trie_branches(self.levels, self.cap, self.count, self.depth, as_of, t, root_at=root_at)
        return out.cpu().numpy().tobytes(), root_at.cpu().numpy().tobytes()


def check_rollback(gpu, raw, base, count, c, depth, k_new):
    """One roll back of a copy of `base` (count deposits) to c, then k_new other deposits appended."""
    import torch

    a, b = raw
    t = DevTrie(gpu, base.cap, depth)
    t.levels.copy_(base.levels)
    t.root.copy_(base.root)
    t.count = count
    t.poison_dead()
    before = t.host().copy()
    t.truncate(c)
    torch.cuda.synchronize()
    t.arena.check_guards(f"roll back {count} -> {c}: ")
    after = t.host()
    want_root, want = oracle_levels((depth, c), deps(a, 0, c), depth)
    for d, (g, w) in enumerate(zip(live(after, t.cap, c, depth), want)):
        assert np.array_equal(g, w), (count, c, d)
    assert t.root.cpu().numpy().tobytes() == want_root, (count, c)
    allowed = np.zeros(after.size, dtype=bool)
    if 0 < c < count:
        for d in range(1, depth + 1):
            if c % (1 << d):
                j = off(t.cap, d) + ((c - 1) >> d)
                allowed[32 * j:32 * j + 32] = True
    allowed[32 * off(t.cap, depth):32 * off(t.cap, depth) + 32] = True
    assert not ((before != after) & ~allowed).any(), (count, c)
    assert t.audit() == CLEAN, (count, c)
    # other deposits appended, then branches as of the new and of an older count, and the root
    k_new = min(k_new, (1 << depth) - c, t.cap - c)
    t.poison_dead()
    t.append(b, 0, k_new)
    n2 = c + k_new
    seq = deps(a, 0, c) + deps(b, 0, k_new)
    root2, lv2 = oracle_levels((depth, c, k_new), seq, depth)
    for d, (g, w) in enumerate(zip(live(t.host(), t.cap, n2, depth), lv2)):
        assert np.array_equal(g, w), (count, c, d, "after the append")
    assert t.root.cpu().numpy().tobytes() == (root2 if n2 else bytes(32))
    assert t.audit() == CLEAN, (count, c, "after the append")
    t.arena.check_guards(f"append after the roll back {count} -> {c}: ")
    if n2:
        idx = sorted({0, n2 - 1, n2 // 2, max(c - 1, 0), min(c, n2 - 1)})
        got, groot = t.branches(n2, idx)
        assert got == b"".join(branch_of(lv2, i, depth) for i in idx) and groot == root2, (count, c)
        old = max(c - 1, 1) if c else 1  # an older count: inside the kept deposits where there are any
        old = min(old, n2)
        rold, lold = oracle_levels((depth, c, k_new, old), seq[:old], depth)
        got, groot = t.branches(old, idx)
        assert got == b"".join(branch_of(lold, i, depth) for i in idx) and groot == rold, (count, c, old)


@pytest.fixture(scope="module")
def bases(gpu, raw):
    built = {}

    def get(depth, count, cap=None):
        key = (depth, count)
        if key not in built:
            built[key] = DevTrie(gpu, cap or min(count + 7, 1 << depth), depth).append(raw[0], 0, count)
        return built[key]

    return get


@pytest.mark.parametrize("count", COUNTS6)
def test_dev_rollback_depth6(gpu, raw, bases, count):
    base = bases(6, count)
    for c in targets(count):
        check_rollback(gpu, raw, base, count, c, 6, 5)


@pytest.mark.parametrize("count", COUNTS32)
def test_dev_rollback_depth32(gpu, raw, bases, count):
    base = bases(32, count)
    for c in targets(count):
        check_rollback(gpu, raw, base, count, c, 32, 5)


@pytest.mark.parametrize("part", range(8))
def test_dev_rollback_wide(gpu, raw, bases, part):
    """2^17 + 3 deposits at depth 32: the appends after a roll back take the batch front (c == 0), the wide
    one-launch-per-level form past 1020 changed nodes and the top launches past 2^17 nodes."""
    base = bases(32, BIG, BIG + 5)
    for c in targets(BIG)[part::8]:
        check_rollback(gpu, raw, base, BIG, c, 32, BIG - c if c <= 1 else 1500)


# ---- the handle ----------------------------------------------------------------------------------
def var_deposits(buf, n, salt=0):
    return [bytes(buf[320 * i:320 * i + 200 + 8 * ((i + salt) % 14) + (i % 7)]) for i in range(n)]


@pytest.fixture(scope="module")
def vdeps(raw):
    return var_deposits(raw[0], 1100), var_deposits(raw[1], 1100, 3)


def dict_trie(seq, depth):
    from oracle import oracle as O

    t = O.DictTrie(depth)
    for d in seq:
        t.update(d)
    return t


def handle(seq, depth=32, capacity=0):
    from prysm_amd import trieutil as T

    t = T.DepositTrie(depth, capacity=capacity)
    for d in seq:
        t.update_deposit_trie(d)
    return t


@pytest.mark.parametrize("depth,count", [(6, 33), (6, 64), (32, 5), (32, 1025)])
def test_handle_rollback(gpu, vdeps, depth, count):
    from oracle import oracle as O
    from prysm_amd import _lib

    a, b = vdeps
    for c in sorted({0, 1, count // 2 + 1, 1 << (count.bit_length() - 1), count - 1, count} - {-1}):
        t = handle(a[:count], depth)
        t.root()
        t.truncate(c)
        assert t.deposit_count == c
        m = dict_trie(a[:c], depth)
        assert t.root() == m.root(), (count, c)
        assert t.audit() == CLEAN, (count, c)
        idx = sorted({0, max(c - 1, 0), min(c, (1 << depth) - 1), c // 2})
        got = t.generate_merkle_branches(idx).tobytes()
        assert got == b"".join(b"".join(m.branch(i)) for i in idx), (count, c)
        if c:
            assert t.leaf(c - 1) == O.keccak256(a[c - 1]) and t.leaf(c) == bytes(32)
            older = H.Snapshots(a, [max(c // 2, 1)], depth)
            assert t.root_at(max(c // 2, 1)) == older.root(max(c // 2, 1)), (count, c)
        # save_logs of other deposits: log j carries the root before it; one wrong log in the middle is skipped
        k = min(6, (1 << depth) - c)
        logs, roots, want = b[:k], [], []
        for j, d in enumerate(logs):
            ok = j != 2
            roots.append(m.root() if ok else b"\x5a" * 32)
            want.append(ok)
            if ok:
                m.update(d)
        assert t.save_logs(logs, roots) == want, (count, c)
        assert t.root() == m.root() and t.deposit_count == m.count, (count, c)
        assert t.audit() == CLEAN, (count, c)
        assert t.root_at(c) == dict_trie(a[:c], depth).root() if c else True
    t = handle(a[:count], depth)
    r = t.root()
    with pytest.raises(_lib.MerkleError) as e:
        t.truncate(count + 1)
    assert e.value.code == _lib.MK_EINVAL
    with pytest.raises(_lib.MerkleError) as e:  # the C entry point itself, past the Python check
        _lib.invoke("mk_deposit_trie_truncate", t._handle, count + 1)
    assert e.value.code == _lib.MK_EINVAL
    assert t.root() == r and t.deposit_count == count


def test_dev_argument_checks(gpu):
    """Every refusal is MK_EINVAL before anything is launched: the buffers keep their bytes."""
    import torch

    from prysm_amd import _lib
    from prysm_amd import device as D

    lv = torch.full((D.deposit_trie_levels_bytes(200, 6) + 16,), 0x11, dtype=torch.uint8, device=gpu)
    root = torch.full((48,), 0x22, dtype=torch.uint8, device=gpu)
    rep = torch.full((40,), 0x33, dtype=torch.uint8, device=gpu)
    bad = [
        lambda: D.deposit_trie_truncate(lv, 16, 8, 9, 6, root),          # new_count > count
        lambda: D.deposit_trie_truncate(lv, 16, 17, 3, 6, root),         # count > capacity
        lambda: D.deposit_trie_truncate(lv, 200, 65, 3, 6, root),        # count > 2^depth
        lambda: D.deposit_trie_truncate(lv, 16, 8, 3, 0, root),          # depth 0
        lambda: D.deposit_trie_truncate(lv, 16, 8, 3, 64, root),         # depth 64
        lambda: D.deposit_trie_truncate(lv[8:], 16, 8, 3, 6, root),      # levels misaligned
        lambda: D.deposit_trie_truncate(lv, 16, 8, 3, 6, root[8:]),      # root misaligned
        lambda: D.deposit_trie_audit(lv, 16, 8, 6, root, rep[4:]),       # report misaligned
        lambda: D.deposit_trie_audit(lv, 16, 17, 6, root, rep),
        lambda: D.deposit_trie_fork_point(lv, 16, 8, lv, 16, 8, 6, rep[4:12]),
        lambda: D.deposit_trie_fork_point(lv, 16, 8, lv, 16, 17, 6),
        lambda: D.deposit_trie_copy(lv, 16, 8, lv, 16, 6, root, root[16:]),   # overlap
        lambda: D.deposit_trie_copy(lv, 16, 8, lv.clone(), 7, 6),             # dst_capacity < count
    ]
    for i, f in enumerate(bad):
        with pytest.raises(_lib.MerkleError) as e:
            f()
        assert e.value.code == _lib.MK_EINVAL, i
    torch.cuda.synchronize()
    assert bool((lv == 0x11).all()) and bool((root == 0x22).all()) and bool((rep == 0x33).all())


# ---- fork point ----------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,m", [(6, 33), (6, 64), (32, 1), (32, 1000), (32, 1025)])
def test_fork_point(gpu, vdeps, depth, m):
    a, b = vdeps
    A = handle(a[:m], depth)
    assert A.fork_point(A) == m
    assert A.fork_point(handle(a[:m], depth, capacity=3 * m + 11)) == m  # identical, another capacity
    for at in sorted({0, 1, m // 2, m - 1} & set(range(m))):
        seq = list(a[:m])
        seq[at] = b[at]
        B = handle(seq, depth, capacity=m + 100)
        assert A.fork_point(B) == at == B.fork_point(A), (m, at)
        if at < m - 1:  # a second difference further right: the smaller index
            seq[m - 1] = b[m - 1]
            assert A.fork_point(handle(seq, depth)) == at, (m, at)
    if m < (1 << depth):  # differences only at or beyond m
        longer = handle(list(a[:m]) + list(b[:3 if m + 3 <= (1 << depth) else 1]), depth)
        assert A.fork_point(longer) == m == longer.fork_point(A)
    empty = handle([], depth)
    assert A.fork_point(empty) == 0 == empty.fork_point(A)
    never = handle([], depth)
    never.reserve(8)  # a handle without deposits
    assert A.fork_point(never) == 0
    from prysm_amd import _lib

    with pytest.raises(_lib.MerkleError) as e:
        A.fork_point(handle(a[:1], depth + 1))
    assert e.value.code == _lib.MK_EINVAL


def test_fork_point_after_rollbacks_poisoned(gpu, raw):
    """Two device tries of different capacity, each rolled back and re-appended, dead nodes 0xFF."""
    import torch

    from prysm_amd import device as D

    a, b = raw
    for depth, n, ca, cb, ka, kb in ((6, 33, 20, 13, 9, 4), (32, 1025, 700, 513, 300, 100)):
        A = DevTrie(gpu, n + 9, depth).append(a, 0, n)
        B = DevTrie(gpu, 2 * n + 1, depth).append(a, 0, n)
        for t, c in ((A, ca), (B, cb)):
            t.poison_dead()
            t.truncate(c)
            t.poison_dead()
        A.append(b, 0, ka)                      # a[:ca] + b[:ka]
        B.append(a, cb, ca + 5).append(b, 5, 5 + kb)  # a[:ca + 5] + b[5:5 + kb]: parts at leaf ca
        A.poison_dead()
        B.poison_dead()
        out = D.deposit_trie_fork_point(A.levels, A.cap, A.count, B.levels, B.cap, B.count, depth)
        back = D.deposit_trie_fork_point(B.levels, B.cap, B.count, A.levels, A.cap, A.count, depth)
        torch.cuda.synchronize()
        la, lb = live(A.host(), A.cap, A.count, depth)[0], live(B.host(), B.cap, B.count, depth)[0]
        mm = min(len(la), len(lb))
        scan = next((i for i in range(mm) if not np.array_equal(la[i], lb[i])), mm)
        assert scan == ca and int(out.item()) == ca == int(back.item()), (depth, int(out.item()))
        assert A.audit() == CLEAN and B.audit() == CLEAN
        A.arena.check_guards()
        B.arena.check_guards()


# ---- clone / copy / reserve ----------------------------------------------------------------------
@pytest.mark.parametrize("depth,n", [(6, 33), (32, 1025)])
def test_clone_copy_reserve(gpu, vdeps, depth, n):
    from oracle import oracle as O
    from prysm_amd import _lib

    a, b = vdeps
    snaps = H.Snapshots(a, {n, n // 2 + 1, 1}, depth)
    src = handle(a[:n], depth)
    cl = src.clone()
    assert cl.deposit_count == n and cl.root() == snaps.root(n) and cl.audit() == CLEAN
    idx = [0, n - 1, n // 2]
    for c in (n, n // 2 + 1, 1):
        assert cl.generate_merkle_branches(idx, c).tobytes() == b"".join(snaps.branch(c, i) for i in idx), c
        assert cl.root_at(c) == snaps.root(c)
    k = min(4, (1 << depth) - n)
    if k == 0:
        cl.truncate(n - 4)
        k = 4
    for d in b[:k]:
        cl.update_deposit_trie(d)
    assert cl.root() == dict_trie(list(a[:cl.deposit_count - k]) + list(b[:k]), depth).root()
    assert src.root() == snaps.root(n) and src.deposit_count == n
    assert src.leaf(n - 1) == O.keccak256(a[n - 1]) and src.audit() == CLEAN
    # copy_from into a smaller handle (it grows) and into a larger one (it keeps its capacity)
    small, large = handle(b[:2], depth), handle(b[:3], depth, capacity=4 * n)
    large.root()
    cap_large = large.capacity
    for dst in (small, large):
        dst.copy_from(src)
        assert dst.deposit_count == n and dst.root() == snaps.root(n) and dst.audit() == CLEAN
        assert dst.generate_merkle_branches(idx, n // 2 + 1).tobytes() == \
            b"".join(snaps.branch(n // 2 + 1, i) for i in idx)
    assert small.capacity >= n and large.capacity == cap_large
    # reserve keeps the root; the next appends do not change the capacity
    t = handle(a[:n], depth)
    r = t.root()
    want_cap = min(3 * n + 5, 1 << depth)
    t.reserve(want_cap)
    assert t.capacity == want_cap and t.root() == r and t.audit() == CLEAN
    t.reserve(1)
    assert t.capacity == want_cap
    if n < (1 << depth):
        t.update_deposit_trie(b[0])
        assert t.root() == dict_trie(list(a[:n]) + [b[0]], depth).root() and t.capacity == want_cap
    with pytest.raises(_lib.MerkleError) as e:
        t.copy_from(handle(a[:2], depth + 1))
    assert e.value.code == _lib.MK_EINVAL
    assert t.audit() == CLEAN


def test_dev_copy_between_capacities(gpu, raw):
    import torch

    a, _b = raw
    for depth, n in ((6, 33), (32, 1025)):
        src = DevTrie(gpu, n + 9, depth).append(a, 0, n)
        src.poison_dead()
        for cap in (n, 2 * n + 3):
            dst = DevTrie(gpu, cap, depth)
            dst.levels.fill_(0xEE)
            src.D.deposit_trie_copy(src.levels, src.cap, n, dst.levels, cap, depth, src.root, dst.root)
            dst.count = n
            torch.cuda.synchronize()
            dst.arena.check_guards()
            _root, want = oracle_levels((depth, n), deps(a, 0, n), depth)
            host = dst.host()
            for d, (g, w) in enumerate(zip(live(host, cap, n, depth), want)):
                assert np.array_equal(g, w), (depth, cap, d)
            assert (host[dead_mask(cap, n, depth)] == 0xEE).all()
            assert torch.equal(dst.root, src.root) and dst.audit() == CLEAN


# ---- audit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,n", [(6, 33), (6, 64), (32, 5), (32, 1025)])
def test_audit_flips(gpu, raw, bases, depth, n):
    import torch

    base = bases(depth, n)
    t = DevTrie(gpu, base.cap, depth)
    t.levels.copy_(base.levels)
    t.root.copy_(base.root)
    t.count = n
    t.poison_dead()
    keep = t.levels.clone()
    assert t.audit() == CLEAN

    def flipped(d, j, byte=5):
        t.levels.copy_(keep)
        t.levels[32 * (off(t.cap, d) + j) + byte] ^= 0x40
        snap = t.levels.clone()
        rep = t.audit()
        assert torch.equal(t.levels, snap)  # read-only
        return rep

    for d in sorted({1, depth // 2, depth - 1}):
        j = cnt(n, d) - 1
        assert flipped(d, j) == (2, d, j), (d, j)
    if cnt(n, 2) > 2:  # two flips under different parents: the smallest key
        t.levels.copy_(keep)
        t.levels[32 * (off(t.cap, 2) + 1)] ^= 1
        t.levels[32 * (off(t.cap, 1) + cnt(n, 1) - 1)] ^= 1
        assert t.audit() == (4, 1, cnt(n, 1) - 1)
    assert flipped(0, n - 1) == (1, 1, (n - 1) >> 1)
    assert flipped(depth, 0) == (2, depth, 0)
    if cnt(n, 1) < cnt(t.cap, 1):
        assert flipped(1, cnt(n, 1)) == CLEAN  # a dead node
    t.levels.copy_(keep)
    t.root[7] ^= 0x08
    assert t.audit() == (1, ROOT_LEVEL, 0)
    t.arena.check_guards()


def test_audit_empty(gpu):
    t = DevTrie(gpu, 8, 6)
    t.root.fill_(0)
    assert t.audit() == CLEAN
    t.root[0] = 1
    assert t.audit() == (1, ROOT_LEVEL, 0)
    t.truncate(0)
    assert t.audit() == CLEAN and bool((t.root == 0).all())


# ---- capture -------------------------------------------------------------------------------------
def test_capture_truncate_audit_fork(gpu, raw, bases):
    """Truncate, audit and fork point in one graph on one stream (a linear chain), replayed twice."""
    import torch

    from prysm_amd import device as D

    depth, n, c = 32, 1025, 771
    base = bases(depth, n)
    other = DevTrie(gpu, n + 40, depth).append(raw[0], 0, 600).append(raw[1], 0, 300)
    t = DevTrie(gpu, base.cap, depth)
    report = torch.zeros(24, dtype=torch.uint8, device=gpu)
    fork = torch.zeros(1, dtype=torch.int64, device=gpu)

    def reset():
        t.levels.copy_(base.levels)
        t.root.fill_(0x77)
        report.fill_(0x33)
        fork.fill_(-1)

    def chain():
        D.deposit_trie_truncate(t.levels, t.cap, n, c, depth, t.root)
        D.deposit_trie_audit(t.levels, t.cap, c, depth, t.root, report)
        D.deposit_trie_fork_point(t.levels, t.cap, c, other.levels, other.cap, other.count, depth, fork)

    reset()
    chain()
    torch.cuda.synchronize()
    eager = (t.levels.clone(), t.root.clone(), D.audit_reports(report)[0], int(fork.item()))
    want_root, _lv = oracle_levels((depth, c), deps(raw[0], 0, c), depth)
    assert eager[1].cpu().numpy().tobytes() == want_root and eager[2] == CLEAN and eager[3] == 600
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        reset()
        with torch.cuda.graph(g, stream=s):
            chain()
    torch.cuda.synchronize()
    for rep in range(2):
        reset()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = (t.levels, t.root, D.audit_reports(report)[0], int(fork.item()))
        assert torch.equal(got[0], eager[0]) and torch.equal(got[1], eager[1]) and got[2:] == eager[2:], rep
