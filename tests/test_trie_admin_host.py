"""The rules of the deposit trie's roll back, fork point and audit (DESIGN.md
§5p), as tests/trie_admin_ref.py restates them, against the oracle: the level
array oracle.deposit_trie_levels builds from the deposits (the restatement of
shared/trieutil/deposit_trie.go:29-63).  No GPU and no library code here: these
are the properties the kernels' rules must have, checked where a dead-node read
raises."""
import pytest

from oracle import oracle as O
from tests import trie_admin_ref as R

COUNTS6 = (1, 2, 3, 4, 5, 7, 8, 9, 31, 33, 63, 64)
COUNTS32 = (1, 2, 5, 1000, 1025, (1 << 17) + 3)
NMAX = (1 << 17) + 3 + 40
POISON = b"\xff" * 32


def targets(count):
    """0, 1, every power of two below count, an odd value, count - 1 and count."""
    t = {0, 1, count - 1, count, (count // 2) | 1}
    p = 1
    while p < count:
        t.add(p)
        p *= 2
    return sorted(c for c in t if 0 <= c <= count)


@pytest.fixture(scope="module")
def deposits():
    raw = O.splitmix_bytes(NMAX * 48, 0x5EED000000000000 + 0x7A1E)
    return [bytes(raw[48 * i:48 * i + 40 + i % 9]) for i in range(NMAX)]


@pytest.fixture(scope="module")
def others():
    raw = O.splitmix_bytes(64 * 48, 0x5EED000000000000 + 0x07E2)
    return [bytes(raw[48 * i:48 * i + 33 + i % 13]) for i in range(64)]


_built = {}


def built(deposits, n, depth):
    """(root, levels) of the first n deposits, computed once and never changed."""
    key = (n, depth)
    if key not in _built:
        _built[key] = O.deposit_trie_levels(deposits[:n], depth)
    return _built[key]


def poisoned(levels, count, depth, extra=3):
    """A Levels whose every level has `extra` dead nodes of 0xFF behind the live ones."""
    L = R.Levels(levels, count, depth)
    for d in range(depth + 1):
        L.lv[d] = L.lv[d][:R.cnt(count, d)] + [POISON] * extra
    return L


def check_rollback(deposits, others, count, c, depth, k_new):
    _root, levels = built(deposits, count, depth)
    want_root, want = built(deposits, c, depth)
    L = poisoned(levels, count, depth)
    before = [list(l) for l in L.lv]
    root = R.truncate(L, c, O.keccak256)
    assert root == want_root, (count, c)
    assert L.live() == ([l[:] for l in want] if c else [[] for _ in range(depth + 1)]), (count, c)
    # nothing outside the straddlers and level `depth` node 0 changed (the root is not part of the array)
    allowed = R.straddlers(count, c, depth) | {(depth, 0)}
    assert L.written <= allowed, (count, c, L.written - allowed)
    for d in range(depth + 1):
        for j, (x, y) in enumerate(zip(before[d], L.lv[d])):
            assert x == y or (d, j) in allowed, (count, c, d, j)
    assert R.audit(L, root, O.keccak256) == [], (count, c)
    # other deposits appended afterwards: the levels of the new sequence
    if c + k_new <= (1 << depth):
        new = others[:k_new]
        got_root = R.append(L, [O.keccak256(x) for x in new], O.keccak256)
        seq_root, seq = O.deposit_trie_levels(deposits[:c] + new, depth)
        assert got_root == seq_root and L.live() == seq, (count, c)


@pytest.mark.parametrize("count", COUNTS6)
def test_rollback_depth6(deposits, others, count):
    for c in targets(count):
        check_rollback(deposits, others, count, c, 6, min(5, 64 - c))


@pytest.mark.parametrize("count", COUNTS32)
def test_rollback_depth32(deposits, others, count):
    for c in targets(count):
        check_rollback(deposits, others, count, c, 32, 3)


def leaf_scan(a, b):
    m = min(len(a), len(b))
    return next((i for i in range(m) if a[i] != b[i]), m)


@pytest.mark.parametrize("depth,count", [(6, n) for n in COUNTS6] + [(32, n) for n in COUNTS32[:5]])
def test_fork_point(deposits, others, depth, count):
    _r, la = built(deposits, count, depth)
    A = poisoned(la, count, depth)
    assert R.fork_point(A, A) == count
    for nb in sorted({1, count // 2 + 1, count, min(count + 3, 1 << depth)}):
        for at in sorted({0, 1, nb // 2, nb - 1}):
            if at >= nb:
                continue
            for second in (None, nb - 1):
                seq = list(deposits[:nb])
                seq[at] = others[at % 64]
                if second is not None and second > at:
                    seq[second] = others[second % 64]
                _rb, lb = O.deposit_trie_levels(seq, depth)
                B = poisoned(lb, nb, depth)
                want = leaf_scan(la[0], lb[0])
                assert want == (at if at < min(count, nb) else min(count, nb))
                assert R.fork_point(A, B) == want == R.fork_point(B, A), (count, nb, at)
    E = R.Levels([], 0, depth)
    assert R.fork_point(A, E) == 0


def test_fork_point_after_rollbacks(deposits, others):
    """Two tries each rolled back and re-appended, dead nodes poisoned."""
    depth = 6
    _r, la = built(deposits, 33, depth)
    A, B = poisoned(la, 33, depth), poisoned(la, 33, depth)
    R.truncate(A, 20, O.keccak256)
    R.truncate(B, 13, O.keccak256)
    R.append(A, [O.keccak256(x) for x in others[:9]], O.keccak256)
    R.append(B, [O.keccak256(x) for x in deposits[13:18] + others[:4]], O.keccak256)
    assert R.fork_point(A, B) == 18 == leaf_scan(A.live()[0], B.live()[0])


@pytest.mark.parametrize("depth,count", [(6, n) for n in COUNTS6] + [(32, n) for n in (1, 2, 5, 1000, 1025)])
def test_audit_reports_the_flipped_nodes(deposits, depth, count):
    root, levels = built(deposits, count, depth)
    assert R.audit(poisoned(levels, count, depth), root, O.keccak256) == []

    def flipped(d, j):
        L = poisoned(levels, count, depth)
        v = bytearray(L.lv[d][j])
        v[(7 * d + j) % 32] ^= 0x10
        L.lv[d][j] = bytes(v)
        return L

    # a leaf: its parent only; an interior node: itself and its parent; the top: itself and the root
    assert R.audit(flipped(0, count - 1), root, O.keccak256) == [(1, (count - 1) >> 1)]
    for d in sorted({1, depth // 2, depth - 1}):
        j = R.cnt(count, d) - 1
        assert R.audit(flipped(d, j), root, O.keccak256) == [(d, j), (d + 1, j >> 1)], (d, j)
    assert R.audit(flipped(depth, 0), root, O.keccak256) == [(depth, 0), (R.AUDIT_ROOT, 0)]
    # a dead node: clean; the root alone: the root key
    assert R.audit(flipped(1, R.cnt(count, 1)), root, O.keccak256) == []
    assert R.audit(poisoned(levels, count, depth), bytes(31) + b"\x01", O.keccak256) == [(R.AUDIT_ROOT, 0)]


def test_empty_trie():
    L = R.Levels([], 0, 6)
    assert R.audit(L, R.ZERO, O.keccak256) == []
    assert R.audit(L, POISON, O.keccak256) == [(R.AUDIT_ROOT, 0)]
    assert R.truncate(L, 0, O.keccak256) == R.ZERO
