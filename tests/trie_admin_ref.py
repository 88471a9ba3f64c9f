"""The rules of the resident deposit trie's roll back, fork point and audit
(prysm_amd/csrc/trie_admin.hpp) restated in Python over a list
of levels: levels[d][j] is node j of level d, and a level may be LONGER than
its live count ceil(count / 2^d) -- what lies behind is dead, and ``Levels``
raises when a rule reads it.

Nothing here comes from the library: keccak is the oracle's, and the tests
compare with oracle.deposit_trie_levels / oracle.DictTrie."""
ZERO = bytes(32)
AUDIT_ROOT = 64


def cnt(c, d):
    return -(-c // (1 << d))


class Levels:
    """A level array with a live count; a read at or beyond a level's live count raises."""

    def __init__(self, levels, count, depth):
        self.lv = [list(l) for l in levels]
        while len(self.lv) <= depth:
            self.lv.append([])
        self.count, self.depth = count, depth
        self.written = set()

    def get(self, d, j):
        if not 0 <= j < cnt(self.count, d):
            raise AssertionError(f"dead node read: level {d} node {j}, {self.count} deposits")
        return self.lv[d][j]

    def put(self, d, j, v):
        while len(self.lv[d]) <= j:
            self.lv[d].append(ZERO)
        self.lv[d][j] = v
        self.written.add((d, j))

    def live(self):
        return [self.lv[d][:cnt(self.count, d)] for d in range(self.depth + 1)]


def straddlers(count, c, depth):
    """The nodes a roll back from count to c may write, besides level `depth` node 0 and the root."""
    if c == 0 or count <= c:
        return set()
    return {(d, (c - 1) >> d) for d in range(1, depth + 1) if c % (1 << d)}


def truncate(L, c, keccak):
    """Roll L back to its first c <= L.count deposits in place; returns the root."""
    count, depth = L.count, L.depth
    assert c <= count
    if c == 0:
        L.put(depth, 0, ZERO)
        L.count = 0
        return ZERO
    L.count = c  # every read below is of a node that is live in the trie of c deposits
    d0 = (c & -c).bit_length()  # ctz(c) + 1: the lowest straddling level
    if count == c or d0 > depth:
        return L.get(depth, 0)
    e = L.get(d0 - 1, (c - 1) >> (d0 - 1))
    for d in range(d0 - 1, depth):
        q = (c - 1) >> d
        e = keccak(L.get(d, q - 1) + e) if q & 1 else keccak(e + ZERO)
        L.put(d + 1, (c - 1) >> (d + 1), e)
    return e


def fork_point(A, B):
    """The smallest leaf index below min(count) at which A and B differ, else that minimum: compares only
    nodes (d, j) with (j + 1) 2^d <= m."""
    m = min(A.count, B.count)

    def ne(d, j):
        assert ((j + 1) << d) <= m, "a node that is not comparable was compared"
        return A.get(d, j) != B.get(d, j)

    for d in range(A.depth, -1, -1):
        if not (m >> d) & 1:
            continue
        j = (m >> d) - 1
        if not ne(d, j):
            continue
        while d > 0:
            d -= 1
            j = 2 * j if ne(d, 2 * j) else 2 * j + 1
        return j
    return m


def audit(L, root, keccak):
    """The keys (level, index) of every mismatch, ascending; the root's level is AUDIT_ROOT."""
    bad = []
    for d in range(1, L.depth + 1):
        for j in range(cnt(L.count, d)):
            right = L.get(d - 1, 2 * j + 1) if 2 * j + 1 < cnt(L.count, d - 1) else ZERO
            if keccak(L.get(d - 1, 2 * j) + right) != L.get(d, j):
                bad.append((d, j))
    if root != (L.get(L.depth, 0) if L.count else ZERO):
        bad.append((AUDIT_ROOT, 0))
    return bad


def append(L, leaves, keccak):
    """UpdateDepositTrie for each leaf hash, reading live nodes only (the right edge, as the library's append)."""
    for leaf in leaves:
        i = L.count
        L.count = i + 1
        L.put(0, i, leaf)
        for d in range(L.depth):
            q = i >> d
            left = L.get(d, q - 1) if q & 1 else L.get(d, q)
            right = L.get(d, q) if q & 1 else ZERO
            L.put(d + 1, q >> 1, keccak(left + right))
    return L.get(L.depth, 0) if L.count else ZERO
