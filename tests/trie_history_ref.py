"""A small model of the deposit trie's as-of rule, the
algorithm k_trie_branches_at implements, over the FINAL level array of a trie
of `count` deposits (levels[d][j]: node j of level d, oracle.deposit_trie_levels).

As of deposit count c <= count: a node whose leaves all lie below c still has
the value it had then; a node whose leaves all lie at or above c did not exist
(0^32); per level only the ancestor of leaf c - 1 can straddle c, and those
straddling nodes E_d form one chain of hashes over final left siblings.

Also the shared oracle side of the GPU tests: DictTrie snapshots by count."""
ZERO = bytes(32)


def edge_chain(levels, count, c, depth, keccak):
    """E_0 .. E_depth: the ancestors of leaf c - 1 as of c deposits."""
    if c == 0:
        return [ZERO] * (depth + 1)
    last = c - 1
    edge = []
    for d in range(depth + 1):
        if count > c and c % (1 << d):  # level d's node holds leaves on both sides of c
            p = last >> (d - 1)
            below = edge[d - 1]
            edge.append(keccak(levels[d - 1][p - 1] + below) if p & 1 else keccak(below + ZERO))
        else:
            edge.append(levels[d][last >> d])
    return edge


def branch_at(levels, edge, c, index, depth):
    out = []
    for d in range(depth):
        s = (index >> d) ^ 1
        if (s << d) >= c:
            out.append(ZERO)
        elif s == (c - 1) >> d:
            out.append(edge[d])
        else:
            out.append(levels[d][s])
    return out


def root_at(edge, c, depth):
    return edge[depth] if c else ZERO


class Snapshots:
    """oracle.DictTrie run over `deposits`, its map kept at every count in
    `counts`: branch(c, i) and root(c) are what the reference's trie answered
    right after its c-th UpdateDepositTrie."""

    def __init__(self, deposits, counts, depth):
        from oracle import oracle as O

        self.depth = depth
        self._maps = {}
        self._cache = {}
        counts = set(counts)
        t = O.DictTrie(depth)
        if 0 in counts:
            self._maps[0] = {}
        for j, d in enumerate(deposits):
            if not any(c > j for c in counts):
                break
            t.update(d)
            if j + 1 in counts:
                self._maps[j + 1] = dict(t.m)

    def _trie(self, c):
        from oracle import oracle as O

        t = O.DictTrie(self.depth)
        t.m, t.count = self._maps[c], c
        return t

    def root(self, c):
        return self._trie(c).root()

    def branch(self, c, index):
        """DictTrie.branch(index) at count c, the depth siblings joined."""
        key = (c, index)
        if key not in self._cache:
            self._cache[key] = b"".join(self._trie(c).branch(index))
        return self._cache[key]
