"""The rule of two resident trees' diff (include/prysm_merkle.h)
in plain Python over host copies of the trees' buffers: the indices below
m = min(n_a, n_b) whose leaf differs, found by walking down from the nodes of
level h0 = min(h, D_a, D_b) only through stored nodes that differ.  A node is
read only when it is comparable (it covers the same values in both trees); the
straddler of a level is descended without a look.  Every count comes from n_a
and n_b; a capacity only places its tree's levels.  `diff` returns the indices
(ascending) and the list of (level, index) nodes it read, in both trees each."""
import numpy as np

H = 10  # the kernel's subtree height (csrc/tree_diff.hpp kDiffHeight)


def per(len0):
    return 128 // len0 if len0 < 128 else 1


def chunks(n, len0):
    return -(-n // per(len0))


def depth(n, len0):
    c, d = chunks(n, len0), 0
    while c > 1:
        c, d = (c + 1) // 2, d + 1
    return d


def level_count(n, len0, d):
    return -(-chunks(n, len0) // (1 << d))


def level_off(capacity, len0, d):
    """First node of level d >= 1 in a level array laid out for `capacity` values."""
    cc, off = chunks(capacity, len0), 0
    for _ in range(1, d):
        cc = (cc + 1) // 2
        off += cc
    return off


def items(n_a, n_b, len0, h=H):
    """Work items of a pair: the visited nodes of level h0."""
    m = min(n_a, n_b)
    h0 = min(h, depth(n_a, len0), depth(n_b, len0))
    return -(-chunks(m, len0) // (1 << h0))


def diff(a, b, len0, h=H):
    """a, b: (leaves, levels, n, capacity) -- the leaf bytes (the items of a list
    tree, the 32-B roots / digests of the other kinds) and the level array laid
    out for `capacity` values."""
    (la, va, na, ca), (lb, vb, nb, cb) = a, b
    la, lb = (np.asarray(x, dtype=np.uint8).reshape(-1) for x in (la, lb))
    va, vb = (np.asarray(x, dtype=np.uint8).reshape(-1) for x in (va, vb))
    p, m = per(len0), min(na, nb)
    h0 = min(h, depth(na, len0), depth(nb, len0))
    reads, out = [], []

    def node(v, n, cap, d, j):
        assert j < level_count(n, len0, d), f"node ({d}, {j}) at or beyond the level's count"
        assert d <= depth(n, len0)
        o = 32 * (level_off(cap, len0, d) + j)
        return bytes(v[o:o + 32])

    def visited(d, j):
        return j * (1 << d) * p < m

    def comparable(d, j):
        return na == nb or (j + 1) * (1 << d) * p <= m

    def leaves(lo, hi):
        for i in range(lo, min(hi, m)):
            assert (i + 1) * len0 <= m * len0
            if bytes(la[i * len0:(i + 1) * len0]) != bytes(lb[i * len0:(i + 1) * len0]):
                out.append(i)

    def walk(d, j):
        if comparable(d, j):
            reads.append((d, j))
            if node(va, na, ca, d, j) == node(vb, nb, cb, d, j):
                return
        if d == 1:
            leaves(2 * j * p, (2 * j + 2) * p)
            return
        walk(d - 1, 2 * j)
        if visited(d - 1, 2 * j + 1):
            walk(d - 1, 2 * j + 1)

    if m == 0:
        return [], []
    if h0 == 0:
        leaves(0, p)
        return out, reads
    j = 0
    while visited(h0, j):
        walk(h0, j)
        j += 1
    assert j == items(na, nb, len0, h)
    return sorted(out), reads


def answer(a_leaves, b_leaves, n_a, n_b, len0):
    """[i < m : leaf_a[i] != leaf_b[i]]: no tree needed."""
    m = min(n_a, n_b)
    x = np.asarray(a_leaves, dtype=np.uint8).reshape(-1)[:m * len0].reshape(m, len0)
    y = np.asarray(b_leaves, dtype=np.uint8).reshape(-1)[:m * len0].reshape(m, len0)
    return [int(i) for i in np.flatnonzero((x != y).any(axis=1))]
