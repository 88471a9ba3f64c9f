"""Host side of the resident trees' diff: the plain-Python model
of the rule (tests/tree_diff_ref.py) over the oracle's trees against the answer
that needs no tree -- [i < m : leaf_a[i] != leaf_b[i]] -- on every pair of
counts, the nodes it reads, the zero-pad collision, and every argument error of
mk_dev_ssz_trees_diff and of the handle forms, decided before a device is
looked up (the pointers are made-up addresses that are only ever compared)."""
import ctypes
import os

import numpy as np
import pytest

from prysm_amd import _lib
from tests import tree_diff_ref as R
from tests.test_gpu_list_tree import oracle_tree

P = 0x7F0000001000  # a 4096-B aligned address that is never dereferenced
MB = 1 << 20
LIST, STRUCT, BYTES = _lib.MK_TREE_LIST, _lib.MK_TREE_STRUCT, _lib.MK_TREE_BYTES
SEED = 0x5EED000000000000 + 2700
LENS = [1, 8, 32, 48, 100, 128]
SMALL = list(range(41))
MORE = [63, 64, 65, 127, 129, 257]
FILL = 0xA5


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def rand(nbytes, salt):
    from oracle import oracle as O

    return O.splitmix_bytes((nbytes + 7) // 8 * 8 + 8, SEED + salt)[:nbytes].copy()


def host_tree(data, n, cap, L):
    """(leaves, level array laid out for cap, n, cap) of the oracle's tree of the first n items of `data`;
    every byte the tree does not own is FILL."""
    leaves = np.full(cap * L + 16, FILL, dtype=np.uint8)
    leaves[:n * L] = data[:n * L]
    levels, _root = oracle_tree(leaves, n, L)
    total = R.level_off(cap, L, R.depth(cap, L) + 1) if cap else 0
    lv = np.full(32 * max(total, 1), FILL, dtype=np.uint8)
    for d, nodes in enumerate(levels, 1):
        off = R.level_off(cap, L, d)
        assert len(nodes) == R.level_count(n, L, d)
        lv[32 * off:32 * (off + len(nodes))] = nodes.reshape(-1)
    return leaves, lv, n, cap


class Trees:
    """The trees of x[:n] and of y[:n] (y: x with some items changed) for one item length, built once."""

    def __init__(self, L):
        self.L = L
        top = max(MORE) + 8
        self.x = rand(top * L, 17 * L)
        self.y = self.x.copy()
        rng = np.random.default_rng(L)
        for i in np.flatnonzero(rng.random(top) < 0.12):
            self.y[i * L + int(rng.integers(L))] ^= 1 << int(rng.integers(8))
        self._made = {}

    def tree(self, which, n, cap=None):
        cap = 2 * n + 3 if cap is None else cap
        key = (which, n, cap)
        if key not in self._made:
            self._made[key] = host_tree(self.x if which == "x" else self.y, n, cap, self.L)
        return self._made[key]


_trees = {}


def trees(L):
    if L not in _trees:
        _trees[L] = Trees(L)
    return _trees[L]


def check_pair(T, na, nb, h, other="y"):
    a, b = T.tree("x", na, na + 1), T.tree(other, nb)
    got, reads = R.diff(a, b, T.L, h)
    want = R.answer(a[0], b[0], na, nb, T.L)
    assert got == want, (T.L, na, nb, h, other)
    # never a node at or beyond a level's count, in either tree, nor a level above min(D_a, D_b)
    for d, j in reads:
        assert j < R.level_count(na, T.L, d) and j < R.level_count(nb, T.L, d), (T.L, na, nb, d, j)
        assert d <= min(R.depth(na, T.L), R.depth(nb, T.L))
    assert len(set(reads)) == len(reads)
    return got, reads


@pytest.mark.parametrize("L", LENS)
def test_model_against_the_leafwise_answer(L):
    T = trees(L)
    for na in SMALL:
        for nb in SMALL:
            check_pair(T, na, nb, R.H)
            check_pair(T, na, nb, R.H, other="x")  # nothing differs: only the straddlers are descended
    for na in MORE:
        for nb in (na, na + 1, MORE[0], 5):
            for h in (R.H, 2):
                check_pair(T, na, nb, h)
                check_pair(T, nb, na, h)
    # equal trees of equal length: one read per work item and nothing else
    for n in (40, 257):
        got, reads = check_pair(T, n, n, 2, other="x")
        h0 = min(2, R.depth(n, L))  # a list of one chunk has no node to read
        assert got == [] and len(reads) == (R.items(n, n, L, 2) if h0 else 0) and all(d == h0 for d, _ in reads)


def test_zero_pad_collision():
    """With the 128-zero-byte odd pad, K(c || 0^128) is both 'chunk c was the last' and 'chunk c is followed by
    an all-zero chunk': the straddling level-1 node of the longer tree is byte-equal to the shorter tree's, and
    the rule never looks at it.  s = 32 (p = 4, a chunk is 128 bytes)."""
    L = 32
    x = rand(64 * L, 99)
    zeros = np.zeros(16 * L, dtype=np.uint8)

    def pair(k, extra):
        a = host_tree(x, k, k + 3, L)
        b = host_tree(np.concatenate([x[:k * L], zeros]), k + extra, 2 * k + 9, L)
        return a, b

    def node(t, d, j):
        o = 32 * (R.level_off(t[3], L, d) + j)
        return bytes(t[1][o:o + 32])

    # 4 items against the same 4 and four zero items: the shorter tree has no level at all, so no node of the
    # longer one is read and the four values are compared directly
    a, b = pair(4, 4)
    assert R.diff(a, b, L) == ([], [])
    # one level up, 8 items against 8 + 8 zeros: node (1, 0) covers values [0, 8) in both trees, is comparable,
    # equal, and ends the descent; node (1, 1) of the longer tree covers nothing below m and is not visited
    a, b = pair(8, 8)
    assert node(a, 1, 0) == node(b, 1, 0)
    assert R.diff(a, b, L) == ([], [(1, 0)])
    # the collision itself: 12 items (3 chunks) against 12 + 4 zeros.  Node (1, 1) is K(c2 || 0^128) in both
    # trees -- the pad in one, a chunk of zero items in the other -- and covers [8, 16) against m = 12: not
    # comparable, so it is descended, never read, and values 8 .. 11 are compared leaf by leaf
    a, b = pair(12, 4)
    assert node(a, 1, 1) == node(b, 1, 1)
    got, reads = R.diff(a, b, L)
    assert got == [] and (1, 1) not in reads and reads == [(1, 0)]
    # and with a value under the straddler changed, it is found although its node was never compared
    y = x.copy()
    y[10 * L + 7] ^= 0x20
    b = host_tree(np.concatenate([y[:12 * L], zeros]), 16, 40, L)
    got, reads = R.diff(a, b, L)
    assert got == [10] and (1, 1) not in reads
    # a longer pair: 20 items (5 chunks) against 20 + 4 zeros; the straddlers are (1, 2), (2, 1) and (3, 0)
    a, b = pair(20, 4)
    assert node(a, 1, 2) == node(b, 1, 2)
    got, reads = R.diff(a, b, L)
    assert got == [] and set(reads) == {(2, 0)}


def test_a_straddler_that_hides_nothing():
    """n_a = 6, n_b = 8 (s = 32: two chunks each), item 5 changed: node (1, 0) covers [0, 8) against m = 6."""
    L = 32
    x = rand(8 * L, 7)
    y = x.copy()
    y[5 * L + 31] ^= 1
    a, b = host_tree(x, 6, 6, L), host_tree(y, 8, 19, L)
    assert R.diff(a, b, L) == ([5], [])
    assert R.diff(b, a, L) == ([5], [])
    a = host_tree(x, 8, 8, L)
    assert R.diff(a, b, L) == ([5], [(1, 0)])


# ---- the device entry's refusals, without a device ---------------------------------------------------
def pair(kind=BYTES, item_len=32, n_a=257, capacity_a=260, n_b=300, capacity_b=300, base=P, max_out=64, **ptrs):
    t = _lib.TreeDiff()
    t.kind, t.item_len = kind, item_len
    t.n_a, t.capacity_a, t.n_b, t.capacity_b = n_a, capacity_a, n_b, capacity_b
    names = ("d_a_items", "d_a_level0", "d_a_levels", "d_b_items", "d_b_level0", "d_b_levels", "d_idx_out")
    for i, name in enumerate(names):
        v = base + 2 * i * MB
        if kind == LIST and name.endswith("level0"):
            v = None
        setattr(t, name, ptrs.get(name, v))
    t.max_out = max_out
    return t


REP = P + 400 * MB


def diff(lib, pairs, reports=REP, ntrees=None):
    arr = (_lib.TreeDiff * max(len(pairs), 1))(*pairs)
    call = _lib.Call(-1, 0, b"")
    rc = lib.mk_dev_ssz_trees_diff(ctypes.byref(call), arr, len(pairs) if ntrees is None else ntrees,
                                   ctypes.c_void_p(reports), None)
    assert call.code == rc
    return rc, call.err


def test_every_refusal_needs_no_device(lib):
    levels_a = P + 4 * MB  # pair()'s d_a_levels
    bad = [
        ("no pairs", b"0 tree pairs", [], {}),
        ("17 pairs", b"17 tree pairs", [pair(base=P + 16 * i * MB) for i in range(17)], {}),
        ("an unknown kind", b"unknown kind", [pair(kind=0)], {}),
        ("another unknown kind", b"unknown kind", [pair(kind=4)], {}),
        ("item_len == 0", b"item_len == 0", [pair(LIST, 0)], {}),
        ("a list item above 128", b"above 128", [pair(LIST, 129)], {}),
        ("n_a above its capacity", b"capacity", [pair(n_a=261)], {}),
        ("n_b above its capacity", b"capacity", [pair(n_b=301)], {}),
        ("capacity * item_len overflows", b"overflows", [pair(BYTES, 1 << 20, capacity_b=1 << 50)], {}),
        ("a level 0 for a list tree", b"list tree", [pair(LIST, 8, d_b_level0=P + 50 * MB)], {}),
        ("null level 0 (a)", b"null pointer", [pair(d_a_level0=None)], {}),
        ("null level 0 (b)", b"null pointer", [pair(d_b_level0=None)], {}),
        ("null values of a list tree", b"null pointer", [pair(LIST, 8, d_a_items=None)], {}),
        ("null levels (a)", b"null level array", [pair(d_a_levels=None)], {}),
        ("null levels (b)", b"null level array", [pair(d_b_levels=None)], {}),
        ("misaligned levels", b"misaligned", [pair(d_b_levels=P + 10 * MB + 8)], {}),
        ("misaligned level 0", b"misaligned", [pair(d_a_level0=P + 2 * MB + 4)], {}),
        ("a null index buffer", b"null index buffer", [pair(d_idx_out=None)], {}),
        ("a misaligned index buffer", b"misaligned", [pair(d_idx_out=P + 12 * MB + 4)], {}),
        ("null reports", b"reports", [pair()], {"reports": None}),
        ("misaligned reports", b"reports", [pair()], {"reports": REP + 4}),
        ("the indices over a's levels", b"overlaps an input", [pair(d_idx_out=levels_a + 32)], {}),
        ("the indices over b's level 0", b"overlaps an input", [pair(d_idx_out=P + 8 * MB + 32 * 299)], {}),
        ("the indices over another pair's values", b"overlaps an input",
         [pair(), pair(LIST, 8, base=P + 40 * MB, d_idx_out=P + 8)], {}),
        ("the reports over an input", b"overlaps an input", [pair()], {"reports": levels_a}),
        ("the reports over the indices", b"two output ranges", [pair()], {"reports": P + 12 * MB + 8}),
        ("two pairs' indices over each other", b"two output ranges",
         [pair(), pair(base=P + 40 * MB, d_idx_out=P + 12 * MB + 8 * 63)], {}),
        ("2^31 work items", b"work items", [pair(LIST, 128, n_a=1 << 41, capacity_a=1 << 41, n_b=1 << 41,
                                                 capacity_b=1 << 41)], {}),
    ]
    for what, text, pairs, kw in bad:
        rc, err = diff(lib, pairs, **kw)
        assert rc == _lib.MK_EINVAL and text in err, f"{what}: {rc} {err}"
    assert lib.mk_dev_ssz_trees_diff(None, None, 3, ctypes.c_void_p(REP), None) == _lib.MK_EINVAL


def test_what_the_shape_does_not_need_may_be_null(lib):
    """m == 0 needs no leaves and no levels, min(D_a, D_b) == 0 no levels, max_out == 0 no index buffer, and a
    STRUCT / BYTES pair no values: with the rest of the call refused (no reports), none of these is reported.
    The same buffers on both sides are no overlap."""
    ok = [pair(n_a=0, d_a_level0=None, d_a_levels=None, d_b_levels=None, d_b_level0=None),
          pair(n_a=4, d_a_levels=None, d_b_levels=None),
          pair(LIST, 8, n_b=16, d_a_levels=None, d_b_levels=None),
          pair(max_out=0, d_idx_out=None), pair(d_a_items=None, d_b_items=None),
          pair(d_b_items=P, d_b_level0=P + 2 * MB, d_b_levels=P + 4 * MB, n_b=257, capacity_b=260)]
    for t in ok:
        rc, err = diff(lib, [t], reports=None)
        assert rc == _lib.MK_EINVAL and b"reports" in err, err
    rc, err = diff(lib, [pair(n_a=5, d_a_levels=None)])
    assert rc == _lib.MK_EINVAL and b"null level array" in err


@pytest.mark.parametrize("kind", ["list", "struct_list", "bytes_list"])
def test_handle_entries_refuse_null(lib, kind):
    fn = getattr(lib, f"mk_{kind}_tree_diff")
    call = _lib.Call(-1, 0, b"")
    out = (ctypes.c_uint64 * 4)()
    tot, na, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    h = ctypes.c_void_p(P)
    r = [ctypes.byref(tot), ctypes.byref(na), ctypes.byref(nb)]
    assert fn(ctypes.byref(call), None, h, out, 4, *r) == _lib.MK_EINVAL
    assert b"null pointer" in call.err and call.code == _lib.MK_EINVAL
    assert fn(ctypes.byref(call), h, None, out, 4, *r) == _lib.MK_EINVAL
    assert fn(ctypes.byref(call), h, h, None, 4, *r) == _lib.MK_EINVAL
    for k in range(3):
        assert fn(ctypes.byref(call), h, h, out, 4, *[None if i == k else x for i, x in enumerate(r)]) == _lib.MK_EINVAL
    assert fn(ctypes.byref(call), h, ctypes.c_void_p(P + MB), out, 1 << 61, *r) == _lib.MK_EINVAL
    assert b"overflows" in call.err


def test_set_entry_without_a_device(lib):
    call = _lib.Call(-1, 0, b"")
    rep = (_lib.DiffReport * 2)()
    assert lib.mk_tree_set_diff(ctypes.byref(call), None, None, rep, None, 0) == _lib.MK_EINVAL
    assert b"null pointer" in call.err
    s, t, u = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.mk_tree_set_new(ctypes.byref(call), 64, ctypes.byref(s)) == _lib.MK_OK
    assert lib.mk_tree_set_new(ctypes.byref(call), 64, ctypes.byref(t)) == _lib.MK_OK
    assert lib.mk_tree_set_new(ctypes.byref(call), 72, ctypes.byref(u)) == _lib.MK_OK
    try:
        assert lib.mk_tree_set_diff(ctypes.byref(call), s, t, None, None, 0) == _lib.MK_EINVAL
        assert lib.mk_tree_set_diff(ctypes.byref(call), s, t, rep, None, 4) == _lib.MK_EINVAL
        assert lib.mk_tree_set_diff(ctypes.byref(call), s, u, rep, None, 0) == _lib.MK_EINVAL
        assert b"containers of 64 and 72 bytes" in call.err
        # two sets without trees need no device: the container report is the host's
        data = (ctypes.c_uint8 * 3)(1, 0, 3)
        assert lib.mk_tree_set_put(ctypes.byref(call), t, 9, data, 3) == _lib.MK_OK
        assert lib.mk_tree_set_diff(ctypes.byref(call), s, t, rep, None, 0) == _lib.MK_OK, call.err
        assert rep[0].astuple() == (2, 9)
        assert lib.mk_tree_set_diff(ctypes.byref(call), t, t, rep, None, 0) == _lib.MK_OK
        assert rep[0].astuple() == (0, (1 << 64) - 1)
    finally:
        for x in (s, t, u):
            lib.mk_tree_set_free(x)


def test_header_table_and_library_agree_on_the_new_entries(lib):
    want = {f"mk_{k}_tree_diff" for k in ("list", "struct_list", "bytes_list")}
    want |= {"mk_tree_set_diff", "mk_dev_ssz_trees_diff"}
    names = set(_lib.header_symbols())
    for sym in sorted(want):
        assert sym in names and sym in _lib._SIGS and hasattr(lib, sym), sym
    assert ctypes.sizeof(_lib.DiffReport) == 16 and ctypes.sizeof(_lib.TreeDiff) == 104
