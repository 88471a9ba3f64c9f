"""Host side of the resident trees' audit: the numpy model of
the rule (tests/tree_audit_ref.py) against the oracle's trees -- clean on every
shape, and a flipped node reported exactly where it is stored and where it is a
child -- and every argument error of mk_dev_ssz_trees_audit, decided before a
device is looked up (the pointers are made-up addresses that are only ever
compared)."""
import ctypes
import os

import numpy as np
import pytest

from prysm_amd import _lib
from tests import tree_audit_ref as A
from tests.test_gpu_list_tree import oracle_tree

P = 0x7F0000001000  # a 4096-B aligned address that is never dereferenced
MB = 1 << 20
LIST, STRUCT, BYTES = _lib.MK_TREE_LIST, _lib.MK_TREE_STRUCT, _lib.MK_TREE_BYTES
SEED = 0x5EED000000000000 + 2600
LENS = [1, 8, 32, 48, 64, 100, 128]
COUNTS = list(range(41)) + [63, 64, 65, 129]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def host_tree(n, cap, L, fill=0xA5, salt=0):
    """(items, level array laid out for cap, root) of the oracle's tree of n items of L bytes; every byte
    the tree does not own is `fill`."""
    from oracle import oracle as O

    items = np.full(cap * L + 16, fill, dtype=np.uint8)
    items[:n * L] = O.splitmix_bytes((n * L + 7) // 8 * 8 + 8, SEED + 131 * L + n + salt)[:n * L]
    levels, root = oracle_tree(items, n, L)
    total = sum(c for _, c in A.level_layout(cap, cap, L)) if cap else 0
    lv = np.full(32 * max(total, 1), fill, dtype=np.uint8)
    for (off, c), nodes in zip(A.level_layout(n, cap, L), levels):
        assert len(nodes) == c
        lv[32 * off:32 * (off + c)] = nodes.reshape(-1)
    return items, lv, np.frombuffer(root, dtype=np.uint8).copy()


@pytest.mark.parametrize("L", LENS)
def test_model_is_clean_on_the_oracles_trees(L):
    for n in COUNTS:
        for cap in (n, 2 * n + 3):
            items, lv, root = host_tree(n, cap, L)
            assert A.tree_mismatches(items, lv, root, n, cap, L) == set(), (L, n, cap)
            assert A.report(set()) == (0, A.NONE, A.NO_INDEX)


@pytest.mark.parametrize("L", [8, 32, 100])
def test_a_flipped_node_is_reported_where_it_is_stored_and_where_it_is_a_child(L):
    p = A.per(L)
    for n in (p + 1, 5 * p, 37 * p, 64 * p + 1):
        cap = 2 * n + 3
        items, lv, root = host_tree(n, cap, L)
        lay = A.level_layout(n, cap, L)
        D = len(lay)
        assert D >= 1
        for d, (off, c) in enumerate(lay, 1):
            for j in range(c):
                x = lv.copy()
                x[32 * (off + j) + (7 * j + d) % 32] ^= 0x10
                want = {(d, j), (A.ROOT, 0) if d == D else (d + 1, j >> 1)}
                assert A.tree_mismatches(items, x, root, n, cap, L) == want, (L, n, d, j)
            # a node beyond the level's count belongs to no check
            nxt = lay[d][0] if d < D else len(lv) // 32
            if off + c < nxt:
                x = lv.copy()
                x[32 * (off + c) + 3] ^= 0xFF
                assert A.tree_mismatches(items, x, root, n, cap, L) == set(), (L, n, d, "beyond")
        r = root.copy()
        r[31] ^= 1
        assert A.tree_mismatches(items, lv, r, n, cap, L) == {(A.ROOT, 0)}
        x = items.copy()
        x[n * L - 1] ^= 1  # the last item: its window only
        assert A.tree_mismatches(x, lv, root, n, cap, L) == {(1, lay[0][1] - 1)}
        x = items.copy()
        x[n * L] ^= 1  # the first byte beyond the list
        assert A.tree_mismatches(x, lv, root, n, cap, L) == set()
        assert A.report({(3, 1), (2, 9), (A.ROOT, 0)}) == (3, 2, 9)


def test_short_lists_have_only_a_root():
    for L, n in ((8, 0), (8, 1), (8, 16), (32, 4), (128, 1), (100, 1)):
        items, lv, root = host_tree(n, n + 2, L)
        assert A.level_layout(n, n + 2, L) == []
        assert A.tree_mismatches(items, lv, root, n, n + 2, L) == set()
        if n:
            x = items.copy()
            x[0] ^= 1
            assert A.tree_mismatches(x, lv, root, n, n + 2, L) == {(A.ROOT, 0)}


def test_container_model():
    from oracle import oracle as O

    r0, r1 = bytes(range(32)), bytes(range(32, 64))
    msg = bytearray(r0 + bytes(8) + r1)
    croot = O.keccak256(bytes(msg))
    trees = [(r0, 0), (b"x" * 32, None), (r1, 40)]
    assert A.container_mismatches(msg, croot, trees) == set()
    msg[41] ^= 1
    assert A.container_mismatches(msg, croot, trees) == {(A.CONTAINER, 0), (A.CONTAINER, 3)}
    assert A.level0_mismatches(np.arange(96, dtype=np.uint8), np.arange(96, dtype=np.uint8), 3) == set()
    x = np.arange(96, dtype=np.uint8)
    x[40] ^= 1
    assert A.level0_mismatches(x, np.arange(96, dtype=np.uint8), 3) == {(0, 1)}


# ---- the device entry's refusals, without a device ---------------------------------------------------
FIELDS = [(1, 0, 48), (2, 48, 8)]
_KEEP = []


def tree(kind=BYTES, item_len=32, n=257, capacity=260, base=P, fields=None, container_off=None, **ptrs):
    t = _lib.TreeAudit()
    t.kind, t.item_len, t.n, t.capacity = kind, item_len, n, capacity
    for i, name in enumerate(("d_items", "d_level0", "d_levels", "d_root32")):
        v = base + 2 * i * MB
        if kind == LIST and name == "d_level0":
            v = None
        setattr(t, name, ptrs.get(name, v))
    keep = None
    if fields is not None:
        from prysm_amd.registry import _fields

        keep = _fields(fields)
        t.fields, t.nfields = ctypes.cast(keep, ctypes.c_void_p), len(fields)
    t.container_off = _lib.MK_NO_CONTAINER if container_off is None else container_off
    _KEEP.append(keep)  # a descriptor copied into an array still points at its fields
    return t


REP, WS, MSG, CROOT = P + 100 * MB, P + 102 * MB, P + 104 * MB, P + 106 * MB


def audit(lib, trees, container=(None, 0, None), reports=REP, ws=WS, ws_bytes=1 << 30, ntrees=None):
    arr = (_lib.TreeAudit * max(len(trees), 1))(*trees)
    call = _lib.Call(-1, 0, b"")
    rc = lib.mk_dev_ssz_trees_audit(ctypes.byref(call), arr, len(trees) if ntrees is None else ntrees,
                                    ctypes.c_void_p(container[0]), container[1], ctypes.c_void_p(container[2]),
                                    ctypes.c_void_p(reports), ctypes.c_void_p(ws), ws_bytes, None)
    assert call.code == rc
    return rc, call.err


def test_every_refusal_needs_no_device(lib):
    with_msg = (MSG, 72, CROOT)
    bad = [
        ("no trees", b"0 trees", [], {}),
        ("17 trees", b"17 trees", [tree(base=P + 8 * i * MB) for i in range(17)], {}),
        ("an unknown kind", b"unknown kind", [tree(kind=0)], {}),
        ("another unknown kind", b"unknown kind", [tree(kind=4)], {}),
        ("item_len == 0", b"item_len == 0", [tree(LIST, 0)], {}),
        ("a list item above 128", b"above 128", [tree(LIST, 129)], {}),
        ("n above the capacity", b"capacity", [tree(n=261)], {}),
        ("capacity * item_len overflows", b"overflows", [tree(BYTES, 1 << 20, capacity=1 << 50)], {}),
        ("a level 0 for a list tree", b"list tree", [tree(LIST, 8, d_level0=P + 50 * MB)], {}),
        ("a struct tree without fields", b"field layout", [tree(STRUCT, 56)], {}),
        ("fields for a bytes tree", b"field layout", [tree(BYTES, 32, fields=FIELDS)], {}),
        ("a bad field layout", b"", [tree(STRUCT, 56, fields=[(1, 40, 48)])], {}),
        ("null root", b"null pointer", [tree(d_root32=None)], {}),
        ("null values", b"null pointer", [tree(d_items=None)], {}),
        ("null level 0", b"null pointer", [tree(d_level0=None)], {}),
        ("null levels", b"null level array", [tree(d_levels=None)], {}),
        ("misaligned levels", b"misaligned", [tree(d_levels=P + 8)], {}),
        ("misaligned level 0", b"misaligned", [tree(d_level0=P + 50 * MB + 4)], {}),
        ("misaligned root", b"misaligned", [tree(d_root32=P + 50 * MB + 8)], {}),
        ("misaligned records", b"misaligned", [tree(STRUCT, 56, fields=FIELDS, d_items=P + 2)], {}),
        ("null reports", b"reports", [tree()], {"reports": None}),
        ("misaligned reports", b"reports", [tree()], {"reports": REP + 4}),
        ("null workspace", b"workspace", [tree()], {"ws": None}),
        ("misaligned workspace", b"workspace", [tree()], {"ws": WS + 8}),
        ("a container offset without a container", b"without a container", [tree(container_off=0)], {}),
        ("a container above the limit", b"limit", [tree()], {"container": (MSG, 4097, CROOT)}),
        ("a null container", b"null pointer", [tree(container_off=0)], {"container": (None, 72, CROOT)}),
        ("a null container root", b"null pointer", [tree(container_off=0)], {"container": (MSG, 72, None)}),
        ("a misaligned container", b"misaligned", [tree(container_off=0)], {"container": (MSG + 2, 72, CROOT)}),
        ("a misaligned container offset", b"aligned", [tree(container_off=2)], {"container": with_msg}),
        ("a container offset beyond the message", b"beyond", [tree(container_off=44)], {"container": with_msg}),
        ("overlapping container offsets", b"overlaps",
         [tree(container_off=0), tree(LIST, 8, base=P + 20 * MB, container_off=16)], {"container": with_msg}),
        ("2^31 work items", b"work items", [tree(LIST, 128, n=1 << 31, capacity=1 << 31)], {}),
        ("2^31 level-0 entries", b"work items", [tree(BYTES, 32, n=(1 << 31) - 5, capacity=1 << 31)], {}),
    ]
    for what, text, trees, kw in bad:
        rc, err = audit(lib, trees, **kw)
        assert rc == _lib.MK_EINVAL and text in err, f"{what}: {rc} {err}"
    assert lib.mk_dev_ssz_trees_audit(None, None, 3, None, 0, None, ctypes.c_void_p(REP), None, 0, None) == _lib.MK_EINVAL


def test_a_short_workspace_is_enomem(lib):
    t = [tree(), tree(STRUCT, 56, n=300000, capacity=300000, base=P + 20 * MB, fields=FIELDS)]
    arr = (_lib.TreeAudit * 2)(*t)
    need = lib.mk_ssz_trees_audit_workspace_bytes(arr, 2)
    assert need >= 32 * (1 << 18)
    rc, err = audit(lib, t, ws_bytes=need - 1)
    assert rc == _lib.MK_ENOMEM and b"workspace too small" in err
    # the workspace is one piece's whatever n is, and nothing for list trees
    big = (_lib.TreeAudit * 1)(tree(STRUCT, 56, n=1 << 24, capacity=1 << 24, fields=FIELDS))
    assert lib.mk_ssz_trees_audit_workspace_bytes(big, 1) == need
    only = (_lib.TreeAudit * 1)(tree(LIST, 8, n=1 << 20, capacity=1 << 20))
    assert lib.mk_ssz_trees_audit_workspace_bytes(only, 1) == 0
    assert lib.mk_ssz_trees_audit_workspace_bytes(None, 1) == 0
    assert lib.mk_ssz_trees_audit_workspace_bytes((_lib.TreeAudit * 1)(tree(kind=9)), 1) == 0


def test_what_the_shape_does_not_need_may_be_null(lib):
    """An empty tree needs no values, no level 0 and no levels, a list of one chunk no levels: with the rest
    of the call refused (no reports), the null pointers are not what is reported."""
    for t in (tree(n=0, d_items=None, d_level0=None, d_levels=None), tree(n=4, d_levels=None),
              tree(LIST, 8, n=16, capacity=900, d_levels=None)):
        rc, err = audit(lib, [t], reports=None)
        assert rc == _lib.MK_EINVAL and b"reports" in err, err
    rc, err = audit(lib, [tree(n=5, d_levels=None)])
    assert rc == _lib.MK_EINVAL and b"null level array" in err


@pytest.mark.parametrize("kind", ["list", "struct_list", "bytes_list"])
def test_handle_entries_refuse_null(lib, kind):
    call = _lib.Call(-1, 0, b"")
    out = _lib.AuditReport()
    assert getattr(lib, f"mk_{kind}_tree_audit")(ctypes.byref(call), None, ctypes.byref(out)) == _lib.MK_EINVAL
    assert b"null pointer" in call.err and call.code == _lib.MK_EINVAL
    assert getattr(lib, f"mk_{kind}_tree_audit")(ctypes.byref(call), ctypes.c_void_p(P), None) == _lib.MK_EINVAL


def test_set_entry_without_a_device(lib):
    call = _lib.Call(-1, 0, b"")
    out = (_lib.AuditReport * 2)()
    assert lib.mk_tree_set_audit(ctypes.byref(call), None, out) == _lib.MK_EINVAL and b"null pointer" in call.err
    s = ctypes.c_void_p()
    assert lib.mk_tree_set_new(ctypes.byref(call), 64, ctypes.byref(s)) == _lib.MK_OK
    try:
        assert lib.mk_tree_set_audit(ctypes.byref(call), s, None) == _lib.MK_EINVAL
        assert lib.mk_tree_set_audit(ctypes.byref(call), s, out) == _lib.MK_EINVAL and b"without trees" in call.err
    finally:
        lib.mk_tree_set_free(s)


def test_header_table_and_library_agree_on_the_new_entries(lib):
    want = {f"mk_{k}_tree_audit" for k in ("list", "struct_list", "bytes_list")}
    want |= {"mk_tree_set_audit", "mk_dev_ssz_trees_audit", "mk_ssz_trees_audit_workspace_bytes"}
    names = set(_lib.header_symbols())
    for sym in sorted(want):
        assert sym in names and sym in _lib._SIGS and hasattr(lib, sym), sym
    assert ctypes.sizeof(_lib.AuditReport) == 24 and ctypes.sizeof(_lib.TreeAudit) == 72
    with open(_lib.HEADER) as f:
        h = f.read()
    assert "#define MK_AUDIT_ROOT 64u" in h and "#define MK_AUDIT_CONTAINER 65u" in h
    assert (_lib.MK_AUDIT_ROOT, _lib.MK_AUDIT_CONTAINER, _lib.MK_AUDIT_NONE) == (A.ROOT, A.CONTAINER, A.NONE)
