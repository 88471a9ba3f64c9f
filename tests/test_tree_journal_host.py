"""The undo journal's device entries without a device: every
refusal of mk_dev_ssz_trees_journal / _restore is decided before a device is
looked up, by the rules of mk_dev_ssz_trees_update, and
mk_ssz_trees_journal_bytes is the layout of csrc/tree_journal.hpp, restated
here by hand.  The pointers are made-up addresses: nothing is launched."""
import ctypes

import pytest

from prysm_amd import _lib

LIST, STRUCT, BYTES = _lib.MK_TREE_LIST, _lib.MK_TREE_STRUCT, _lib.MK_TREE_BYTES
P = 0x7F0000000000  # a made-up, 16-B aligned device address
MB = 1 << 20


@pytest.fixture(scope="module")
def lib():
    import os

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def tree(kind=LIST, item_len=8, n_old=1000, n_new=1000, capacity=1024, k_idx=3, off=_lib.MK_NO_CONTAINER, **over):
    t = _lib.TreeUpdate()
    t.kind, t.item_len, t.n_old, t.n_new, t.capacity, t.k_idx = kind, item_len, n_old, n_new, capacity, k_idx
    t.d_items, t.d_levels, t.d_root32, t.d_idx, t.d_values = P, P + 2 * MB, P + 4 * MB, P + 6 * MB, P + 8 * MB
    t.d_level0 = None if kind == LIST else P + 10 * MB
    t.container_off = off
    for name, v in over.items():
        setattr(t, name, v)
    return t


def call(lib, name, trees, journal=P + 32 * MB, nbytes=1 << 40, container=(None, 0, None), ntrees=None):
    arr = (_lib.TreeUpdate * max(len(trees), 1))(*trees)
    c = _lib.Call(-1, 0, b"")
    rc = getattr(lib, name)(ctypes.byref(c), arr, len(trees) if ntrees is None else ntrees, ctypes.c_void_p(container[0]),
                            container[1], ctypes.c_void_p(container[2]), ctypes.c_void_p(journal), nbytes, None)
    assert c.code == rc
    return rc, c.err


def want_bytes(kind, item_len, n_old, n_new, k_idx):
    """tree_journal.hpp by hand: the index list (to 16 B), the root, a record per work item."""
    leaf = item_len if kind == LIST else 32
    p = 128 // leaf if leaf < 128 else 1
    nch, D = -(-n_old // p), 0
    while -(-nch // (1 << D)) > 1:
        D += 1
    W = (k_idx + (1 if n_new > n_old else 0)) if n_old else 0
    up16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    return up16(8 * W) + 32 + W * (up16(item_len) + (0 if kind == LIST else 32) + 32 * D)


@pytest.mark.parametrize("kind,item_len,n_old,n_new,k_idx", [
    (LIST, 8, 1000, 1000, 3), (LIST, 8, 1000, 1025, 0), (LIST, 48, 5, 5, 1), (LIST, 160, 9, 12, 2), (LIST, 32, 0, 7, 4),
    (BYTES, 48, 37, 38, 2), (BYTES, 32, 4, 4, 1), (BYTES, 32, 1 << 20, 1 << 20, 1000), (LIST, 8, 1, 1, 1)])
def test_journal_bytes_is_the_layout(lib, kind, item_len, n_old, n_new, k_idx):
    t = tree(kind, item_len, n_old, n_new, max(n_new, 1) + 5, k_idx)
    arr = (_lib.TreeUpdate * 1)(t)
    want = want_bytes(kind, item_len, n_old, n_new, k_idx)
    assert lib.mk_ssz_trees_journal_bytes(arr, 1, 0) == want
    two = (_lib.TreeUpdate * 2)(t, tree(off=8))
    assert lib.mk_ssz_trees_journal_bytes(two, 2, 107) == want + want_bytes(LIST, 8, 1000, 1000, 3) + 112 + 32


def test_journal_bytes_of_a_refused_array_is_zero(lib):
    for t, n, clen in ((tree(kind=0), 1, 0), (tree(item_len=0), 1, 0), (tree(n_new=999), 1, 0), (tree(n_new=2000), 1, 0),
                       (tree(), 0, 0), (tree(), 17, 0), (tree(), 1, _lib.MK_CONTAINER_MAX + 1)):
        arr = (_lib.TreeUpdate * 17)(*([t] * 17))
        assert lib.mk_ssz_trees_journal_bytes(arr, n, clen) == 0
    assert lib.mk_ssz_trees_journal_bytes(None, 1, 0) == 0


@pytest.mark.parametrize("name", ["mk_dev_ssz_trees_journal", "mk_dev_ssz_trees_restore"])
def test_every_refusal_needs_no_device(lib, name):
    EINVAL, ENOMEM = _lib.MK_EINVAL, _lib.MK_ENOMEM
    need = want_bytes(LIST, 8, 1000, 1000, 3)
    assert call(lib, name, [tree()], journal=None)[0] == EINVAL
    rc, err = call(lib, name, [tree()], journal=P + 8)
    assert rc == EINVAL and b"journal" in err
    rc, err = call(lib, name, [tree()], nbytes=need - 1)
    assert rc == ENOMEM and b"journal" in err
    bad = [("no trees", b"trees in one call", []), ("an unknown kind", b"unknown kind", [tree(kind=7)]),
           ("item_len == 0", b"item_len == 0", [tree(item_len=0)]), ("a shrink", b"n_old", [tree(n_new=10)]),
           ("beyond the capacity", b"capacity", [tree(n_new=1025)]),
           ("a level 0 for a list tree", b"d_level0", [tree(d_level0=P + 10 * MB)]),
           ("no level 0 for a bytes tree", b"d_level0", [tree(BYTES, 32, d_level0=None)]),
           ("a null root", b"null pointer", [tree(d_root32=None)]),
           ("misaligned levels", b"misaligned", [tree(d_levels=P + 2 * MB + 8)]),
           ("a container offset without a container's room", b"beyond", [tree(off=96)])]
    for what, text, trees in bad:
        cont = (P + 40 * MB, 100, P + 41 * MB) if what.startswith("a container") else (None, 0, None)
        rc, err = call(lib, name, trees, container=cont)
        assert rc == EINVAL and text in err, f"{what}: {rc} {err}"
    rc, err = call(lib, name, [tree(off=8)], container=(None, 100, P + 41 * MB), nbytes=need + 112 + 32)
    assert rc == EINVAL and b"container" in err
    rc, err = call(lib, name, [tree(off=8)], container=(P + 40 * MB, 100, P + 41 * MB), nbytes=need + 112 + 31)
    assert rc == ENOMEM
    # the index list: journal reads it, restore does not
    rc, err = call(lib, name, [tree(d_idx=None)], nbytes=need - 1)
    if name.endswith("journal"):
        assert rc == EINVAL and b"index array" in err
    else:
        assert rc == ENOMEM  # the next check in line: the list was not asked for


def test_header_table_and_library_agree_on_the_new_entries(lib):
    names = set(_lib.header_symbols())
    for sym in ("mk_ssz_trees_journal_bytes", "mk_dev_ssz_trees_journal", "mk_dev_ssz_trees_restore"):
        assert sym in names and sym in _lib._SIGS and hasattr(lib, sym), sym
