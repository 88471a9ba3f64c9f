"""Host-side logic of the tree copy entries: every argument
error of mk_dev_ssz_trees_copy is decided before a device is looked up -- the
code and the mk_call text -- and the handle and set entries refuse null.  Every
call here carries an error or has nothing to do, so none reaches a device (the
pointers are made-up addresses that are only ever compared)."""
import ctypes
import os

import pytest

from prysm_amd import _lib

P = 0x7F0000001000  # a 4096-B aligned address that is never dereferenced
MB = 1 << 20
LIST, STRUCT, BYTES = _lib.MK_TREE_LIST, _lib.MK_TREE_STRUCT, _lib.MK_TREE_BYTES


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def tree(kind=BYTES, item_len=32, n=257, src_capacity=260, dst_capacity=517, base=P, **ptrs):
    """A well-formed descriptor in its own 16 MB of made-up address space; ptrs overrides single pointers."""
    t = _lib.TreeCopy()
    t.kind, t.item_len, t.n, t.src_capacity, t.dst_capacity = kind, item_len, n, src_capacity, dst_capacity
    names = ("d_src_items", "d_src_level0", "d_src_levels", "d_src_root32",
             "d_dst_items", "d_dst_level0", "d_dst_levels", "d_dst_root32")
    for i, name in enumerate(names):
        v = base + 2 * i * MB
        if kind == LIST and name.endswith("level0"):
            v = None
        setattr(t, name, ptrs.get(name, v))
    return t


def copy(lib, trees, extra=(None, None), ntrees=None):
    arr = (_lib.TreeCopy * max(len(trees), 1))(*trees)
    call = _lib.Call(-1, 0, b"")
    rc = lib.mk_dev_ssz_trees_copy(ctypes.byref(call), arr, len(trees) if ntrees is None else ntrees,
                                   ctypes.c_void_p(extra[0]), ctypes.c_void_p(extra[1]), None)
    assert call.code == rc
    return rc, call.err


def test_every_refusal_needs_no_device(lib):
    other = P + 64 * MB
    bad = [
        ("null destination root", b"null pointer", [tree(d_dst_root32=None)]),
        ("null source root", b"null pointer", [tree(d_src_root32=None)]),
        ("null values", b"null pointer", [tree(d_dst_items=None)]),
        ("null level 0", b"null pointer", [tree(d_src_level0=None)]),
        ("null levels", b"null level array", [tree(d_dst_levels=None)]),
        ("a level 0 for a list tree", b"list tree", [tree(LIST, 8, d_dst_level0=other)]),
        ("misaligned levels", b"misaligned", [tree(d_dst_levels=other + 8)]),
        ("misaligned level 0", b"misaligned", [tree(d_src_level0=other + 4)]),
        ("misaligned root", b"misaligned", [tree(d_dst_root32=other + 8)]),
        ("item_len == 0", b"item_len == 0", [tree(LIST, 0)]),
        ("item_len above 2^30", b"2^30", [tree(LIST, (1 << 30) + 1)]),
        ("an unknown kind", b"unknown kind", [tree(kind=0)]),
        ("another unknown kind", b"unknown kind", [tree(kind=4)]),
        ("n above the source's capacity", b"capacity", [tree(n=261)]),
        ("n above the destination's capacity", b"capacity", [tree(dst_capacity=256)]),
        ("capacity * item_len overflows", b"overflows", [tree(LIST, 1 << 20, dst_capacity=1 << 50)]),
        ("17 trees", b"17 trees", [tree(base=P + 32 * i * MB) for i in range(17)]),
        ("the values onto themselves", b"overlaps", [tree(d_dst_items=P)]),
        ("a destination that ends inside a source", b"overlaps", [tree(d_dst_items=P - 257 * 32 + 16)]),
        ("the source's levels as the destination's", b"overlaps", [tree(d_dst_levels=P + 4 * MB)]),
        ("a destination root that is another tree's source root", b"overlaps",
         [tree(), tree(LIST, 8, base=other, d_dst_root32=P + 6 * MB)]),
    ]
    for what, text, trees in bad:
        rc, err = copy(lib, trees)
        assert rc == _lib.MK_EINVAL and text in err, f"{what}: {rc} {err}"
    for what, text, extra in (("a one-sided extra", b"extra", (None, other)), ("the other side", b"extra", (other, None)),
                              ("a misaligned extra", b"misaligned", (other, other + 64 + 8)),
                              ("the extra onto a source root", b"overlaps", (other, P + 6 * MB)),
                              ("the extra from a destination", b"overlaps", (P + 14 * MB, other))):
        rc, err = copy(lib, [tree()], extra)
        assert rc == _lib.MK_EINVAL and text in err, f"{what}: {rc} {err}"
    assert lib.mk_dev_ssz_trees_copy(None, None, 3, None, None, None) == _lib.MK_EINVAL  # no table for three trees


def test_what_the_shape_does_not_need_may_be_null(lib):
    """An empty tree needs no values, no level 0 and no levels; a list of one chunk needs no levels: with the
    rest of the call refused (an overlap at the roots), the null pointers are not what is reported."""
    for t in (tree(n=0, d_src_items=None, d_dst_items=None, d_src_level0=None, d_dst_level0=None, d_src_levels=None,
                   d_dst_levels=None, d_dst_root32=P + 6 * MB),
              tree(n=4, d_src_levels=None, d_dst_levels=None, d_dst_root32=P + 6 * MB),
              tree(LIST, 8, n=16, d_src_levels=None, d_dst_levels=None, d_dst_root32=P + 6 * MB)):
        rc, err = copy(lib, [t])
        assert rc == _lib.MK_EINVAL and b"overlaps" in err, err
    rc, err = copy(lib, [tree(n=5, d_src_levels=None)])  # two chunks: a level
    assert rc == _lib.MK_EINVAL and b"null level array" in err


def test_nothing_to_do_is_ok_without_a_device(lib):
    rc, err = copy(lib, [])
    assert rc == _lib.MK_OK and err == b""


@pytest.mark.parametrize("kind", ["list", "struct_list", "bytes_list"])
def test_handle_entries_refuse_null(lib, kind):
    call = _lib.Call(-1, 0, b"")
    out = ctypes.c_void_p(1)
    fake = ctypes.c_void_p(P)
    assert getattr(lib, f"mk_{kind}_tree_clone")(ctypes.byref(call), None, ctypes.byref(out)) == _lib.MK_EINVAL
    assert b"null pointer" in call.err and call.code == _lib.MK_EINVAL and not out.value
    assert getattr(lib, f"mk_{kind}_tree_clone")(ctypes.byref(call), None, None) == _lib.MK_EINVAL
    assert getattr(lib, f"mk_{kind}_tree_copy")(ctypes.byref(call), None, None) == _lib.MK_EINVAL
    assert getattr(lib, f"mk_{kind}_tree_copy")(ctypes.byref(call), fake, None) == _lib.MK_EINVAL
    assert getattr(lib, f"mk_{kind}_tree_copy")(ctypes.byref(call), None, fake) == _lib.MK_EINVAL
    assert getattr(lib, f"mk_{kind}_tree_copy")(ctypes.byref(call), fake, fake) == _lib.MK_OK  # onto itself: nothing
    assert getattr(lib, f"mk_{kind}_tree_reserve")(ctypes.byref(call), None, 10) == _lib.MK_EINVAL
    assert getattr(lib, f"mk_{kind}_tree_capacity")(None) == 0


def test_set_entries_without_a_device(lib):
    call = _lib.Call(-1, 0, b"")
    a, b, c = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.mk_tree_set_new(ctypes.byref(call), 64, ctypes.byref(a)) == _lib.MK_OK
    assert lib.mk_tree_set_new(ctypes.byref(call), 72, ctypes.byref(b)) == _lib.MK_OK
    try:
        msg = (ctypes.c_uint8 * 8)(*range(8))
        assert lib.mk_tree_set_put(ctypes.byref(call), a, 8, msg, 8) == _lib.MK_OK
        assert lib.mk_tree_set_copy(ctypes.byref(call), b, a) == _lib.MK_EINVAL and b"containers of 72 and 64" in call.err
        assert lib.mk_tree_set_copy(ctypes.byref(call), a, a) == _lib.MK_OK
        assert lib.mk_tree_set_copy(ctypes.byref(call), None, a) == _lib.MK_EINVAL and b"null pointer" in call.err
        assert lib.mk_tree_set_copy(ctypes.byref(call), a, None) == _lib.MK_EINVAL
        assert lib.mk_tree_set_clone(ctypes.byref(call), None, ctypes.byref(c)) == _lib.MK_EINVAL
        assert lib.mk_tree_set_clone(ctypes.byref(call), a, None) == _lib.MK_EINVAL
        assert lib.mk_tree_set_reserve(ctypes.byref(call), a, 0, 10) == _lib.MK_EINVAL and b"tree 0 of a set of 0" in call.err
        assert lib.mk_tree_set_reserve(ctypes.byref(call), None, 0, 10) == _lib.MK_EINVAL
        assert lib.mk_tree_set_capacity(a, 0) == 0 and lib.mk_tree_set_capacity(None, 0) == 0
        # a set without trees clones and copies on any machine: only its message travels
        assert lib.mk_tree_set_clone(ctypes.byref(call), a, ctypes.byref(c)) == _lib.MK_OK and c.value
        d = ctypes.c_void_p()
        assert lib.mk_tree_set_new(ctypes.byref(call), 64, ctypes.byref(d)) == _lib.MK_OK
        assert lib.mk_tree_set_copy(ctypes.byref(call), d, a) == _lib.MK_OK
        lib.mk_tree_set_free(d)
    finally:
        for h in (a, b, c):
            if h.value:
                lib.mk_tree_set_free(h)


def test_header_table_and_library_agree_on_the_new_entries(lib):
    kinds = ("list", "struct_list", "bytes_list")
    want = {f"mk_{k}_tree_{op}" for k in kinds for op in ("clone", "copy", "reserve", "capacity")}
    want |= {f"mk_tree_set_{op}" for op in ("clone", "copy", "reserve", "capacity")} | {"mk_dev_ssz_trees_copy"}
    assert len(want) == 17
    names = set(_lib.header_symbols())
    for sym in sorted(want):
        assert sym in names and sym in _lib._SIGS and hasattr(lib, sym), sym
