"""Host-side logic of the shrink entry points: the erase
workspace queries and every argument error of the six device entry points
(mk_dev_ssz_*_tree_erase and their *_erase_workspace_bytes) and of the handle
and set entries that is decided before a device is looked up -- the code and
the mk_call text.  Every call here carries an error, so none reaches a device
(the pointers are made-up addresses that are only ever compared)."""
import ctypes
import os

import pytest

from prysm_amd import _lib
from prysm_amd import state as ST
from prysm_amd.registry import VALIDATOR_FIELDS, _fields

KINDS = ("list", "struct_list", "bytes_list")
NOUN = {"list": b"items", "struct_list": b"records", "bytes_list": b"elements"}
P = 0x7F0000001000  # a 4096-B aligned address that is never dereferenced


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def ws_bytes(lib, kind, moved, item_len):
    return getattr(lib, f"mk_ssz_{kind}_tree_erase_workspace_bytes")(moved, item_len)


def erase(lib, kind, n_old, n_new, cap, item_len=32, k_rm=0, first=0, ws=1 << 40, items=P, level0=P + (1 << 20),
          levels=P + (2 << 20), rm=P + (3 << 20), root=P + (4 << 20), d_ws=P + (5 << 20), fields=VALIDATOR_FIELDS):
    """One erase call with made-up device pointers; (rc, call)."""
    call = _lib.Call(-1, 0, b"")
    vp = ctypes.c_void_p
    if kind == "list":
        rc = lib.mk_dev_ssz_list_tree_erase(ctypes.byref(call), vp(items), n_old, n_new, cap, item_len, vp(levels),
                                            vp(rm), k_rm, first, vp(root), vp(d_ws), ws, None)
    elif kind == "struct_list":
        f = _fields(fields) if fields is not None else None
        rc = lib.mk_dev_ssz_struct_list_tree_erase(ctypes.byref(call), vp(items), n_old, n_new, cap, item_len, f,
                                                   len(fields or ()), vp(level0), vp(levels), vp(rm), k_rm, first,
                                                   vp(root), vp(d_ws), ws, None)
    else:
        rc = lib.mk_dev_ssz_bytes_list_tree_erase(ctypes.byref(call), vp(items), n_old, n_new, cap, item_len,
                                                  vp(level0), vp(levels), vp(rm), k_rm, first, vp(root), vp(d_ws),
                                                  ws, None)
    assert call.code == rc
    return rc, call


def item_len_of(kind):
    return 160 if kind == "struct_list" else 32


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("item_len", [1, 5, 8, 32, 33, 48, 160])
def test_workspace_is_monotone_and_never_zero(lib, kind, item_len):
    level0 = kind != "list"
    prev = 0
    for moved in (0, 1, 2, 31, 32, 33, 1000, 1 << 20, (1 << 20) + 1, (1 << 31) - 1):
        ws = ws_bytes(lib, kind, moved, item_len)
        # the arrival words of the climb, the moved values and (struct, bytes) their level-0 entries
        assert ws > 0 and ws >= prev and ws >= moved * (8 + item_len + (32 if level0 else 0)), moved
        prev = ws
    for moved in (0, 7, 4099):
        sizes = [ws_bytes(lib, kind, moved, L) for L in (1, 2, 8, 31, 32, 33, 160, 1 << 20)]
        assert sizes == sorted(sizes) and sizes[0] > 0, moved


@pytest.mark.parametrize("kind", KINDS)
def test_workspace_refuses_what_no_call_takes(lib, kind):
    assert ws_bytes(lib, kind, 1, 0) == 0        # no tree of 0-byte values
    assert ws_bytes(lib, kind, 1 << 31, 32) == 0  # more than one call moves


@pytest.mark.parametrize("kind", KINDS)
def test_shape_errors_need_no_device(lib, kind):
    L = item_len_of(kind)
    for what, text, kw in (
            ("item_len == 0", b"_len == 0", dict(n_old=10, n_new=9, cap=10, item_len=0)),
            ("n_old > capacity", b"capacity", dict(n_old=11, n_new=5, cap=10)),
            ("capacity * item_len overflows", b"overflows", dict(n_old=10, n_new=9, cap=1 << 62)),
            ("n_new > n_old", b"does not grow", dict(n_old=10, n_new=11, cap=20)),
            ("k_rm > n_old", b"removed indices", dict(n_old=10, n_new=0, cap=10, k_rm=11)),
            ("n_new != n_old - k_rm", b"less the 3 removed", dict(n_old=10, n_new=8, cap=10, k_rm=3)),
            ("n_new != n_old - k_rm (unchanged)", b"less the 1 removed", dict(n_old=10, n_new=10, cap=10, k_rm=1)),
            ("first > n_new", b"first 8 beyond the 7", dict(n_old=10, n_new=7, cap=10, k_rm=3, first=8)),
            ("first > n_new (truncate)", b"first 6 beyond the 5", dict(n_old=10, n_new=5, cap=10, first=6)),
            ("n_new - first >= 2^31", b"to move in one call",
             dict(n_old=(1 << 31) + 5, n_new=(1 << 31) + 4, cap=1 << 32, k_rm=1, first=4))):
        kw.setdefault("item_len", L)
        rc, call = erase(lib, kind, **kw)
        assert rc == _lib.MK_EINVAL and text in call.err, f"{what}: {rc} {call.err}"
    rc, call = erase(lib, kind, 10, 7, 10, item_len=L, k_rm=3, first=8)
    assert NOUN[kind] in call.err  # the kind's own word for a value


def test_elem_and_item_len_above_2_30(lib):
    for kind in ("list", "bytes_list"):
        rc, call = erase(lib, kind, 10, 9, 10, item_len=(1 << 30) + 1)
        assert rc == _lib.MK_EINVAL and b"2^30" in call.err


def test_struct_layout_errors_come_first(lib):
    rc, call = erase(lib, "struct_list", 10, 9, 10, item_len=36, fields=ST.CROSSLINK_FIELDS)  # a field beyond the record
    assert rc == _lib.MK_EINVAL and call.err
    rc, call = erase(lib, "struct_list", 10, 9, 10, item_len=160, fields=None)
    assert rc == _lib.MK_EINVAL and call.err


@pytest.mark.parametrize("kind", KINDS)
def test_short_workspace_is_enomem(lib, kind):
    L = item_len_of(kind)
    for n_old, k_rm, first in ((1000, 10, 0), (1000, 10, 500), (1000, 999, 0), (5000, 1, 4998)):
        n_new = n_old - k_rm
        need = ws_bytes(lib, kind, n_new - first, L)
        rc, call = erase(lib, kind, n_old, n_new, n_old, item_len=L, k_rm=k_rm, first=first, ws=need - 1)
        assert rc == _lib.MK_ENOMEM and b"workspace too small" in call.err, (n_old, k_rm, first)
    # a truncate moves nothing: the size of moved == 0, whatever `first` says
    need = ws_bytes(lib, kind, 0, L)
    rc, call = erase(lib, kind, 1000, 400, 1000, item_len=L, first=0, ws=need - 1)
    assert rc == _lib.MK_ENOMEM and b"workspace too small" in call.err
    rc, call = erase(lib, kind, 1000, 400, 1000, item_len=L, ws=0)
    assert rc == _lib.MK_ENOMEM
    # a bad shape is reported before a short workspace
    rc, call = erase(lib, kind, 10, 11, 20, item_len=L, ws=0)
    assert rc == _lib.MK_EINVAL


@pytest.mark.parametrize("kind", KINDS)
def test_pointer_errors_need_no_device(lib, kind):
    L = item_len_of(kind)
    shape = dict(n_old=1000, n_new=990, cap=1000, item_len=L, k_rm=10, first=3)
    bad = [("null items", b"null pointer", dict(items=0)),
           ("null root", b"null pointer", dict(root=0)),
           ("null workspace", b"null pointer", dict(d_ws=0)),
           ("null levels", b"null level array", dict(levels=0)),
           ("misaligned levels", b"misaligned", dict(levels=P + 8)),
           ("misaligned root", b"misaligned", dict(root=P + 2)),
           ("misaligned workspace", b"misaligned", dict(d_ws=P + 4)),
           ("null index array", b"index array", dict(rm=0)),
           ("misaligned index array", b"index array", dict(rm=P + 4))]
    if kind != "list":
        bad += [("null level 0", b"null pointer", dict(level0=0)), ("misaligned level 0", b"misaligned", dict(level0=P + 8))]
    if kind == "struct_list":
        bad += [("misaligned records", b"misaligned", dict(items=P + 2))]
    for what, text, kw in bad:
        rc, call = erase(lib, kind, **shape, **kw)
        assert rc == _lib.MK_EINVAL and text in call.err, f"{what}: {rc} {call.err}"
    # every pointer null: refused on any machine, with or without a device
    rc, call = erase(lib, kind, **shape, items=0, level0=0, levels=0, rm=0, root=0, d_ws=0)
    assert rc == _lib.MK_EINVAL


@pytest.mark.parametrize("kind", KINDS)
def test_update_entries_still_refuse_a_shrink(lib, kind):
    """The erase entries are the only way down: the update entries answer n_new < n_old as before."""
    call = _lib.Call(-1, 0, b"")
    if kind == "list":
        rc = lib.mk_dev_ssz_list_tree_update(ctypes.byref(call), None, 10, 9, 10, 32, None, None, 0, None, None, None,
                                             1 << 30, None)
        text = b"(a list tree does not shrink)"
    elif kind == "struct_list":
        rc = lib.mk_dev_ssz_struct_list_tree_update(ctypes.byref(call), None, 10, 9, 10, 160, _fields(VALIDATOR_FIELDS),
                                                    len(VALIDATOR_FIELDS), None, None, None, 0, None, None, None,
                                                    1 << 30, None)
        text = b"(a registry tree does not shrink)"
    else:
        rc = lib.mk_dev_ssz_bytes_list_tree_update(ctypes.byref(call), None, 10, 9, 10, 32, None, None, None, 0, None,
                                                   None, None, 1 << 30, None)
        text = b"(a bytes tree does not shrink)"
    assert rc == _lib.MK_EINVAL and text in call.err


@pytest.mark.parametrize("kind", KINDS)
def test_handle_entries_refuse_null(lib, kind):
    call = _lib.Call(-1, 0, b"")
    idx = (ctypes.c_uint64 * 2)(0, 1)
    trunc = getattr(lib, f"mk_{kind}_tree_truncate")
    er = getattr(lib, f"mk_{kind}_tree_erase")
    assert trunc(ctypes.byref(call), None, 0) == _lib.MK_EINVAL and b"null pointer" in call.err
    assert call.code == _lib.MK_EINVAL
    assert er(ctypes.byref(call), None, idx, 2) == _lib.MK_EINVAL and b"null pointer" in call.err
    assert er(ctypes.byref(call), None, None, 0) == _lib.MK_EINVAL


def test_set_entries_without_a_tree(lib):
    call = _lib.Call(-1, 0, b"")
    h = ctypes.c_void_p()
    assert lib.mk_tree_set_new(ctypes.byref(call), 64, ctypes.byref(h)) == _lib.MK_OK
    try:
        idx = (ctypes.c_uint64 * 1)(0)
        assert lib.mk_tree_set_truncate(ctypes.byref(call), h, 0, 0) == _lib.MK_EINVAL
        assert b"tree 0 of a set of 0" in call.err and call.code == _lib.MK_EINVAL
        assert lib.mk_tree_set_erase(ctypes.byref(call), h, 3, idx, 1) == _lib.MK_EINVAL
        assert b"tree 3 of a set of 0" in call.err
        assert lib.mk_tree_set_erase(ctypes.byref(call), h, 0, None, 0) == _lib.MK_EINVAL  # still no such tree
        assert lib.mk_tree_set_truncate(ctypes.byref(call), None, 0, 0) == _lib.MK_EINVAL
        assert b"null pointer" in call.err
        assert lib.mk_tree_set_erase(ctypes.byref(call), None, 0, idx, 1) == _lib.MK_EINVAL
        assert lib.mk_tree_set_erase(ctypes.byref(call), h, 0, None, 1) == _lib.MK_EINVAL
        assert b"null pointer" in call.err
    finally:
        lib.mk_tree_set_free(h)


def test_header_table_and_library_agree_on_the_new_entries(lib):
    want = {f"mk_ssz_{k}_tree_erase_workspace_bytes" for k in KINDS} | {f"mk_dev_ssz_{k}_tree_erase" for k in KINDS}
    want |= {f"mk_{k}_tree_{op}" for k in KINDS for op in ("truncate", "erase")}
    want |= {"mk_tree_set_truncate", "mk_tree_set_erase"}
    assert len(want) == 14
    names = set(_lib.header_symbols())
    for sym in sorted(want):
        assert sym in names and sym in _lib._SIGS and hasattr(lib, sym), sym
