"""Host-side argument checks of mk_tree_set (a set of resident trees behind
one handle): every MK_EINVAL of new, add and put that is decided before a
device is needed.  mk_tree_set_new needs no device, so a set exists on any
machine; an add that passes its checks then needs one (MK_ENODEV without).
(The 17th tree, overlapping roots and a put into a root range need trees in
the set, hence a device: tests/test_gpu_tree_set.py.)"""
import ctypes
import os

import pytest

from prysm_amd import _lib
from prysm_amd import registry as R
from prysm_amd import state as ST

LIST, STRUCT, BYTES = _lib.MK_TREE_LIST, _lib.MK_TREE_STRUCT, _lib.MK_TREE_BYTES
NOC = _lib.MK_NO_CONTAINER


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


@pytest.fixture()
def tset(lib):
    h = ctypes.c_void_p()
    call = _lib.Call(-1, 0, b"")
    assert lib.mk_tree_set_new(ctypes.byref(call), 536, ctypes.byref(h)) == _lib.MK_OK
    yield h
    lib.mk_tree_set_free(h)


def add(lib, h, kind=LIST, item_len=8, fields=None, nfields=None, capacity=0, off=NOC):
    call = _lib.Call(-1, 0, b"")
    out = ctypes.c_uint32(77)
    f = R._fields(fields) if fields is not None else None
    n = (len(fields) if fields is not None else 0) if nfields is None else nfields
    rc = lib.mk_tree_set_add(ctypes.byref(call), h, kind, item_len, f, n, capacity, off, ctypes.byref(out))
    return rc, call.err.decode(), out.value


def test_header_declares_the_set(lib):
    want = {"mk_tree_set_new", "mk_tree_set_free", "mk_tree_set_add", "mk_tree_set_put", "mk_tree_set_assign",
            "mk_tree_set_update", "mk_tree_set_append", "mk_tree_set_count", "mk_tree_set_root",
            "mk_tree_set_tree_root", "mk_tree_set_items"}
    assert want <= set(_lib.header_symbols())
    assert want <= set(_lib._SIGS)
    for s in want:
        assert hasattr(lib, s), s


def test_new_checks(lib):
    call = _lib.Call(-1, 0, b"")
    h = ctypes.c_void_p(1)
    assert lib.mk_tree_set_new(ctypes.byref(call), _lib.MK_CONTAINER_MAX + 1, ctypes.byref(h)) == _lib.MK_EINVAL
    assert h.value is None and b"container" in call.err
    assert lib.mk_tree_set_new(ctypes.byref(call), 0, None) == _lib.MK_EINVAL
    for n in (0, _lib.MK_CONTAINER_MAX):
        assert lib.mk_tree_set_new(ctypes.byref(call), n, ctypes.byref(h)) == _lib.MK_OK
        assert lib.mk_tree_set_count(h, 0) == 0
        lib.mk_tree_set_free(h)
    lib.mk_tree_set_free(None)


@pytest.mark.parametrize("what,kw", [
    ("unknown kind 0", dict(kind=0)),
    ("unknown kind 4", dict(kind=4)),
    ("fields for a list tree", dict(kind=LIST, fields=ST.CROSSLINK_FIELDS)),
    ("fields for a bytes tree", dict(kind=BYTES, item_len=32, fields=ST.CROSSLINK_FIELDS)),
    ("a field count without fields", dict(kind=LIST, nfields=2)),
    ("a struct tree without fields", dict(kind=STRUCT, item_len=40)),
    ("a struct tree with zero fields", dict(kind=STRUCT, item_len=40, fields=[])),
    ("list item_len 0", dict(kind=LIST, item_len=0)),
    ("bytes elem_len 0", dict(kind=BYTES, item_len=0)),
    ("bytes elem_len above 2^30", dict(kind=BYTES, item_len=(1 << 30) + 1)),
    ("struct record_len 0", dict(kind=STRUCT, item_len=0, fields=ST.CROSSLINK_FIELDS)),
    ("a field beyond the record", dict(kind=STRUCT, item_len=36, fields=ST.CROSSLINK_FIELDS)),
    ("an unknown field kind", dict(kind=STRUCT, item_len=40, fields=[(9, 0, 8)])),
    ("capacity * item_len overflows", dict(kind=LIST, item_len=16, capacity=1 << 61)),
    ("bytes capacity overflows", dict(kind=BYTES, item_len=1, capacity=1 << 60)),
    ("struct capacity overflows", dict(kind=STRUCT, item_len=40, fields=ST.CROSSLINK_FIELDS, capacity=1 << 60)),
    ("container offset not 4-byte aligned", dict(off=2)),
    ("root leaves the message", dict(off=508)),
    ("root far outside the message", dict(off=0xFFFFFFF0)),
])
def test_add_einval_before_any_device(lib, tset, what, kw):
    rc, err, out = add(lib, tset, **kw)
    assert rc == _lib.MK_EINVAL, f"{what}: {rc} {err}"
    assert err, what
    assert lib.mk_tree_set_count(tset, 0) == 0, f"{what}: a tree was added"


def test_add_null_pointers(lib, tset):
    call = _lib.Call(-1, 0, b"")
    out = ctypes.c_uint32()
    assert lib.mk_tree_set_add(ctypes.byref(call), None, LIST, 8, None, 0, 0, NOC, ctypes.byref(out)) == _lib.MK_EINVAL
    assert lib.mk_tree_set_add(ctypes.byref(call), tset, LIST, 8, None, 0, 0, NOC, None) == _lib.MK_EINVAL


def test_a_good_add_gets_past_the_checks(lib, tset):
    """MK_OK with a device, MK_ENODEV without: never MK_EINVAL."""
    for kw in (dict(kind=LIST, item_len=8, off=40), dict(kind=BYTES, item_len=32, off=504),
               dict(kind=STRUCT, item_len=40, fields=ST.CROSSLINK_FIELDS, off=0), dict(kind=LIST, item_len=5)):
        rc, err, _ = add(lib, tset, **kw)
        assert rc in (_lib.MK_OK, _lib.MK_ENODEV), f"{kw}: {rc} {err}"


def test_no_container_takes_no_offset(lib):
    call = _lib.Call(-1, 0, b"")
    h = ctypes.c_void_p()
    assert lib.mk_tree_set_new(ctypes.byref(call), 0, ctypes.byref(h)) == _lib.MK_OK
    try:
        rc, err, _ = add(lib, h, off=0)
        assert rc == _lib.MK_EINVAL and "container" in err
        root = ctypes.create_string_buffer(32)
        assert lib.mk_tree_set_root(ctypes.byref(call), h, root) == _lib.MK_EINVAL  # no container, on any machine
    finally:
        lib.mk_tree_set_free(h)


@pytest.mark.parametrize("off,n", [(536, 1), (530, 8), (0, 537), (0xFFFFFFFF, 1), (0xFFFFFFFF, 0xFFFFFFFF), (537, 0)])
def test_put_outside_the_message(lib, tset, off, n):
    call = _lib.Call(-1, 0, b"")
    buf = ctypes.create_string_buffer(8)  # never read: the range is refused first
    assert lib.mk_tree_set_put(ctypes.byref(call), tset, off, buf, n) == _lib.MK_EINVAL
    assert b"container" in call.err


def test_put_inside_and_null(lib, tset):
    call = _lib.Call(-1, 0, b"")
    buf = ctypes.create_string_buffer(b"\x01" * 8, 8)
    assert lib.mk_tree_set_put(ctypes.byref(call), tset, 528, buf, 8) == _lib.MK_OK
    assert lib.mk_tree_set_put(ctypes.byref(call), tset, 536, None, 0) == _lib.MK_OK
    assert lib.mk_tree_set_put(ctypes.byref(call), tset, 0, None, 8) == _lib.MK_EINVAL
    assert lib.mk_tree_set_put(ctypes.byref(call), None, 0, buf, 8) == _lib.MK_EINVAL
    root = ctypes.create_string_buffer(32)
    assert lib.mk_tree_set_root(ctypes.byref(call), tset, root) == _lib.MK_EINVAL  # no tree takes part yet
    assert b"no tree" in call.err


def test_calls_on_a_tree_that_is_not_there(lib, tset):
    call = _lib.Call(-1, 0, b"")
    buf = ctypes.create_string_buffer(32)
    idx = (ctypes.c_uint64 * 1)(0)
    assert lib.mk_tree_set_update(ctypes.byref(call), tset, 0, idx, buf, 1) == _lib.MK_EINVAL
    assert lib.mk_tree_set_append(ctypes.byref(call), tset, 3, buf, 1) == _lib.MK_EINVAL
    assert lib.mk_tree_set_assign(ctypes.byref(call), tset, 0, buf, 1) == _lib.MK_EINVAL
    assert lib.mk_tree_set_tree_root(ctypes.byref(call), tset, 0, buf) == _lib.MK_EINVAL
    assert lib.mk_tree_set_items(ctypes.byref(call), tset, 0, 0, 0, buf) == _lib.MK_EINVAL
    assert lib.mk_tree_set_count(tset, 5) == 0
