"""Host-side logic of the bytes tree entry points (mk_*bytes_list_tree*): the
workspace queries and the argument checks that need no device."""
import ctypes
import os

import pytest

from prysm_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


@pytest.mark.parametrize("elem_len", [1, 32, 48, 300])
def test_workspace_queries(lib, elem_len):
    prev = 0
    for k in (0, 1, 2, 31, 32, 33, 1000, 1 << 20, (1 << 20) + 1):
        ws = lib.mk_ssz_bytes_list_tree_update_workspace_bytes(k, elem_len)
        assert ws >= prev and ws >= 8 * k and ws > 0, k  # one arrival word per work item
        prev = ws
    prev = 0
    for n in (0, 1, 5, 1000, 1 << 20, 1 << 28):
        ws = lib.mk_ssz_bytes_list_tree_build_workspace_bytes(n, elem_len)
        assert ws >= prev and ws > 0, n
        prev = ws


def test_workspace_queries_refuse_empty_elements(lib):
    assert lib.mk_ssz_bytes_list_tree_update_workspace_bytes(1, 0) == 0  # no tree of 0-byte elements, no size
    assert lib.mk_ssz_bytes_list_tree_build_workspace_bytes(1, 0) == 0


def _update(lib, n_old, n_new, cap, elem_len=32, ws_bytes=1 << 30, k=0):
    call = _lib.Call(-1, 0, b"")
    rc = lib.mk_dev_ssz_bytes_list_tree_update(ctypes.byref(call), None, n_old, n_new, cap, elem_len, None, None,
                                               None, k, None, None, None, ws_bytes, None)
    return rc, call


def _build(lib, n, cap, elem_len=32, ws_bytes=1 << 30):
    call = _lib.Call(-1, 0, b"")
    rc = lib.mk_dev_ssz_bytes_list_tree_build(ctypes.byref(call), None, n, cap, elem_len, None, None, None, None,
                                              ws_bytes, None)
    return rc, call


def test_update_argument_checks_need_no_device(lib):
    for what, kw in (("elem_len == 0", dict(n_old=10, n_new=10, cap=10, elem_len=0)),
                     ("elem_len > 2^30", dict(n_old=10, n_new=10, cap=10, elem_len=(1 << 30) + 1)),
                     ("n_new < n_old", dict(n_old=10, n_new=9, cap=10)),
                     ("n_new > capacity", dict(n_old=10, n_new=11, cap=10)),
                     ("capacity * elem_len overflows", dict(n_old=10, n_new=10, cap=1 << 62, elem_len=48)),
                     ("capacity * 32 overflows", dict(n_old=10, n_new=10, cap=1 << 60, elem_len=1)),
                     ("k >= 2^31", dict(n_old=10, n_new=10, cap=10, k=1 << 31)),
                     ("k + appended >= 2^31", dict(n_old=10, n_new=10 + (1 << 30), cap=1 << 40, k=1 << 30))):
        rc, call = _update(lib, **kw)
        assert rc == _lib.MK_EINVAL and call.code == rc and call.err != b"", what
    rc, call = _update(lib, 1000, 1000, 1000, ws_bytes=64, k=500)
    assert rc == _lib.MK_ENOMEM and call.code == rc and b"workspace" in call.err
    for elem_len in (32, 132):
        need = lib.mk_ssz_bytes_list_tree_update_workspace_bytes(500 + 24, elem_len)
        rc, call = _update(lib, 1000, 1024, 2000, elem_len=elem_len, ws_bytes=need - 1, k=500)
        assert rc == _lib.MK_ENOMEM and b"workspace" in call.err
    # a bad shape is reported before a short workspace
    rc, call = _update(lib, 10, 9, 10, ws_bytes=0)
    assert rc == _lib.MK_EINVAL


def test_build_argument_checks_need_no_device(lib):
    for what, kw in (("elem_len == 0", dict(n=10, cap=10, elem_len=0)),
                     ("n > capacity", dict(n=11, cap=10)),
                     ("capacity * elem_len overflows", dict(n=10, cap=1 << 62, elem_len=48))):
        rc, call = _build(lib, **kw)
        assert rc == _lib.MK_EINVAL and call.code == rc and call.err != b"", what
    need = lib.mk_ssz_bytes_list_tree_build_workspace_bytes(1000, 32)
    rc, call = _build(lib, 1000, 1000, ws_bytes=need - 1)
    assert rc == _lib.MK_ENOMEM and call.code == rc and b"workspace" in call.err
    rc, call = _build(lib, 1000, 1000, ws_bytes=0)
    assert rc == _lib.MK_ENOMEM


def test_handle_needs_a_device(lib):
    call = _lib.Call(-1, 0, b"")
    h = ctypes.c_void_p()
    if _lib.device_count() == 0:
        rc = lib.mk_bytes_list_tree_new(ctypes.byref(call), 32, 10, ctypes.byref(h))
        assert rc == _lib.MK_ENODEV and call.code == rc and not h.value
    rc = lib.mk_bytes_list_tree_new(ctypes.byref(call), 0, 10, ctypes.byref(h))
    assert rc == _lib.MK_EINVAL and not h.value  # elem_len == 0 is refused before the device is looked up
    assert lib.mk_bytes_list_tree_count(None) == 0
    lib.mk_bytes_list_tree_free(None)


def test_header_declares_the_entry_points():
    names = set(_lib.header_symbols())
    for sym in ("mk_ssz_bytes_list_tree_build_workspace_bytes", "mk_dev_ssz_bytes_list_tree_build",
                "mk_ssz_bytes_list_tree_update_workspace_bytes", "mk_dev_ssz_bytes_list_tree_update",
                "mk_bytes_list_tree_new", "mk_bytes_list_tree_free", "mk_bytes_list_tree_count",
                "mk_bytes_list_tree_assign", "mk_bytes_list_tree_update", "mk_bytes_list_tree_append",
                "mk_bytes_list_tree_root", "mk_bytes_list_tree_elems"):
        assert sym in names and sym in _lib._SIGS, sym
