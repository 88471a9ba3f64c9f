"""Host-side logic of the list tree entry points: the level-array layout, the
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


def _layout_bytes(capacity, item_len):
    if item_len == 0:
        return 0
    per = 128 // item_len if item_len < 128 else 1
    c = -(-capacity // per)
    total = 0
    while c > 1:
        c = (c + 1) // 2
        total += c
    return 32 * total


@pytest.mark.parametrize("item_len", [1, 8, 32, 48, 128, 200])
@pytest.mark.parametrize("cap_chunks", [0, 1, 2, 3, 5, 1000, (1 << 20) + 1])
def test_levels_bytes_is_the_layout(lib, item_len, cap_chunks):
    per = 128 // item_len if item_len < 128 else 1
    for capacity in {cap_chunks * per, max(cap_chunks * per - (per - 1), 0)}:
        assert lib.mk_ssz_list_tree_levels_bytes(capacity, item_len) == _layout_bytes(capacity, item_len)
    if cap_chunks <= 1:
        assert lib.mk_ssz_list_tree_levels_bytes(cap_chunks * per, item_len) == 0
    assert lib.mk_ssz_list_tree_levels_bytes(cap_chunks * per, 0) == 0


def test_levels_bytes_examples(lib):
    assert lib.mk_ssz_list_tree_levels_bytes(5 * 4, 32) == 32 * (3 + 2 + 1)
    assert lib.mk_ssz_list_tree_levels_bytes(3, 200) == 32 * (2 + 1)
    assert lib.mk_ssz_list_tree_levels_bytes(2 * 2, 48) == 32 * 1


def test_workspace_queries(lib):
    prev = 0
    for k in (0, 1, 2, 31, 32, 33, 1000, 1 << 20, (1 << 20) + 1):
        ws = lib.mk_ssz_list_tree_update_workspace_bytes(k)
        assert ws >= prev and ws >= 8 * k
        if k >= 1:
            assert ws > 0
        prev = ws
    prev = 0
    for n in (0, 1, 5, 1000, 1 << 24):
        ws = lib.mk_ssz_list_tree_build_workspace_bytes(n, 32)
        assert ws >= prev and ws > 0
        prev = ws


def _update(lib, n_old, n_new, cap, item_len, ws_bytes=1 << 20, k=0):
    call = _lib.Call(-1, 0, b"")
    rc = lib.mk_dev_ssz_list_tree_update(ctypes.byref(call), None, n_old, n_new, cap, item_len, None, None, k, None,
                                         None, None, ws_bytes, None)
    return rc, call


def test_argument_checks_need_no_device(lib):
    for args in ((10, 9, 10, 32), (10, 11, 10, 32), (10, 10, 10, 0)):
        rc, call = _update(lib, *args)
        assert rc == _lib.MK_EINVAL and call.code == rc and call.err != b"", args
    rc, call = _update(lib, 1000, 1000, 1000, 32, ws_bytes=64, k=500)
    assert rc == _lib.MK_ENOMEM and call.code == rc and b"workspace" in call.err
    call = _lib.Call(-1, 0, b"")
    rc = lib.mk_dev_ssz_list_tree_build(ctypes.byref(call), None, 11, 10, 32, None, None, None, 1 << 20, None)
    assert rc == _lib.MK_EINVAL and call.err != b""
    rc = lib.mk_dev_ssz_list_tree_build(ctypes.byref(call), None, 10, 10, 0, None, None, None, 1 << 20, None)
    assert rc == _lib.MK_EINVAL and call.err == b"item_len == 0"
    h = ctypes.c_void_p()
    rc = lib.mk_list_tree_new(ctypes.byref(call), 0, 10, ctypes.byref(h))
    assert rc == _lib.MK_EINVAL and not h.value


def test_handle_needs_a_device(lib):
    if _lib.device_count() == 0:
        call = _lib.Call(-1, 0, b"")
        h = ctypes.c_void_p()
        rc = lib.mk_list_tree_new(ctypes.byref(call), 32, 10, ctypes.byref(h))
        assert rc == _lib.MK_ENODEV and call.code == rc and not h.value
    assert lib.mk_list_tree_count(None) == 0
    lib.mk_list_tree_free(None)
