"""Host-side logic of the registry tree entry points (mk_*struct_list_tree*):
the workspace queries and the argument checks that need no device."""
import ctypes
import os

import pytest

from prysm_amd import _lib

B, R = _lib.MK_FIELD_BYTES, _lib.MK_FIELD_RAW
V_FIELDS = [(B, 0, 48), (B, 48, 32), (B, 80, 32)] + [(R, 112 + 8 * k, 8) for k in range(6)]  # 160-B records
G_FIELDS = [(B, 0, 96), (R, 96, 8), (R, 104, 2)]  # 108-B records: struct roots in two launches


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _f(spec):
    arr = (_lib.Field * len(spec))()
    for i, (k, o, n) in enumerate(spec):
        arr[i].kind, arr[i].offset, arr[i].len = k, o, n
    return arr


@pytest.mark.parametrize("spec", [V_FIELDS, G_FIELDS])
def test_workspace_queries(lib, spec):
    f = _f(spec)
    prev = 0
    for k in (0, 1, 2, 31, 32, 33, 1000, 1 << 20, (1 << 20) + 1):
        ws = lib.mk_ssz_struct_list_tree_update_workspace_bytes(k, f, len(spec))
        assert ws >= prev and ws >= 8 * k + 32 * k and ws > 0, k
        prev = ws
    prev = 0
    for n in (0, 1, 5, 1000, 1 << 20):
        ws = lib.mk_ssz_struct_list_tree_build_workspace_bytes(n, f, len(spec))
        assert ws >= prev and ws > 0, n
        prev = ws
    assert lib.mk_ssz_struct_list_tree_update_workspace_bytes(1, None, 0) == 0  # no layout, no size


def _update(lib, n_old, n_new, cap, record_len=160, spec=V_FIELDS, ws_bytes=1 << 30, k=0):
    call = _lib.Call(-1, 0, b"")
    rc = lib.mk_dev_ssz_struct_list_tree_update(ctypes.byref(call), None, n_old, n_new, cap, record_len, _f(spec),
                                                len(spec), None, None, None, k, None, None, None, ws_bytes, None)
    return rc, call


def _build(lib, n, cap, record_len=160, spec=V_FIELDS, ws_bytes=1 << 30):
    call = _lib.Call(-1, 0, b"")
    rc = lib.mk_dev_ssz_struct_list_tree_build(ctypes.byref(call), None, n, cap, record_len, _f(spec), len(spec),
                                               None, None, None, None, ws_bytes, None)
    return rc, call


def test_update_argument_checks_need_no_device(lib):
    for what, kw in (("n_new < n_old", dict(n_old=10, n_new=9, cap=10)),
                     ("n_new > capacity", dict(n_old=10, n_new=11, cap=10)),
                     ("k >= 2^31", dict(n_old=10, n_new=10, cap=10, k=1 << 31)),
                     ("record_len % 4", dict(n_old=10, n_new=10, cap=10, record_len=110, spec=G_FIELDS)),
                     ("field past the record", dict(n_old=10, n_new=10, cap=10, record_len=104, spec=G_FIELDS)),
                     ("record_len == 0", dict(n_old=10, n_new=10, cap=10, record_len=0))):
        rc, call = _update(lib, **kw)
        assert rc == _lib.MK_EINVAL and call.code == rc and call.err != b"", what
    rc, call = _update(lib, 1000, 1000, 1000, ws_bytes=64, k=500)
    assert rc == _lib.MK_ENOMEM and call.code == rc and b"workspace" in call.err
    need = lib.mk_ssz_struct_list_tree_update_workspace_bytes(500, _f(G_FIELDS), len(G_FIELDS))
    rc, call = _update(lib, 1000, 1000, 1000, record_len=108, spec=G_FIELDS, ws_bytes=need - 1, k=500)
    assert rc == _lib.MK_ENOMEM and b"workspace" in call.err


def test_build_argument_checks_need_no_device(lib):
    for what, kw in (("n > capacity", dict(n=11, cap=10)),
                     ("record_len % 4", dict(n=10, cap=10, record_len=110, spec=G_FIELDS)),
                     ("field past the record", dict(n=10, cap=10, record_len=104, spec=G_FIELDS)),
                     ("record_len == 0", dict(n=10, cap=10, record_len=0))):
        rc, call = _build(lib, **kw)
        assert rc == _lib.MK_EINVAL and call.code == rc and call.err != b"", what
    need = lib.mk_ssz_struct_list_tree_build_workspace_bytes(1000, _f(G_FIELDS), len(G_FIELDS))
    rc, call = _build(lib, 1000, 1000, record_len=108, spec=G_FIELDS, ws_bytes=need - 1)
    assert rc == _lib.MK_ENOMEM and call.code == rc and b"workspace" in call.err
    rc, call = _build(lib, 1000, 1000, ws_bytes=0)
    assert rc == _lib.MK_ENOMEM


def test_handle_needs_a_device(lib):
    call = _lib.Call(-1, 0, b"")
    h = ctypes.c_void_p()
    if _lib.device_count() == 0:
        rc = lib.mk_struct_list_tree_new(ctypes.byref(call), 160, _f(V_FIELDS), len(V_FIELDS), 10, ctypes.byref(h))
        assert rc == _lib.MK_ENODEV and call.code == rc and not h.value
    rc = lib.mk_struct_list_tree_new(ctypes.byref(call), 110, _f(G_FIELDS), len(G_FIELDS), 10, ctypes.byref(h))
    assert rc == _lib.MK_EINVAL and not h.value  # a bad layout is refused before the device is looked up
    assert lib.mk_struct_list_tree_count(None) == 0
    lib.mk_struct_list_tree_free(None)
