"""Host-side logic of mk_dev_ssz_trees_update (several resident trees in one
call): the workspace query and every argument check, none of which needs a
device.  Every call here fails its checks, so nothing is ever launched and the
pointers are never dereferenced."""
import ctypes
import os
import re

import pytest

from prysm_amd import _lib
from prysm_amd import registry as R
from prysm_amd import state as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x10000  # a well-aligned non-NULL address; no call that gets past its checks uses it
LIST, STRUCT, BYTES = _lib.MK_TREE_LIST, _lib.MK_TREE_STRUCT, _lib.MK_TREE_BYTES
NOC = _lib.MK_NO_CONTAINER


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


_KEEP = []


def tree(kind=LIST, item_len=8, n_old=1000, n_new=None, cap=None, k=0, level0=None, spec=None, off=NOC, ptrs=True):
    t = _lib.TreeUpdate()
    n_new = n_old if n_new is None else n_new
    t.kind, t.item_len, t.n_old, t.n_new, t.capacity, t.k_idx = kind, item_len, n_old, n_new, \
        (max(n_new, 1) if cap is None else cap), k
    if ptrs:
        t.d_items, t.d_levels, t.d_root32, t.d_idx = P, P, P, (P if k else None)
        t.d_level0 = (P if kind != LIST else None) if level0 is None else (level0 or None)
    if kind == STRUCT:
        spec = R.VALIDATOR_FIELDS if spec is None else spec
        f = R._fields(spec)
        _KEEP.append(f)
        t.fields, t.nfields = ctypes.cast(f, ctypes.c_void_p), len(spec)
    t.container_off = off
    return t


def table(trees):
    arr = (_lib.TreeUpdate * max(len(trees), 1))()
    for i, t in enumerate(trees):
        arr[i] = t
    return arr


def ws_bytes(lib, trees):
    return lib.mk_ssz_trees_update_workspace_bytes(table(trees), len(trees))


def call(lib, trees, container_len=0, ws=1 << 40, d_ws=P, d_container=P, d_croot=P, ntrees=None):
    c = _lib.Call(-1, 0, b"")
    rc = lib.mk_dev_ssz_trees_update(ctypes.byref(c), table(trees), len(trees) if ntrees is None else ntrees,
                                     d_container, container_len, d_croot, d_ws, ws, None)
    return rc, c


def einval(lib, what, trees, **kw):
    rc, c = call(lib, trees, **kw)
    assert rc == _lib.MK_EINVAL and c.code == rc and c.err != b"", (what, rc, c.err)


def test_header_and_bindings_declare_the_entry():
    names = set(_lib.header_symbols())
    for sym in ("mk_ssz_trees_update_workspace_bytes", "mk_dev_ssz_trees_update"):
        assert sym in names and sym in _lib._SIGS, sym
    txt = open(_lib.HEADER).read()
    for name in ("MK_TREE_LIST", "MK_TREE_STRUCT", "MK_TREE_BYTES", "MK_TREES_MAX", "MK_CONTAINER_MAX"):
        assert int(re.search(rf"#define {name}\s+(\d+)", txt).group(1)) == getattr(_lib, name), name
    assert int(re.search(r"#define MK_NO_CONTAINER\s+(0x[0-9a-f]+)u", txt).group(1), 16) == _lib.MK_NO_CONTAINER
    # mk_tree_update as the C compiler lays it out: 8-B aligned members, no padding surprises
    assert ctypes.sizeof(_lib.TreeUpdate) == 104 and _lib.TreeUpdate.d_root32.offset == 96
    assert _lib.TreeUpdate.container_off.offset == 92 and _lib.TreeUpdate.n_old.offset == 32


def test_rebuild_shares_are_the_handles_own():
    """ResidentBeaconState rebuilds at the dirty share at which each kind's host handle does."""
    for name, src in (("LIST", "list_tree_api.cpp"), ("STRUCT", "struct_tree_api.cpp"), ("BYTES", "bytes_tree_api.cpp")):
        txt = open(os.path.join(ROOT, "prysm_amd", "csrc", src)).read()
        div = int(re.search(rf"#define MK_{name}_TREE_REBUILD_DIV\s+(\d+)", txt).group(1))
        assert getattr(_lib, f"{name}_TREE_REBUILD_DIV") == div
    assert ST._REBUILD_DIV == {LIST: 512, STRUCT: 32, BYTES: 256}
    assert ST.CONTAINER_LEN == 536 and all(off % 8 == 0 for off in ST.CONTAINER_OFF.values())


def test_workspace_query_covers_every_kind(lib):
    vf, nvf = R._fields(R.VALIDATOR_FIELDS), len(R.VALIDATOR_FIELDS)
    af, naf = R._fields(ST.PENDING_ATTESTATION_FIELDS), len(ST.PENDING_ATTESTATION_FIELDS)
    prev = 0
    for k in (0, 1, 3, 100, 4099, 1 << 20):
        own = [lib.mk_ssz_list_tree_update_workspace_bytes(k),
               lib.mk_ssz_struct_list_tree_update_workspace_bytes(k, vf, nvf),
               lib.mk_ssz_struct_list_tree_update_workspace_bytes(k, af, naf),
               lib.mk_ssz_bytes_list_tree_update_workspace_bytes(k, 32)]
        trees = [tree(LIST, 8, 1 << 21, k=k), tree(STRUCT, 160, 1 << 21, k=k),
                 tree(STRUCT, ST.pending_attestation_record_len(48), 1 << 21, k=k, spec=ST.PENDING_ATTESTATION_FIELDS),
                 tree(BYTES, 32, 1 << 21, k=k)]
        for t, w in zip(trees, own):
            one = ws_bytes(lib, [t])
            assert one >= w + 4 and one % 16 == 0, k  # its own workspace and the container's counter
        ws = ws_bytes(lib, trees)
        assert ws >= sum(own) + 4 and ws % 16 == 0 and ws >= prev, k
        prev = ws
    # appended items are work items too
    assert ws_bytes(lib, [tree(LIST, 8, 1000, 1000 + (1 << 16), cap=1 << 20)]) >= 8 << 16
    assert ws_bytes(lib, [tree(LIST, 8, 1000)] * 16) >= 16 * lib.mk_ssz_list_tree_update_workspace_bytes(0)
    # a list of trees the call refuses has no size
    assert ws_bytes(lib, []) == 0
    assert lib.mk_ssz_trees_update_workspace_bytes(table([tree()] * 16), 17) == 0
    assert ws_bytes(lib, [tree(kind=7)]) == 0
    assert ws_bytes(lib, [tree(LIST, 0)]) == 0
    assert ws_bytes(lib, [tree(BYTES, 32, 10, 9)]) == 0


def test_tree_count_and_kind(lib):
    einval(lib, "ntrees == 0", [])
    rc, c = call(lib, [tree()] * 16, ntrees=17)
    assert rc == _lib.MK_EINVAL and c.err != b""
    einval(lib, "unknown kind 0", [tree(kind=0)])
    einval(lib, "unknown kind 4", [tree(), tree(kind=4)])


@pytest.mark.parametrize("kind,item_len", [(LIST, 8), (STRUCT, 160), (BYTES, 32)])
def test_each_kinds_own_checks(lib, kind, item_len):
    einval(lib, "item_len == 0", [tree(kind, 0)])
    einval(lib, "n_new < n_old", [tree(kind, item_len, 10, 9, cap=10)])
    einval(lib, "n_new > capacity", [tree(kind, item_len, 10, 11, cap=10)])
    einval(lib, "k >= 2^31", [tree(kind, item_len, 10, k=1 << 31)])
    einval(lib, "k + appended >= 2^31", [tree(kind, item_len, 10, 10 + (1 << 30), cap=1 << 40, k=1 << 30)])
    einval(lib, "capacity * item_len overflows", [tree(kind, item_len, 10, cap=1 << 62)])
    # the bad tree need not be the first
    einval(lib, "second tree", [tree(), tree(kind, item_len, 10, 9, cap=10)])


def test_bad_field_layouts(lib):
    einval(lib, "no fields", [tree(STRUCT, 160, spec=[])])
    einval(lib, "field beyond the record", [tree(STRUCT, 160, spec=[(_lib.MK_FIELD_RAW, 156, 8)])])
    einval(lib, "unknown field kind", [tree(STRUCT, 160, spec=[(9, 0, 8)])])
    t = tree(STRUCT, 160)
    t.fields = None
    einval(lib, "null fields", [t])


def test_level0_must_match_the_kind(lib):
    einval(lib, "LIST with a d_level0", [tree(LIST, 8, level0=P)])
    einval(lib, "STRUCT without d_level0", [tree(STRUCT, 160, level0=0)])
    einval(lib, "BYTES without d_level0", [tree(BYTES, 32, level0=0)])
    einval(lib, "BYTES without d_level0, behind good trees", [tree(), tree(STRUCT, 160), tree(BYTES, 32, level0=0)])
    # ... and the other pointers, where the single-tree entries check theirs
    t = tree()
    t.d_root32 = None
    einval(lib, "null root", [t])
    t = tree()
    t.d_levels = P + 8
    einval(lib, "misaligned levels", [t])
    t = tree(k=3)
    t.d_idx = None
    einval(lib, "null index array", [t])
    einval(lib, "null workspace", [tree()], d_ws=None)
    einval(lib, "workspace not 16-B aligned", [tree()], d_ws=P + 8)


def test_container_checks(lib):
    ten = [tree(off=32 * i) for i in range(10)]
    einval(lib, "container_len above the maximum", ten, container_len=_lib.MK_CONTAINER_MAX + 1)
    einval(lib, "offset not 4-B aligned", [tree(off=2)], container_len=536)
    einval(lib, "offset not 4-B aligned (odd)", [tree(off=0), tree(off=41)], container_len=536)
    einval(lib, "root beyond the container", [tree(off=508)], container_len=536)
    einval(lib, "root beyond a short container", [tree(off=0)], container_len=31)
    einval(lib, "root in no container", [tree(off=0)], container_len=0)
    einval(lib, "equal offsets", [tree(off=64), tree(off=64)], container_len=536)
    einval(lib, "overlap from below", [tree(off=64), tree(BYTES, 32, off=36)], container_len=536)
    einval(lib, "overlap from above", [tree(off=64), tree(), tree(STRUCT, 160, off=92)], container_len=536)
    einval(lib, "no participating tree", [tree(), tree(BYTES, 32)], container_len=536)
    einval(lib, "null container", [tree(off=0)], container_len=536, d_container=None)
    einval(lib, "null container root", [tree(off=0)], container_len=536, d_croot=None)
    einval(lib, "misaligned container", [tree(off=0)], container_len=536, d_container=P + 2)


def test_short_workspace(lib):
    trees = [tree(LIST, 8, 1000, 1024, cap=2000, k=500), tree(STRUCT, 160, 5000, k=70), tree(BYTES, 32, 8192, k=1)]
    need = ws_bytes(lib, trees)
    assert need > 0
    for ws in (0, 64, need - 1):
        rc, c = call(lib, trees, ws=ws)
        assert rc == _lib.MK_ENOMEM and c.code == rc and b"workspace" in c.err, ws
    rc, c = call(lib, [t for t in trees] + [tree(off=0)], container_len=536, ws=need - 1)
    assert rc == _lib.MK_ENOMEM
    # a bad shape or container is reported before a short workspace; the pointers are not looked at yet
    rc, c = call(lib, [tree(LIST, 8, 10, 9, cap=10, ptrs=False)], ws=0, d_ws=None)
    assert rc == _lib.MK_EINVAL
    rc, c = call(lib, [tree(off=2, ptrs=False)], container_len=536, ws=0, d_ws=None)
    assert rc == _lib.MK_EINVAL
    rc, c = call(lib, [tree(ptrs=False)], ws=0, d_ws=None)
    assert rc == _lib.MK_ENOMEM
