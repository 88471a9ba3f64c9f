"""Host-side logic of the nested struct layouts (MK_FIELD_STRUCT,
MK_FIELD_VARBYTES): mk_ssz_struct_msg_len and every check of a layout, which
all run before a device is looked up (prysm_amd/csrc/struct_spec.cpp)."""
import ctypes
import os

import pytest

from prysm_amd import _lib
from prysm_amd import state as ST

B, R, V, S = _lib.MK_FIELD_BYTES, _lib.MK_FIELD_RAW, _lib.MK_FIELD_VARBYTES, _lib.MK_FIELD_STRUCT

FLAT = [(B, 0, 48), (B, 48, 32), (R, 80, 8)]                                   # 32 + 32 + 8
FLAT_VAR = [(R, 0, 8), (V, 8, 20), (B, 32, 32)]                                # 8 + 32 + 32, 64-B records
ONE_LEVEL = [(S, 0, 2), (B, 0, 32), (B, 32, 32), (R, 64, 8)]                   # Eth1DataVote: top 40, nested 64
TWO_LEVEL = [(R, 0, 8), (S, 0, 5), (B, 8, 32), (S, 0, 2), (R, 40, 8), (R, 48, 2), (R, 50, 1),
             (V, 52, 8)]                                                       # top 72, mid 65, inner 10


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


def _build(lib, spec, record_len, n=10, cap=10, ws_bytes=1 << 30):
    call = _lib.Call(-1, 0, b"")
    rc = lib.mk_dev_ssz_struct_list_tree_build(ctypes.byref(call), None, n, cap, record_len, _f(spec), len(spec),
                                               None, None, None, None, ws_bytes, None)
    return rc, call


def test_msg_len(lib):
    assert lib.mk_ssz_struct_msg_len(_f(FLAT), len(FLAT)) == 72           # flat: as before
    assert lib.mk_ssz_struct_msg_len(_f(FLAT_VAR), len(FLAT_VAR)) == 72   # no nested struct: the message itself
    assert lib.mk_ssz_struct_msg_len(_f(ONE_LEVEL), len(ONE_LEVEL)) == 40 + 64
    assert lib.mk_ssz_struct_msg_len(_f(TWO_LEVEL), len(TWO_LEVEL)) == 72 + 65 + 10
    att = ST.PENDING_ATTESTATION_FIELDS
    assert len(att) == 13
    assert lib.mk_ssz_struct_msg_len(_f(att), len(att)) == 104 + 192
    assert lib.mk_ssz_struct_msg_len(_f(ST.ETH1_VOTE_FIELDS), len(ST.ETH1_VOTE_FIELDS)) == 104
    assert lib.mk_ssz_struct_msg_len(_f(ST.CROSSLINK_FIELDS), len(ST.CROSSLINK_FIELDS)) == 40


DEPTH5 = [(S, 0, 4), (S, 0, 3), (S, 0, 2), (S, 0, 1), (R, 0, 8)]   # top + 4 nested levels
DEPTH4 = [(S, 0, 3), (S, 0, 2), (S, 0, 1), (R, 0, 8)]
LDS_PEAK = [(B, 32 * k, 32) for k in range(16)] + [(V, 512, 4)]    # a 544-B message: above the 320-B limit

MALFORMED = [
    ("child count past the end", [(R, 0, 8), (S, 0, 3), (R, 8, 8), (R, 16, 8)], 64),
    ("child count past the parent", [(S, 0, 2), (S, 0, 2), (R, 0, 8), (R, 8, 8)], 64),
    ("depth 5", DEPTH5, 64),
    ("struct with a non-zero offset", [(S, 8, 1), (R, 8, 8)], 64),
    ("struct with len 0", [(R, 0, 8), (S, 0, 0)], 64),
    ("varbytes offset % 4 != 0", [(R, 0, 8), (V, 10, 8)], 64),
    ("varbytes slot past the record", [(R, 0, 8), (V, 8, 53)], 64),
    ("field of a nested struct past the record", [(S, 0, 1), (B, 40, 32)], 64),
    ("LDS peak", LDS_PEAK, 520),
    ("unknown kind", [(5, 0, 8)], 64),
]


@pytest.mark.parametrize("what,spec,record_len", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_specs_need_no_device(lib, what, spec, record_len):
    rc, call = _build(lib, spec, record_len)
    assert rc == _lib.MK_EINVAL and call.code == rc and call.err != b"", what
    assert lib.mk_ssz_struct_msg_len(_f(spec), len(spec)) == 0 or what.endswith("the record")
    h = ctypes.c_void_p()
    rc = lib.mk_struct_list_tree_new(ctypes.byref(call), record_len, _f(spec), len(spec), 10, ctypes.byref(h))
    assert rc == _lib.MK_EINVAL and not h.value


def test_malformed_details_differ(lib):
    errs = {what: _build(lib, spec, rl)[1].err for what, spec, rl in MALFORMED}
    assert len(set(errs.values())) >= len(errs) - 2  # the two "past the ..." pairs may share a text
    assert b"LDS" in errs["LDS peak"]


@pytest.mark.parametrize("spec,record_len", [(ONE_LEVEL, 72), (TWO_LEVEL, 64), (FLAT_VAR, 64), (DEPTH4, 8),
                                             (ST.PENDING_ATTESTATION_FIELDS, ST.pending_attestation_record_len(48)),
                                             (ST.ETH1_VOTE_FIELDS, 72)],
                         ids=["one_level", "two_level", "flat_var", "depth4", "attestation", "eth1_vote"])
def test_valid_nested_spec_gets_past_parsing(lib, spec, record_len):
    """Null buffers: the layout is accepted, so the call fails on the device
    (or on the pointers where there is one), never on the layout."""
    rc, call = _build(lib, spec, record_len)
    if _lib.device_count() == 0:
        assert rc == _lib.MK_ENODEV, call.err
    else:
        assert rc == _lib.MK_EINVAL and b"null pointer" in call.err
    need = lib.mk_ssz_struct_list_tree_build_workspace_bytes(1000, _f(spec), len(spec))
    assert need > 0
    rc, call = _build(lib, spec, record_len, n=1000, cap=1000, ws_bytes=need - 1)
    assert rc == _lib.MK_ENOMEM and b"workspace" in call.err
    assert lib.mk_ssz_struct_list_workspace_bytes(1000, _f(spec), len(spec)) >= \
        1000 * lib.mk_ssz_struct_msg_len(_f(spec), len(spec))
    assert lib.mk_ssz_struct_list_tree_update_workspace_bytes(7, _f(spec), len(spec)) > 0


def test_fast_paths_refuse_the_new_kinds(lib):
    for spec, rl in ((ONE_LEVEL, 72), (FLAT_VAR, 64)):
        assert lib.mk_ssz_struct_list_level1_ok(ctypes.c_void_p(4096), 1 << 20, rl, _f(spec), len(spec)) == 0
