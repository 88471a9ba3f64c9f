"""Host side of the list-tree proofs: the plain-Python rule
(tests/list_branch_ref.py) against ``oracle.merkle_hash_flat``, the record
stride of the library against the rule's, and every argument error of the new
entry points that is decided before a device is looked up (the pointers are
made-up addresses that are only ever compared)."""
import ctypes
import os

import numpy as np
import pytest

from oracle import oracle as O
from prysm_amd import _lib
from tests import list_branch_ref as R

SIZES = (1, 8, 32, 48, 64, 100, 128)
COUNTS = tuple(range(0, 41)) + (63, 64, 65, 127, 129, 257)
P = 0x7F0000001000  # a 4096-B aligned address that is never dereferenced


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def data_of(n, s):
    return bytes(O.splitmix_bytes(max(n * s, 8), 0xB4A9C400 + 131 * n + s)[:n * s])


def indices_of(n):
    if n <= 40:
        return range(n)
    return sorted({0, 1, n // 2, n - 2, n - 1, (n * 7) // 13})


@pytest.mark.parametrize("s", SIZES)
def test_rule_against_merkle_hash(s):
    """Every proof verifies against the oracle's merkleHash, a flipped value bit does not."""
    for n in COUNTS:
        data = data_of(n, s)
        root = O.merkle_hash_flat(np.frombuffer(data, dtype=np.uint8), n, s)
        assert R.list_root(data, n, s) == root, (n, s)
        lv = R.levels(data, n, s)
        for i in indices_of(n):
            rec = R.prove(data, n, s, i, lv)
            assert len(rec) == R.stride(n, s)
            val = data[i * s:(i + 1) * s]
            assert R.verify(val, i, n, s, rec, root), (n, s, i)
            bad = bytearray(val)
            bad[(i * 5) % s] ^= 1 << (i % 8)
            assert not R.verify(bytes(bad), i, n, s, rec, root), (n, s, i)


@pytest.mark.parametrize("s", SIZES)
def test_rule_rejects_corruptions(s):
    p = 128 // s
    for n in (2 * p + 1, 5 * p, 37 * p + 3):
        data = data_of(n, s)
        root = R.list_root(data, n, s)
        lv = R.levels(data, n, s)
        D = R.shape(n, s)[4]
        for i in (0, n // 2, n - 1):
            rec = R.prove(data, n, s, i, lv)
            val = data[i * s:(i + 1) * s]
            # a sibling the fold uses: flipped
            j = (i // p) // 2
            for d in range(1, D):
                q = j >> (d - 1)
                used = (q & 1) or q + 1 < -(-R.shape(n, s)[2] // (1 << d))
                bad = bytearray(rec)
                bad[256 + 32 * (d - 1) + 7] ^= 0x10
                assert R.verify(val, i, n, s, bytes(bad), root) == (not used), (n, s, i, d)
            # a wrong index (another window or another place in it) and a wrong n
            other = (i + p) % n if (i + p) % n != i else (i + 1) % n
            if data[other * s:(other + 1) * s] != val:
                assert not R.verify(val, other, n, s, rec, root), (n, s, i)
            for m in (n + 1, n - 1):
                if i < m:
                    assert not R.verify(val, i, m, s, rec.ljust(R.stride(m, s), b"\0"), root), (n, s, i, m)
            assert not R.verify(val, n, n, s, rec, root)  # i >= n


@pytest.mark.parametrize("s", SIZES)
def test_rule_ignores_what_it_does_not_read(s):
    """Bytes past the window's end and slots of siblings that do not exist do not matter."""
    p = 128 // s
    touched = 0
    for n in (1, p + 1, 2 * p + 1, 4 * p + 1, 37 * p + 3):
        data = data_of(n, s)
        root = R.list_root(data, n, s)
        _, cb, nchunks, total, D = R.shape(n, s)
        i = n - 1
        rec = bytearray(R.prove(data, n, s, i))
        j = (i // p) // 2 if nchunks >= 2 else 0
        wl = min(total, (2 * j + 2) * cb) - 2 * j * cb if nchunks >= 2 else total
        for b in range(wl, 256):
            rec[b] = 0xA5
            touched += 1
        for d in range(1, D):
            q = j >> (d - 1)
            if not (q & 1) and q + 1 >= -(-nchunks // (1 << d)):
                rec[256 + 32 * (d - 1):256 + 32 * d] = b"\x5A" * 32
                touched += 1
        assert R.verify(data[i * s:(i + 1) * s], i, n, s, bytes(rec), root), (n, s)
    assert touched >= 4


def test_record_stride(lib):
    for s in SIZES + (2, 3, 31, 33, 65, 127):
        for n in COUNTS + (1 << 20, (1 << 24) + 1, 1 << 40):
            assert lib.mk_ssz_list_branch_bytes(n, s) == R.stride(n, s), (n, s)
    assert lib.mk_ssz_list_branch_bytes(10, 0) == 0
    assert lib.mk_ssz_list_branch_bytes(10, 129) == 0
    assert lib.mk_ssz_list_branch_bytes(1 << 20, 32) == 256 + 32 * 17


# ---- argument errors: MK_EINVAL with no device looked up ---------------------------------------
def branches(lib, n=100, cap=128, item_len=32, k=4, level0=P, levels=P + (1 << 20), idx=P + (2 << 20),
             out=P + (3 << 20)):
    call = _lib.Call(-1, 0, b"")
    vp = ctypes.c_void_p
    rc = lib.mk_dev_ssz_list_tree_branches(ctypes.byref(call), vp(level0), n, cap, item_len, vp(levels), vp(idx), k,
                                           vp(out), None)
    assert call.code == rc
    return rc, call.err


def verify(lib, host=False, k=4, n=100, item_len=32, values=P, idx=P + (1 << 20), br=P + (2 << 20),
           roots=P + (3 << 20), root_stride=0, container=None, clen=0, coff=0, ok=P + (4 << 20)):
    call = _lib.Call(-1, 0, b"")
    vp = ctypes.c_void_p
    args = [ctypes.byref(call), vp(values), vp(idx), k, n, item_len, vp(br), vp(roots), root_stride, vp(container),
            clen, coff, vp(ok)]
    rc = lib.mk_verify_list_branches(*args) if host else lib.mk_dev_verify_list_branches(*args, None)
    assert call.code == rc
    return rc, call.err


def test_branches_argument_errors(lib):
    E = _lib.MK_EINVAL
    assert branches(lib, item_len=0)[0] == E
    rc, err = branches(lib, item_len=129)
    assert rc == E and b"129" in err
    rc, err = branches(lib, n=129, cap=128)
    assert rc == E and b"capacity" in err
    assert branches(lib, k=1 << 31)[0] == E
    assert branches(lib, cap=1 << 62, item_len=64)[0] == E  # capacity * item_len overflows
    assert branches(lib, idx=None)[0] == E
    assert branches(lib, out=None)[0] == E
    assert branches(lib, level0=None)[0] == E
    assert branches(lib, levels=None)[0] == E            # 100 x 32 B: 25 chunks, levels exist
    assert branches(lib, levels=P + 8)[0] == E
    assert branches(lib, out=P + 8)[0] == E
    assert branches(lib, idx=P + 4)[0] == E


@pytest.mark.parametrize("host", [False, True])
def test_verify_argument_errors(lib, host):
    E = _lib.MK_EINVAL
    assert verify(lib, host, item_len=0)[0] == E
    assert verify(lib, host, item_len=129)[0] == E
    assert verify(lib, host, k=1 << 31)[0] == E
    rc, err = verify(lib, host, root_stride=16)
    assert rc == E and b"root_stride" in err
    assert verify(lib, host, container=P + (5 << 20), clen=64, coff=33)[0] == E
    assert verify(lib, host, container=P + (5 << 20), clen=31, coff=0)[0] == E
    assert verify(lib, host, container=P + (5 << 20), clen=_lib.MK_CONTAINER_MAX + 1, coff=0)[0] == E
    for missing in ("values", "idx", "br", "roots", "ok"):
        assert verify(lib, host, **{missing: None})[0] == E, missing
    if not host:
        assert verify(lib, host, br=P + 8)[0] == E
        assert verify(lib, host, idx=P + 4)[0] == E
        assert verify(lib, host, roots=P + 2)[0] == E


def test_handle_argument_errors(lib):
    E = _lib.MK_EINVAL
    vp = ctypes.c_void_p
    for name in ("mk_list_tree_branches", "mk_struct_list_tree_branches", "mk_bytes_list_tree_branches"):
        call = _lib.Call(-1, 0, b"")
        assert getattr(lib, name)(ctypes.byref(call), None, vp(P), 1, vp(P), vp(P)) == E
        assert call.code == E and b"null" in call.err
    call = _lib.Call(-1, 0, b"")
    assert lib.mk_tree_set_branches(ctypes.byref(call), None, 0, vp(P), 1, vp(P), vp(P), None) == E
    # a set with no tree: the tree number is refused before any device is needed
    h = ctypes.c_void_p()
    _lib.invoke("mk_tree_set_new", 64, ctypes.byref(h))
    try:
        call = _lib.Call(-1, 0, b"")
        assert lib.mk_tree_set_branches(ctypes.byref(call), h, 0, vp(P), 1, vp(P), vp(P), None) == E
        assert b"tree 0" in call.err
        call = _lib.Call(-1, 0, b"")
        assert lib.mk_tree_set_branches(ctypes.byref(call), h, 0, None, 1, vp(P), vp(P), None) == E
    finally:
        lib.mk_tree_set_free(h)
