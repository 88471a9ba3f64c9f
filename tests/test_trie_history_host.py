"""The as-of rule of the deposit trie (tests/trie_history_ref.py, the algorithm
k_trie_branches_at implements: DESIGN.md §5i) against the reference's own
incremental trie: the edge chain and the gather over the FINAL level array of
n deposits must give, for every past count c and index i, exactly what
oracle.DictTrie (deposit_trie.go:13-63 restated) answered right after its
c-th UpdateDepositTrie.  CPU only; it pins the algorithm before any GPU run.
The last test checks the new entry points' host-side argument rules."""
import ctypes

import pytest

from tests import trie_history_ref as H

SEED = 0x5EED000000000000 + 0x71E


def _deposits(n):
    from oracle import oracle as O

    return [bytes(O.splitmix_bytes(48 + 8 * (i % 5), SEED, 64 * i)) for i in range(n)]


def _check(n, depth):
    from oracle import oracle as O

    deps = _deposits(n)
    snaps = H.Snapshots(deps, range(n + 1), depth)
    _, levels = O.deposit_trie_levels(deps, depth)
    hi = min((1 << depth) - 1, n + 2)
    for c in range(n + 1):
        edge = H.edge_chain(levels, n, c, depth, O.keccak256)
        assert H.root_at(edge, c, depth) == snaps.root(c), (n, c)
        for i in range(hi + 1):
            assert b"".join(H.branch_at(levels, edge, c, i, depth)) == snaps.branch(c, i), (n, c, i)


@pytest.mark.parametrize("n", range(1, 34))
def test_as_of_rule_depth6(n):
    _check(n, 6)


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65])
def test_as_of_rule_depth32(n):
    _check(n, 32)


def test_snapshot_at_count_is_the_live_trie():
    """The snapshot helper itself: at c == n it is the DictTrie run to n."""
    from oracle import oracle as O

    deps = _deposits(9)
    t = O.DictTrie(6)
    for d in deps:
        t.update(d)
    snaps = H.Snapshots(deps, [0, 9], 6)
    assert snaps.root(9) == t.root() and snaps.root(0) == bytes(32)
    assert snaps.branch(9, 4) == b"".join(t.branch(4))


def test_new_entry_points_are_declared_and_check_arguments():
    """Header, ctypes table and library agree on the five new calls, and the
    checks that need no device answer without one."""
    from prysm_amd import _lib

    names = set(_lib.header_symbols())
    for sym in ("mk_dev_deposit_trie_branches", "mk_deposit_trie_branches", "mk_deposit_trie_root_at",
                "mk_dev_verify_deposits", "mk_verify_deposits"):
        assert sym in names and sym in _lib._SIGS, sym
        assert hasattr(_lib.load(), sym), sym
    lib = _lib.load()
    call = _lib.Call(-1, 0, b"")
    ok = ctypes.create_string_buffer(4)
    rc = lib.mk_verify_deposits(ctypes.byref(call), None, None, None, None, 0, 32, 32, None, 7, ok)
    assert rc == _lib.MK_EINVAL and b"root_stride" in call.err
    out = ctypes.create_string_buffer(32)
    rc = lib.mk_deposit_trie_root_at(ctypes.byref(call), None, 0, out)
    assert rc == _lib.MK_EINVAL
    rc = lib.mk_deposit_trie_branches(ctypes.byref(call), None, 0, None, 0, None, out)
    assert rc == _lib.MK_EINVAL
