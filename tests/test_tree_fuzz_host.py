"""The resident-tree fuzz's own model, plan and comparison, without a device
(tests/tree_fuzz_plan.py; oracle_tree, split_levels and compare_tree of
tests/test_gpu_list_tree.py): the restated tree reproduces the oracle's
merkleHash at every item length, the plan of the committed seed reaches every
item length, step kind and kernel branch it is there for, every index list is
strictly ascending, and the level comparison rejects a flipped byte and a
stale ancestor."""
import numpy as np
import pytest

from tests import tree_fuzz_plan as P
from tests.test_gpu_list_tree import _per, compare_tree, oracle_tree, split_levels
from tests.tree_fuzz_plan import BYTES, LIST, STRUCT


def _rand(nbytes, salt):
    from oracle import oracle as O

    return O.splitmix_bytes((nbytes + 7) // 8 * 8, P.SEED + 77_000 + salt)[:nbytes].copy()


@pytest.mark.parametrize("L", P.ITEM_LENS)
def test_oracle_tree_reproduces_merkle_hash(L):
    from oracle import oracle as O

    p = _per(L)
    buf = _rand(1025 * p * L, L)
    for n in sorted({0, 1, p - 1, p, p + 1, 2 * p, 2 * p + 1, 5 * p + 1, 1025 * p - 1}):
        levels, root = oracle_tree(buf, n, L)  # asserts its top against the oracle's root itself
        assert root == O.merkle_hash_flat(buf[:n * L], n, L), (L, n)
        nch = -(-n // p)
        assert len(levels) == (nch - 1).bit_length() if nch > 1 else not levels, (L, n)


def test_item_len_list_is_the_shared_one():
    import random

    from tests.test_gpu_fuzz import _item_len

    rng = random.Random(1)
    assert {_item_len(rng) for _ in range(2000)} == set(P.ITEM_LENS)


# ---- the plan of the committed seed ---------------------------------------------------------------
@pytest.fixture(scope="module")
def plans():
    calls = P.plan_calls()
    return {"list": P.plan_list(), "bytes": P.plan_bytes(), "struct": P.plan_struct(),
            "calls": P.flatten_calls(calls), "call_lives": calls}


needs_default_seed = pytest.mark.skipif(P.FUZZ_SEED != 0, reason="coverage is asserted for the committed seed")


@needs_default_seed
def test_plan_coverage(plans):
    cov = P.Coverage(plans["list"])
    cov.check_list()  # every item length, every step kind, the three scatter cases, the misaligned 256-B pair
    P.Coverage(plans["bytes"]).check_bytes()  # every element length and step kind, both fast32 branches
    P.Coverage(plans["struct"]).check_struct()  # every step kind, the validator layout among random ones
    cov = P.Coverage(plans["calls"])
    cov.check_common()
    assert {lf.kind for lf in plans["calls"]} == {LIST, STRUCT, BYTES}
    assert {len(cl.lives) for cl in plans["call_lives"]} >= {1, 16}
    offs = [o for cl in plans["call_lives"] for c in cl.calls for o in c.offs]
    assert any(o is None for o in offs) and any(o is not None for o in offs)


@pytest.mark.parametrize("which", ["list", "bytes", "struct", "calls"])
def test_steps_are_well_formed(plans, which):
    """Strictly ascending index lists (the entries >= n_old included: they lie
    behind the valid ones), each kind what its name says, every size inside the limits."""
    for lf in plans[which]:
        per, n = lf.per, lf.n0
        assert lf.n0 <= lf.cap and P.chunks_of(lf.cap, per) <= P.MAX_CHUNKS and lf.cap * lf.L <= P.MAX_BYTES, lf.name()
        assert 6 <= len(lf.steps) <= 12
        for st in lf.steps:
            what = (lf.name(), st.kind, st.idx[:8], st.n_old, st.n_new)
            assert st.n_old == n and n <= st.n_new <= lf.cap, what
            assert (np.diff(st.idx) > 0).all() and (st.idx >= 0).all(), what
            valid, ignored = st.idx[st.idx < n], st.idx[st.idx >= n]
            co, cn = P.chunks_of(n, per), P.chunks_of(st.n_new, per)
            k = st.kind
            if k.startswith("ignored"):
                assert ignored.size, what
            else:
                assert not ignored.size, what
            if k in ("ignored_alone", "ignored_empty", "ignored_empty_append"):
                assert not valid.size, what
            if k in ("ignored_behind", "ignored_append", "scattered", "update_append"):
                assert valid.size, what
            if k in ("ignored_empty", "ignored_empty_append", "append_from_0"):
                assert n == 0, what
            appends = k.startswith("append") or k in ("update_append", "ignored_append", "ignored_empty_append")
            assert (st.n_new > n) == appends, what
            if k == "nothing":
                assert st.work == 0, what
            if k == "every":
                assert np.array_equal(st.idx, np.arange(n)), what
            if k == "first_last":
                assert list(st.idx) == [0, n - 1], what
            if k == "dense_run":
                assert st.idx[0] % per == 0 and (st.idx[0] // per) % 2 == 1, what
                assert np.array_equal(st.idx, np.arange(st.idx[0], st.idx[0] + st.k)), what
            if k == "level1_pair":
                a, b = st.idx // per
                assert a % 2 == 0 and b == a + 1, what
            if k == "append_in_chunk":
                assert cn == co, what
            if k == "append_chunk":
                assert cn > co, what
            if k == "append_pair":
                assert (cn + 1) // 2 > (co + 1) // 2, what
            if k == "append_taller":
                assert co >= 2 and (cn - 1).bit_length() > (co - 1).bit_length(), what
            if k == "append_1_to_2":
                assert (co, cn) == (1, 2), what
            n = st.n_new


def test_call_containers_are_legal(plans):
    for cl in plans["call_lives"]:
        assert 1 <= len(cl.lives) <= 16 and len({len(lf.steps) for lf in cl.lives}) == 1
        assert len(cl.calls) == len(cl.lives[0].steps)
        for c in cl.calls:
            assert 32 <= c.length <= 4096 and c.base_off % 4 == 0 and c.root_off % 4 == 0
            offs = sorted(o for o in c.offs if o is not None)
            assert offs and len(c.offs) == len(cl.lives)
            assert all(o % 4 == 0 and o + 32 <= c.length for o in offs)
            assert all(b - a >= 32 for a, b in zip(offs, offs[1:]))


def test_model_applies_a_step():
    rows = np.zeros((10, 3), np.uint8)
    st = P.Step("ignored_append", [1, 4, 6, 7, 1 << 40], 6, 9, True, 0)
    vals = np.arange(8 * 3, dtype=np.uint8).reshape(8, 3) + 1
    P.apply_step(rows, st, vals)
    want = np.zeros((10, 3), np.uint8)
    want[1], want[4] = vals[0], vals[1]  # 6, 7 and 2^40 are >= n_old: ignored, also where the append lands
    want[6:9] = vals[5:]
    assert np.array_equal(rows, want)


# ---- the comparison must notice ---------------------------------------------------------------------
def _rooms(cap, L):
    """Nodes each level has room for in the layout of a tree with room for cap items."""
    c, out = -(-cap // _per(L)), []
    while c > 1:
        c = (c + 1) // 2
        out.append(c)
    return out


def _pack(levels, n, cap, L):
    """A level array in the device layout (the inverse of split_levels), unused nodes 0xEE."""
    room = _rooms(cap, L)
    flat = np.full(32 * sum(room), 0xEE, np.uint8)
    off = 0
    for lv, r in zip(levels, room):
        flat[32 * off:32 * (off + len(lv))] = lv.reshape(-1)
        off += r
    return flat


@pytest.mark.parametrize("L,n,cap", [(32, 4 * 37 - 1, 4 * 37 - 1), (8, 16 * 70 - 5, 16 * 100), (200, 19, 31)])
def test_comparison_rejects_a_wrong_tree(L, n, cap):
    p = _per(L)
    buf = _rand(cap * L, 10 * L)
    levels, root = oracle_tree(buf, n, L)
    assert len(levels) >= 4
    root = np.frombuffer(root, np.uint8)
    flat = _pack(levels, n, cap, L)
    compare_tree(buf, split_levels(flat, n, cap, L), root, buf, n, L, "the oracle's own tree")
    # one byte of one level-3 node
    bad = flat.copy()
    node = len(levels[2]) - 1
    bad[32 * (sum(_rooms(cap, L)[:2]) + node) + 17] ^= 0x01
    with pytest.raises(AssertionError, match=rf"level 3 nodes \[{node}\]"):
        compare_tree(buf, split_levels(bad, n, cap, L), root, buf, n, L, "flipped byte")
    # a stale ancestor: an item changes, its level-1 and level-2 nodes and everything from level 4 up to the
    # root are recomputed, its level-3 node is not
    new = buf.copy()
    item = 9 * p  # chunk 9: level-1 node 4, level-2 node 2, level-3 node 1
    new[item * L] ^= 0x80
    new_levels, new_root = oracle_tree(new, n, L)
    stale = [x.copy() for x in new_levels]
    stale[2][1] = levels[2][1]
    assert not np.array_equal(new_levels[2][1], levels[2][1])
    flat = _pack(stale, n, cap, L)
    with pytest.raises(AssertionError, match=r"level 3 nodes \[1\]"):
        compare_tree(new, split_levels(flat, n, cap, L), np.frombuffer(new_root, np.uint8), new, n, L, "stale")
    # and the item buffer and the root themselves
    with pytest.raises(AssertionError, match="items"):
        compare_tree(buf, split_levels(_pack(new_levels, n, cap, L), n, cap, L), np.frombuffer(new_root, np.uint8),
                     new, n, L, "old items")
    with pytest.raises(AssertionError, match="root"):
        compare_tree(new, split_levels(_pack(new_levels, n, cap, L), n, cap, L), root, new, n, L, "old root")

