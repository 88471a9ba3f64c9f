"""diff() of the three handles, of a TreeSet and of a BeaconTreeSet against its
clone (mk_*_tree_diff, mk_tree_set_diff).  The answer per tree
is numpy's over items() of both sides: the indices below the shorter count
whose values differ (every row comes from a pool whose rows differ inside their
hashed fields, so values differ exactly where the level-0 entries do)."""
import numpy as np
import pytest

from prysm_amd import _lib
from tests.test_gpu_resident_state import _state
from tests.test_gpu_tree_audit import kind
from tests.test_gpu_tree_shrink import rows

pytestmark = pytest.mark.gpu

NAMES = ["list-8", "struct-validator", "bytes-32", "list-100", "struct-attestation"]


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def answer(x, y):
    m = min(len(x), len(y))
    return [int(i) for i in np.flatnonzero((x[:m] != y[:m]).any(axis=1))]


def read(t):
    return getattr(t, t._reader)()


def check_tree(a, b, what, **kw):
    idx, total, na, nb = a.diff(b, **kw)
    want = answer(read(a), read(b))
    assert (na, nb) == (len(a), len(b)), what
    assert total == len(want), f"{what}: total {total}, want {len(want)}"
    assert idx.dtype == np.uint64, what
    if kw.get("max_out") is None:
        assert [int(i) for i in idx] == want, what
    return idx, want


@pytest.mark.parametrize("name", NAMES)
def test_handles(gpu, name):
    k = kind(name)
    n = 3 * 1024 * k.per // 2 + 5  # a work item and a half
    a = k.make(n + 10)
    a.assign(k.pool[rows(n, 1)])
    b = a.clone()
    assert check_tree(a, b, "a clone")[1] == []
    idx, total, na, nb = a.diff(a)
    assert (list(idx), total, na, nb) == ([], 0, n, n)
    # a mixed sequence on one side
    b.update([0, 5, n - 1], k.pool[[3, 4, 5]])
    b.append(k.pool[rows(40, 2)])
    check_tree(a, b, "update and append")
    check_tree(b, a, "the other way round")
    b.truncate(n - 3 * k.per - 1)
    check_tree(a, b, "truncated below the other's count")
    b.erase([7, 8, 200])  # everything behind moves up: the dense end
    idx, want = check_tree(a, b, "erase")
    assert len(want) > 4096 or len(want) > len(b) // 2  # (a pool row can repeat three places on)
    # fewer slots than differences: total exact, some max_out of them, ascending
    few, total, _, _ = a.diff(b, max_out=10)
    assert total == len(want) and len(few) == 10 and list(few) == sorted(few) and set(int(i) for i in few) <= set(want)
    none, total, _, _ = a.diff(b, max_out=0)
    assert total == len(want) and len(none) == 0
    a.copy_from(b)
    assert check_tree(a, b, "copy_from, then diff")[1] == []
    # handles that do not agree are refused
    other = kind("list-100" if name != "list-100" else "list-8")
    o = other.make(4)
    with pytest.raises(_lib.MerkleError) as e:
        a.diff(o)
    assert e.value.code == _lib.MK_EINVAL
    if k.tree_kind == _lib.MK_TREE_LIST:
        from prysm_amd.listtree import ListTree

        with pytest.raises(_lib.MerkleError) as e:
            a.diff(ListTree(k.L + 1, capacity=4))
        assert e.value.code == _lib.MK_EINVAL


def mixed_set():
    from prysm_amd.listtree import TreeSet

    ks = [kind(nm) for nm in NAMES]
    offs = [0, 40, None, 72, 104]
    s = TreeSet(container_len=136)
    for k, off in zip(ks, offs):
        s.add(k.tree_kind, k.L, fields=k.fields, capacity=0, container_off=off)
    return s, ks


def check_set(a, b, what, container=(0, None)):
    """container: what the container entry must be; "any": not looked at here."""
    got = a.diff(b)
    assert set(got) == set(range(len(a))) | {"container"}, what
    for i in range(len(a)):
        idx, total, na, nb = got[i]
        want = answer(a.items(i), b.items(i))
        assert (na, nb) == (a.count(i), b.count(i)), f"{what}: tree {i}"
        assert total == len(want) and [int(x) for x in idx] == want, f"{what}: tree {i}: {total} / {len(want)}"
    assert container == "any" or got["container"] == container, f"{what}: {got['container']}"
    return got


def test_tree_set(gpu):
    s, ks = mixed_set()
    s.put(32, bytes(range(8)))
    for i, k in enumerate(ks):
        s.assign(i, k.pool[rows(300 + 50 * i, i)])
    c = s.clone()
    check_set(s, c, "a clone")
    roots = (s.root(), c.root())
    # pending (unflushed) changes on both sides
    for i, k in enumerate(ks):
        c.update(i, [0, 299], k.pool[[7, 8]])
        c.append(i, k.pool[rows(5, 9)])
    s.update(0, [17], ks[0].pool[[9]])
    s.update(3, [299], ks[3].pool[[8]])  # the same value as the other side's: no difference
    got = check_set(s, c, "pending updates and appends on both sides")
    assert [int(x) for x in got[0][0]] == [0, 17, 299] and [int(x) for x in got[3][0]] == [0]
    c.erase(1, [0, 17, 300])
    c.truncate(2, 100)
    c.append(0, ks[0].pool[rows(2000, 3)])  # past the capacity: the two layouts differ from here on
    c.put(33, b"\xff\xfe")
    c.put(39, b"\x01")
    check_set(s, c, "erase, truncate, a rebuilt tree and a put", container=(3, 33))
    check_set(c, s, "the other way round", container=(3, 33))
    got = s.diff(c, max_out=2)
    assert got[1][1] > 2 and len(got[1][0]) == 2 and got[1][0][0] < got[1][0][1]
    assert all(t[1] == 0 for i, t in s.diff(s).items() if i != "container") and s.diff(s)["container"] == (0, None)
    # sets that do not agree are refused and nothing changes
    from prysm_amd.listtree import TreeSet

    t = TreeSet(container_len=136)
    for k, off in zip(ks, [40, 0, None, 72, 104]):
        t.add(k.tree_kind, k.L, fields=k.fields, capacity=0, container_off=off)
    before = (s.root(), c.root())
    for other in (t, TreeSet(container_len=136), TreeSet(container_len=8)):
        with pytest.raises(_lib.MerkleError) as e:
            s.diff(other)
        assert e.value.code == _lib.MK_EINVAL
    assert (s.root(), c.root()) == before and before[0] != roots[0]
    c.copy_from(s)
    check_set(s, c, "copy_from, then diff")


def test_beacon_tree_set_against_its_clone(gpu):
    from prysm_amd import state as ST

    st = _state(300, 16, 4, 2, 64)
    ts = ST.beacon_tree_set(st)
    c = ts.clone()
    check_set(ts, c, "a BeaconState of 300 validators against its clone")
    # one slot's changes on the candidate
    bi = np.array([0, 150, 299])
    c.update("balances", bi, (st.balances[bi] + 1).astype("<u8"))
    rec = st.registry.records.copy()
    rec["exit_epoch"][[7, 255]] ^= 1
    c.update("registry", [7, 255], rec[[7, 255]])
    c.set_scalar("Slot", st.scalars["Slot"] + 1)
    c.truncate("eth1_votes", 0)
    slot = st.scalars["Slot"] % len(st.latest_block_roots)
    c.update("latest_block_roots", [slot], np.full((1, 32), 0x77, dtype=np.uint8))
    got = check_set(ts, c, "after a slot's changes", container="any")
    assert [int(x) for x in got[ts.tree["balances"]][0]] == [0, 150, 299]
    assert [int(x) for x in got[ts.tree["registry"]][0]] == [7, 255]
    assert [int(x) for x in got[ts.tree["latest_block_roots"]][0]] == [slot]
    assert got[ts.tree["eth1_votes"]][1:] == (0, ts.count("eth1_votes"), 0)
    total, first = got["container"]
    assert total >= 1 and first == ST.CONTAINER_OFF["Slot"]
    ts.copy_from(c)
    check_set(ts, c, "the candidate accepted")
