"""TreeSet.audit() (mk_tree_set_audit): whatever is pending is
flushed, then every tree of the set, every root, the roots' places in the hash
message and the hash of the message are checked in one launch.  A set is sound
after every operation a set has -- assign, update, append, put, erase, truncate,
reserve, clone, copy_from -- for a small mixed set and for a whole BeaconState
(the states are test_gpu_resident_state.py's)."""
import numpy as np
import pytest

from prysm_amd import _lib
from tests import tree_audit_ref as A
from tests.test_gpu_resident_state import _oracle, _state
from tests.test_gpu_tree_audit import kind
from tests.test_gpu_tree_shrink import rows

pytestmark = pytest.mark.gpu

CLEAN = (0, A.NONE, A.NO_INDEX)


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def sound(s, what):
    got = s.audit()
    assert got == [CLEAN] * (len(s) + 1), f"{what}: {got}"


def test_mixed_set_through_every_operation(gpu):
    from prysm_amd.listtree import TreeSet

    names = ["list-8", "struct-validator", "bytes-32", "list-100", "struct-attestation"]
    ks = [kind(nm) for nm in names]
    offs = [0, 40, None, 72, 104]
    s = TreeSet(container_len=136)
    for k, off in zip(ks, offs):
        s.add(k.tree_kind, k.L, fields=k.fields, capacity=0, container_off=off)
    s.put(32, bytes(range(8)))
    sound(s, "five empty trees")
    for i, k in enumerate(ks):
        s.assign(i, k.pool[rows(300 + 50 * i, i)])
    sound(s, "assigned")
    root = s.root()
    sound(s, "after a root")
    assert s.root() == root  # the audit changed nothing
    for i, k in enumerate(ks):
        s.update(i, [0, 299], k.pool[[7, 8]])
        s.append(i, k.pool[rows(5, 9)])
    sound(s, "pending updates and appends, flushed by the audit")
    assert s.root() != root
    s.append(0, ks[0].pool[rows(2000, 3)])  # past the capacity: doubled and rebuilt at the flush
    s.put(32, bytes(range(8, 16)))
    sound(s, "a tree that outgrew its capacity")
    s.erase(1, [0, 17, 300])
    s.truncate(2, 100)
    sound(s, "erase and truncate")
    s.reserve(3, 4000)
    s.update(3, [3], ks[3].pool[[11]])
    sound(s, "reserve, then an update in the new layout")
    c = s.clone()
    sound(c, "the clone")
    assert c.root() == s.root()
    c.update(4, [1], ks[4].pool[[12]])
    c.truncate(0, 0)
    sound(c, "the clone after changes of its own")
    sound(s, "the source, untouched")
    c.copy_from(s)
    sound(c, "copied back")
    assert c.root() == s.root()


def test_set_without_a_container(gpu):
    from prysm_amd.listtree import TreeSet

    k = kind("bytes-48")
    s = TreeSet()
    s.add(k.tree_kind, k.L)
    s.assign(0, k.pool[rows(77)])
    assert s.audit() == [CLEAN, CLEAN]
    with pytest.raises(_lib.MerkleError) as e:
        TreeSet(container_len=8).audit()
    assert e.value.code == _lib.MK_EINVAL


def test_beacon_tree_set_and_its_clone(gpu):
    from prysm_amd import state as ST

    st = _state(300, 16, 4, 2, 64)
    ts = ST.beacon_tree_set(st)
    sound(ts, "a BeaconState of 300 validators")
    assert ts.root() == _oracle(st)
    bi = np.array([0, 150, 299])
    st.balances[bi] = np.array([5, 6, 7], dtype=np.uint64)
    ts.update("balances", bi, st.balances[bi].astype("<u8"))
    st.scalars["Slot"] += 1
    ts.set_scalar("Slot", st.scalars["Slot"])
    ts.truncate("eth1_votes", 0)
    st.eth1_votes, st.eth1_vote_counts = st.eth1_votes[:0], st.eth1_vote_counts[:0]
    c = ts.clone()
    sound(ts, "after a slot's changes")
    sound(c, "its clone")
    assert c.root() == ts.root() == _oracle(st)
