"""A second resident state (mk_tree_set_clone / _copy / _reserve, DESIGN.md
§5m): prysm_amd.state.BeaconTreeSet over state.py's small synthetic state,
cloned with changes still pending, a slot's changes applied to the clone alone,
and copy_from as the way back after a block that is thrown away.  Every root is
held against BeaconState.tree_hash_ssz() of a host model that saw the same
changes (and the reflective oracle at the end)."""
import copy

import numpy as np
import pytest

from prysm_amd import _lib
from tests.test_gpu_resident_state import _append_attestation, _one_attestation, _oracle
from tests.test_gpu_tree_set_shrink import _keep_attestations

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000000 + 5300


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def _states():
    from prysm_amd import state as ST

    st = ST.synthetic_state(300, SEED, n_attestations=40, n_batched=5, n_votes=4, lists_len=64, shards=64)
    donor = ST.synthetic_state(64, SEED + 77, n_attestations=16, n_batched=4, n_votes=4, lists_len=64, shards=64)
    return st, donor


def _slot(ts, st, donor, j):
    """A slot's changes on the set and on its host model: a registry update, balances, an attestation
    appended, two attestations erased, a put."""
    from prysm_amd import state as ST

    ri = np.array([3 + j, 250 - j])
    st.registry.records[ri] = donor.registry.records[[j, j + 1]]
    ts.update("registry", ri, donor.registry.records[[j, j + 1]])
    bi = np.array([0, 17 + j, 299])
    bv = np.array([5 + j, 1 << 33, 77], dtype=np.uint64)
    st.balances[bi] = bv
    ts.update("balances", bi, bv.astype("<u8"))
    one = _one_attestation(donor, j)
    _append_attestation(st, one)
    ts.append("attestations", one)
    n = len(st.attestations)
    ts.erase("attestations", [1, n - 2])
    _keep_attestations(st, [i for i in range(n) if i not in (1, n - 2)])
    st.scalars["Slot"] += 1
    ts.set_scalar("Slot", st.scalars["Slot"])
    assert ts.count("attestations") == len(st.attestations)
    assert np.array_equal(ts.items("attestations"), ST.pack_attestations(st.attestations, 48)[0])


def test_clone_a_slot_on_the_clone_and_the_way_back(gpu):
    from prysm_amd import state as ST

    st, donor = _states()
    ts = ST.beacon_tree_set(st)
    assert ts.root() == st.tree_hash_ssz(), "assign"
    # pending and not flushed when the clone is taken: a balance, a block root, an appended vote
    st.balances[9] = 4242
    ts.update("balances", [9], np.array([4242], dtype="<u8"))
    st.latest_block_roots[5] = donor.randao_mixes[0]
    ts.update("latest_block_roots", [5], donor.randao_mixes[0:1])
    st.eth1_votes = np.concatenate([st.eth1_votes, donor.eth1_votes[:1]])
    st.eth1_vote_counts = np.concatenate([st.eth1_vote_counts, donor.eth1_vote_counts[:1]])
    ts.append("eth1_votes", ST.pack_eth1_votes(donor.eth1_votes[:1], donor.eth1_vote_counts[:1]))
    want0 = st.tree_hash_ssz()
    cl = ts.clone()
    assert type(cl) is ST.BeaconTreeSet and cl.tree == ts.tree and cl.tree is not ts.tree
    assert cl.root() == want0, "the clone's root includes what was pending"
    assert ts.root() == want0
    for name in ts.tree:
        assert cl.count(name) == ts.count(name) and cl.capacity(name) == ts.capacity(name), name
        assert np.array_equal(cl.items(name), ts.items(name)), name
        assert cl.tree_root(name) == ts.tree_root(name), name
    # a block's transition on the clone only
    st2 = copy.deepcopy(st)
    for j in range(2):
        _slot(cl, st2, donor, j)
        assert cl.root() == st2.tree_hash_ssz(), f"the clone after slot {j}"
        assert ts.root() == want0, "the original never moves"
    assert cl.root() == _oracle(st2), "the reflective oracle"
    # proofs out of the clone verify against the clone's root
    from prysm_amd.listtree import verify_branches

    idx = [0, 3, 299]
    vals, br, msg = cl.branches("registry", idx)
    assert verify_branches(vals, idx, cl.count("registry"), 32, br, cl.root(), msg, cl.container_off("registry")).all()
    # the block is thrown away: the clone goes back to the original, with something pending on both sides
    cl.update("balances", [1], np.array([99], dtype="<u8"))  # dropped by the copy
    st.balances[2] = 31337
    ts.update("balances", [2], np.array([31337], dtype="<u8"))  # pending on the source: travels
    cl.copy_from(ts)
    want1 = st.tree_hash_ssz()
    assert cl.root() == want1 and ts.root() == want1, "copy_from restores the clone to the original"
    vals, br, msg = cl.branches("balances", [2])  # not dirty after the copy: the message it hands out is its own
    assert verify_branches(vals, [2], cl.count("balances"), 8, br, cl.root(), msg, cl.container_off("balances")).all()
    for name in ts.tree:
        assert cl.count(name) == ts.count(name), name
        assert np.array_equal(cl.items(name), ts.items(name)), name
    # ... and is a state of its own again
    st3 = copy.deepcopy(st)
    _slot(cl, st3, donor, 3)
    assert cl.root() == st3.tree_hash_ssz() and ts.root() == want1
    ts.copy_from(ts)
    assert ts.root() == want1


def test_copy_into_a_set_whose_trees_are_too_small_and_reserve(gpu):
    from prysm_amd import state as ST

    st, donor = _states()
    ts = ST.beacon_tree_set(st)
    empty = ST.beacon_tree_set()  # every tree of capacity 1
    assert empty.capacity("registry") < ts.count("registry")
    empty.copy_from(ts)
    assert empty.root() == st.tree_hash_ssz() == ts.root()
    assert empty.capacity("registry") == ts.capacity("registry")  # it took the source's
    st2 = copy.deepcopy(st)
    _slot(empty, st2, donor, 1)
    assert empty.root() == st2.tree_hash_ssz() and ts.root() == st.tree_hash_ssz()
    # reserve one tree, with a change pending: root, count and values stay, and appends up to it do not regrow
    cap = ts.capacity("balances")
    st.balances[4] = 8
    ts.update("balances", [4], np.array([8], dtype="<u8"))
    ts.reserve("balances", 2 * cap + 3)
    ts.reserve("balances", 5)  # a no-op
    assert ts.capacity("balances") == 2 * cap + 3
    assert ts.root() == st.tree_hash_ssz(), "reserved: the pending change is still applied, nothing else moved"
    more = np.arange(2 * cap + 3 - len(st.balances), dtype=np.uint64) * 3 + 1
    st.balances = np.concatenate([st.balances, more])
    ts.append("balances", more.astype("<u8"))
    assert ts.tree_root("balances") != b"" and ts.capacity("balances") == 2 * cap + 3
    assert np.array_equal(ts.items("balances").reshape(-1).view("<u8"), st.balances)
    from oracle import oracle as O

    flat = np.ascontiguousarray(st.balances.astype("<u8")).view(np.uint8)
    assert ts.tree_root("balances") == O.merkle_hash_flat(flat, len(st.balances), 8)


def test_a_shape_mismatch_changes_nothing(gpu):
    from prysm_amd import state as ST
    from prysm_amd.listtree import TreeSet

    st, _ = _states()
    ts = ST.beacon_tree_set(st)
    want = st.tree_hash_ssz()
    assert ts.root() == want
    a = TreeSet(72)
    a.add(_lib.MK_TREE_LIST, 8, container_off=0)
    a.add(_lib.MK_TREE_BYTES, 32, container_off=32)
    a.assign(0, np.arange(10, dtype="<u8"))
    a.put(64, b"\x01" * 8)
    ra = a.root()
    others = []
    b = TreeSet(80)  # another container length
    b.add(_lib.MK_TREE_LIST, 8, container_off=0)
    b.add(_lib.MK_TREE_BYTES, 32, container_off=32)
    others.append(b)
    b = TreeSet(72)  # another item length
    b.add(_lib.MK_TREE_LIST, 16, container_off=0)
    b.add(_lib.MK_TREE_BYTES, 32, container_off=32)
    others.append(b)
    b = TreeSet(72)  # another kind
    b.add(_lib.MK_TREE_BYTES, 8, container_off=0)
    b.add(_lib.MK_TREE_BYTES, 32, container_off=32)
    others.append(b)
    b = TreeSet(72)  # another container offset
    b.add(_lib.MK_TREE_LIST, 8, container_off=32)
    b.add(_lib.MK_TREE_BYTES, 32, container_off=0)
    others.append(b)
    b = TreeSet(72)  # one tree fewer
    b.add(_lib.MK_TREE_LIST, 8, container_off=0)
    others.append(b)
    others.append(ts)  # another set altogether (ten trees, another record layout)
    for b in others:
        for dst, src in ((a, b), (b, a)):
            with pytest.raises(_lib.MerkleError) as e:
                dst.copy_from(src)
            assert e.value.code == _lib.MK_EINVAL
    assert a.root() == ra and a.count(0) == 10 and ts.root() == want
    c = a.clone()  # a plain TreeSet clones too, and the clone takes a matching copy
    assert type(c) is TreeSet and c.root() == ra
    c.update(0, [3], np.array([77], dtype="<u8"))
    assert c.root() != ra and a.root() == ra
    c.copy_from(a)
    assert c.root() == ra
