"""Merkle proofs out of a tree set (mk_tree_set_branches): a
validator, a balance or a block root shown to be in the root of the whole
BeaconState, with an update still pending when the proofs are asked for.  The
records and verdicts are also held against the plain-Python rule
(tests/list_branch_ref.py)."""
import numpy as np
import pytest

from prysm_amd import _lib
from tests import list_branch_ref as R

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000000 + 5300


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def test_beacon_state_proofs_with_an_update_pending(gpu):
    from prysm_amd import registry as RG
    from prysm_amd import state as ST
    from prysm_amd.listtree import verify_branches

    st = ST.synthetic_state(65, SEED, n_attestations=5, n_batched=3, n_votes=2, lists_len=64, shards=64)
    donor = ST.synthetic_state(8, SEED + 1, n_attestations=1, n_batched=1, n_votes=1, lists_len=8, shards=8)
    ts = ST.beacon_tree_set(st)
    before = ts.root()
    # pending: nothing below is flushed until the proofs are asked for
    st.registry.records[31] = donor.registry.records[3]
    ts.update("registry", [31], donor.registry.records[3:4])
    st.balances[7] = 123456789
    ts.update("balances", [7], st.balances[7:8].astype("<u8"))
    want = st.tree_hash_ssz()
    assert want != before

    vidx = [0, 31, 64]
    values, br, msg = ts.branches("registry", vidx)
    assert len(msg) == ST.CONTAINER_LEN and ts.leaf_len("registry") == 32
    off = ts.container_off("registry")
    ok = verify_branches(values, vidx, 65, 32, br, want, container=msg, container_off=off)
    assert ok.all()
    assert ts.root() == want
    # a leaf is the struct root of the record as the set holds it
    for g, i in enumerate(vidx):
        rec = ts.items("registry", i, 1)
        assert np.array_equal(rec.reshape(-1), st.registry.records[i:i + 1].view(np.uint8).reshape(-1))
        assert values[g].tobytes() == RG.struct_roots(st.registry.records[i:i + 1])[0].tobytes()
    # the rule agrees, record by record
    roots0 = RG.struct_roots(st.registry.records).reshape(-1).tobytes()
    for g, i in enumerate(vidx):
        assert br[g].tobytes() == R.prove(roots0, 65, 32, i)
        assert R.verify(values[g].tobytes(), i, 65, 32, br[g].tobytes(), want, msg, off)
    # the old validator 31 is not in the new root, nor is any validator at another index
    bad = values.copy()
    bad[1] = RG.struct_roots(ST.synthetic_state(65, SEED, n_attestations=5, n_batched=3, n_votes=2, lists_len=64,
                                                shards=64).registry.records[31:32])[0]
    assert verify_branches(bad, vidx, 65, 32, br, want, container=msg, container_off=off).tolist() == [True, False, True]
    assert not verify_branches(values, [1, 30, 63], 65, 32, br, want, container=msg, container_off=off).any()
    # against the root before the update: none
    assert not verify_branches(values, vidx, 65, 32, br, before, container=msg, container_off=off).any()

    bidx = [64, 7, 1]
    values, br, msg2 = ts.branches("balances", bidx)
    assert msg2 == msg and ts.leaf_len("balances") == 8
    assert values.reshape(-1).view("<u8").tolist() == [int(st.balances[i]) for i in bidx]
    off = ts.container_off("balances")
    assert verify_branches(values, bidx, 65, 8, br, want, container=msg, container_off=off).all()
    bal0 = st.balances.astype("<u8").tobytes()
    for g, i in enumerate(bidx):
        assert br[g].tobytes() == R.prove(bal0, 65, 8, i)
    # with another tree's offset the proofs do not verify
    assert not verify_branches(values, bidx, 65, 8, br, want, container=msg,
                               container_off=ts.container_off("registry")).any()

    # a block root: a bytes tree, the leaf is the element's digest
    values, br, _ = ts.branches("latest_block_roots", [0, 63])
    assert verify_branches(values, [0, 63], 64, 32, br, want, container=msg,
                           container_off=ts.container_off("latest_block_roots")).all()
    with pytest.raises(_lib.MerkleError) as ei:
        ts.branches("balances", [65])
    assert ei.value.code == _lib.MK_EINVAL


def test_a_tree_outside_the_container(gpu):
    from oracle import oracle as O
    from prysm_amd.listtree import TreeSet, verify_branches

    s = TreeSet(container_len=40)
    a = s.add(_lib.MK_TREE_LIST, 8, container_off=4)
    b = s.add(_lib.MK_TREE_LIST, 48)  # no field of the message
    s.put(0, b"\x01\x02\x03\x04")
    s.put(36, b"\x05\x06\x07\x08")
    n = 11
    va = O.splitmix_bytes(8 * n, SEED + 2).copy()
    vb = O.splitmix_bytes(48 * n, SEED + 3).copy()
    s.assign(a, va)
    s.assign(b, vb)
    s.append(b, vb[:48])  # pending
    idx = [11, 0, 5]
    values, br, msg = s.branches(b, idx)
    assert s.container_off(b) is None and s.count(b) == 12
    data = vb.tobytes() + vb[:48].tobytes()
    assert br.tobytes() == b"".join(R.prove(data, 12, 48, i) for i in idx)
    root_b = s.tree_root(b)
    assert root_b == R.list_root(data, 12, 48)
    assert verify_branches(values, idx, 12, 48, br, root_b).all()
    # the message carries the other tree's root, and that tree proves into the set's root
    assert msg[:4] == b"\x01\x02\x03\x04" and msg[36:] == b"\x05\x06\x07\x08" and msg[4:36] == s.tree_root(a)
    values, br, msg = s.branches(a, [10])
    assert verify_branches(values, [10], n, 8, br, s.root(), container=msg, container_off=4).all()
    assert O.keccak256(msg) == s.root()

    bare = TreeSet()  # no container at all
    t = bare.add(_lib.MK_TREE_BYTES, 20)
    bare.assign(t, O.splitmix_bytes(20 * 8, SEED + 4)[:20 * 7].copy())
    values, br, msg = bare.branches(t, [6, 0])
    assert msg == b"" and bare.leaf_len(t) == 32
    assert verify_branches(values, [6, 0], 7, 32, br, bare.tree_root(t)).all()
