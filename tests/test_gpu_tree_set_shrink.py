"""Shrinking a tree of a tree set (mk_tree_set_truncate / _erase, DESIGN.md
§5k): the epoch's two shrinking lists of a BeaconState behind
prysm_amd.state.beacon_tree_set() -- CleanupAttestations' stable filter
(epoch_processing.go:310-321) as an erase, the reset of the Eth1 data votes
(epoch_processing.go:81) as a truncate to 0 -- held against
BeaconState.tree_hash_ssz() of the same state after every step (and the
reflective oracle at the end); a shrink while other trees of the set have
changes pending; a shrink of every tree of a 16-tree set against the CPU
oracle (O.merkle_hash_flat over the items, O.elem_digests or O.struct_roots;
O.keccak256 of the message with the roots in place)."""
import numpy as np
import pytest

from prysm_amd import _lib
from tests.test_gpu_resident_state import _append_attestation, _one_attestation, _oracle

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000000 + 5200
EPOCH_LENGTH = 64


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def _keep_attestations(st, keep):
    a = st.attestations
    for f in ("slot", "shard", "roots", "justified_epoch", "justified_root", "justified_slot", "slot_included"):
        setattr(a, f, getattr(a, f)[keep])
    a.aggregation_bitfield = [a.aggregation_bitfield[i] for i in keep]
    a.custody_bitfield = [a.custody_bitfield[i] for i in keep]


def test_epoch_cleanup_of_a_beacon_state(gpu):
    from prysm_amd import state as ST

    st = ST.synthetic_state(256, SEED, n_attestations=128, n_batched=16, n_votes=4, lists_len=8192, shards=1024)
    donor = ST.synthetic_state(64, SEED + 77, n_attestations=16, n_batched=0, n_votes=4, lists_len=64, shards=64)
    st.scalars["Slot"] = int(np.sort(st.attestations.slot)[64])  # about half of the attestations are older
    ts = ST.beacon_tree_set(st)
    assert ts.root() == st.tree_hash_ssz(), "assign"
    # CleanupAttestations: the reference's filter on the host list, the dropped positions erased on the device
    cur = st.scalars["Slot"] // EPOCH_LENGTH
    keep = [i for i in range(len(st.attestations)) if int(st.attestations.slot[i]) // EPOCH_LENGTH >= cur]
    drop = [i for i in range(len(st.attestations)) if i not in set(keep)]
    assert 16 < len(drop) < 112 and drop != list(range(len(drop)))  # a real filter, not a prefix
    _keep_attestations(st, keep)
    ts.erase("attestations", drop)
    assert ts.count("attestations") == len(keep)
    assert ts.root() == st.tree_hash_ssz(), "after the erase"
    assert np.array_equal(ts.items("attestations"), ST.pack_attestations(st.attestations, 48)[0])
    # the end of a voting period
    st.eth1_votes, st.eth1_vote_counts = st.eth1_votes[:0], st.eth1_vote_counts[:0]
    ts.truncate("eth1_votes", 0)
    assert ts.count("eth1_votes") == 0
    assert ts.root() == st.tree_hash_ssz(), "after the truncate"
    # a slot's ordinary updates on the shrunk trees
    rng = np.random.default_rng(3)
    for slot in range(2):
        at = (st.scalars["Slot"] + slot) % 8192
        new32 = donor.randao_mixes[2 * slot:2 * slot + 2]
        st.latest_block_roots[at], st.randao_mixes[at] = new32[0], new32[1]
        ts.update("latest_block_roots", [at], new32[0:1])
        ts.update("randao_mixes", [at], new32[1:2])
        bi = rng.choice(256, 3, replace=False)
        bv = rng.integers(0, 1 << 40, 3).astype(np.uint64)
        st.balances[bi] = bv
        ts.update("balances", bi, bv.astype("<u8"))
        one = _one_attestation(donor, slot)
        _append_attestation(st, one)
        ts.append("attestations", one)
        st.eth1_votes = np.concatenate([st.eth1_votes, donor.eth1_votes[slot:slot + 1]])
        st.eth1_vote_counts = np.concatenate([st.eth1_vote_counts, donor.eth1_vote_counts[slot:slot + 1]])
        ts.append("eth1_votes", ST.pack_eth1_votes(donor.eth1_votes[slot:slot + 1], donor.eth1_vote_counts[slot:slot + 1]))
        st.scalars["Slot"] += 1
        ts.set_scalar("Slot", st.scalars["Slot"])
        assert ts.root() == st.tree_hash_ssz(), f"slot {slot}"
    assert ts.root() == _oracle(st), "the reflective oracle at the end"


def test_shrink_with_changes_pending_elsewhere(gpu):
    """Updates and appends recorded on other trees (and on the shrinking tree itself) before a shrink are
    flushed, not lost; a refused shrink changes nothing."""
    from prysm_amd import state as ST

    st = ST.synthetic_state(37, SEED + 1, n_attestations=9, n_batched=3, n_votes=3, lists_len=5, shards=5)
    donor = ST.synthetic_state(8, SEED + 2, n_attestations=4, n_batched=4, n_votes=2, lists_len=8, shards=8)
    ts = ST.beacon_tree_set(st)
    assert ts.root() == st.tree_hash_ssz()
    # pending: a balance, an appended batched root, an appended attestation (on the tree that shrinks)
    st.balances[5] = 12345
    ts.update("balances", [5], np.array([12345], dtype="<u8"))
    st.batched_block_roots = np.concatenate([st.batched_block_roots, donor.batched_block_roots[:1]])
    ts.append("batched_block_roots", donor.batched_block_roots[:1])
    one = _one_attestation(donor, 0)
    _append_attestation(st, one)
    ts.append("attestations", one)
    n = ts.count("attestations")
    assert n == 10
    for call in (lambda: ts.erase("attestations", [n]), lambda: ts.truncate("attestations", n + 1),
                 lambda: ts.truncate(99, 0)):
        with pytest.raises(_lib.MerkleError) as e:
            call()
        assert e.value.code == _lib.MK_EINVAL
    assert ts.count("attestations") == n
    ts.erase("attestations", [9, 0, 4, 9])  # the pending append goes too
    _keep_attestations(st, [1, 2, 3, 5, 6, 7, 8])
    assert ts.count("attestations") == 7
    assert np.array_equal(ts.items("attestations"), ST.pack_attestations(st.attestations, 48)[0])  # seen at once
    assert ts.tree_root("balances") != b"" and ts.root() == st.tree_hash_ssz(), "nothing pending was lost"
    assert int(ts.items("balances", 5, 1).reshape(-1).view("<u8")[0]) == 12345
    ts.truncate("attestations", 7)  # no-ops
    ts.erase("attestations", [])
    assert ts.root() == st.tree_hash_ssz()


def test_shrink_every_tree_of_a_full_set(gpu):
    from oracle import oracle as O
    from prysm_amd import registry as R
    from prysm_amd import state as ST
    from prysm_amd.listtree import TreeSet

    LIST, STRUCT, BYTES = _lib.MK_TREE_LIST, _lib.MK_TREE_STRUCT, _lib.MK_TREE_BYTES
    spec = {160: R.VALIDATOR_FIELDS, 40: ST.CROSSLINK_FIELDS}
    shapes = [(LIST, 8), (STRUCT, 160), (BYTES, 32), (LIST, 1), (BYTES, 20), (STRUCT, 40), (LIST, 48), (LIST, 32)] * 2
    assert len(shapes) == _lib.MK_TREES_MAX == 16
    counts = [1, 2, 4, 5, 8, 9, 16, 17, 33, 257, 1025, 300, 70, 12, 6, 3]
    s = TreeSet(32 * 16 + 8)
    s.put(512, b"\x07" * 8)
    rows = []
    for i, ((kind, L), n) in enumerate(zip(shapes, counts)):
        t = s.add(kind, L, fields=spec.get(L) if kind == STRUCT else None, container_off=32 * i)
        if kind == STRUCT and L == 160:
            a = R.synthetic_registry(n, SEED + 10 + i).records.view(np.uint8).reshape(n, L).copy()
        else:
            a = O.splitmix_bytes((n * L + 7) // 8 * 8, SEED + 10 + i)[:n * L].copy().reshape(n, L)
        s.assign(t, a)
        rows.append(a)

    def tree_root(i):
        (kind, L), a = shapes[i], rows[i]
        n = len(a)
        flat = np.ascontiguousarray(a).reshape(-1)
        if kind == LIST:
            return O.merkle_hash_flat(flat, n, L)
        lv0 = O.elem_digests(flat, n, L) if kind == BYTES else O.struct_roots(a, n, L, spec[L])
        return O.merkle_hash_flat(np.ascontiguousarray(lv0).reshape(-1), n, 32)

    def want():
        return O.keccak256(b"".join(tree_root(i) for i in range(16)) + b"\x07" * 8)

    assert s.root() == want()
    rng = np.random.default_rng(8)
    for i in range(16):  # every tree shrinks before the next root: erase and truncate in turn
        n = len(rows[i])
        if i % 2:
            s.truncate(i, n // 2)
            rows[i] = rows[i][:n // 2]
        else:
            rm = rng.choice(n, max(1, n // 3), replace=False)
            s.erase(i, rm)
            rows[i] = np.delete(rows[i], rm, axis=0)
        assert s.count(i) == len(rows[i])
    assert s.root() == want()
    for i in range(16):
        assert s.tree_root(i) == tree_root(i), i
        assert np.array_equal(s.items(i), rows[i]), i
