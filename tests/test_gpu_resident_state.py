"""prysm_amd.state.ResidentBeaconState: a whole BeaconState resident in HBM,
its root by one mk_dev_ssz_trees_update.  Every root is held against the
oracle's reflective TreeHash of the same state (oracle/ssz_ref.py) and, slot by
slot, against the existing one-shot BeaconState.tree_hash_ssz of a host
mirror."""
import numpy as np
import pytest

from prysm_amd import _lib

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000000 + 3300


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def _state(nv, natt, nb, nvotes, lists, salt=0):
    from prysm_amd import state as ST

    return ST.synthetic_state(nv, SEED + nv + salt, n_attestations=natt, n_batched=nb, n_votes=nvotes,
                              lists_len=lists, shards=min(1024, lists))


def _oracle(st):
    from oracle import ssz_ref as OS
    from prysm_amd import state as ST
    from tests.ssz_types import to_ref_type

    return OS.tree_hash(to_ref_type(ST.STATE_SSZ), st.as_value())


def _one_attestation(donor, i):
    """Attestation i of ``donor`` as an Attestations of one."""
    from prysm_amd import state as ST

    a = donor.attestations
    return ST.Attestations(a.slot[i:i + 1], a.shard[i:i + 1], a.roots[i:i + 1], a.justified_epoch[i:i + 1],
                           a.justified_root[i:i + 1], a.justified_slot[i:i + 1], a.aggregation_bitfield[i:i + 1],
                           a.custody_bitfield[i:i + 1], a.slot_included[i:i + 1])


def _append_attestation(st, one):
    a = st.attestations
    for f in ("slot", "shard", "roots", "justified_epoch", "justified_root", "justified_slot", "slot_included"):
        setattr(a, f, np.concatenate([getattr(a, f), getattr(one, f)]))
    a.aggregation_bitfield = list(a.aggregation_bitfield) + list(one.aggregation_bitfield)
    a.custody_bitfield = list(a.custody_bitfield) + list(one.custody_bitfield)


@pytest.mark.parametrize("nv,natt,nb,nvotes,lists", [(37, 3, 1, 1, 5), (0, 0, 0, 0, 8192), (1000, 128, 16, 4, 8192)])
def test_root_after_assign(gpu, nv, natt, nb, nvotes, lists):
    from prysm_amd import state as ST

    st = _state(nv, natt, nb, nvotes, lists)
    rs = ST.ResidentBeaconState(gpu)
    rs.assign(st)
    want = _oracle(st)
    assert rs.root() == want
    assert rs.root() == want  # nothing dirty: the same root again


@pytest.fixture(scope="module")
def slots(gpu):
    """The (1000, ...) state after assign, eight slots and one epoch step:
    the resident root, the mirror's one-shot root and (where the test asks for
    it) the oracle's after each step, and the trees_update calls of each root()."""
    from prysm_amd import device as D
    from prysm_amd import registry as R
    from prysm_amd import state as ST

    st = _state(1000, 128, 16, 4, 8192)
    donor = _state(64, 16, 0, 4, 64, salt=77)  # new values: records, attestations, roots
    rs = ST.ResidentBeaconState(gpu)
    rs.assign(st)
    calls, real = [], D.trees_update

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    D.trees_update = counting
    out = {"steps": []}
    try:
        def root():
            del calls[:]
            r = rs.root()
            return r, len(calls)

        out["assign"] = root() + (st.tree_hash_ssz(),)
        rng = np.random.default_rng(5)
        for slot in range(8):
            at = (st.scalars["Slot"] + slot) % 8192
            new32 = donor.randao_mixes[2 * slot:2 * slot + 2]
            st.latest_block_roots[at], st.randao_mixes[at] = new32[0], new32[1]
            rs.update("latest_block_roots", [at], new32[0:1])
            rs.update("randao_mixes", [at], new32[1:2])
            bi = rng.choice(1000, 3, replace=False)
            bv = rng.integers(0, 1 << 40, 3).astype(np.uint64)
            st.balances[bi] = bv
            rs.update("balances", bi, bv)
            vi = rng.choice(1000, 2, replace=False)
            vr = donor.registry.records[4 * slot:4 * slot + 2]
            st.registry.records[vi] = vr
            rs.update("registry", vi, vr)
            one = _one_attestation(donor, slot)
            _append_attestation(st, one)
            rs.append("attestations", one)
            ci = int(rng.integers(0, 1024))
            st.crosslink_epochs[ci] = 7000 + slot
            st.crosslink_roots[ci] = donor.index_roots[slot]
            rs.update("crosslinks", [ci], ST.pack_crosslinks(st.crosslink_epochs[ci:ci + 1],
                                                            st.crosslink_roots[ci:ci + 1]))
            st.scalars["Slot"] += 1
            rs.set_scalar("Slot", st.scalars["Slot"])
            out["steps"].append(root() + (st.tree_hash_ssz(),))
        out["after slots"] = _oracle(st)
        # one epoch step
        empty = _state(0, 0, 0, 0, 1).attestations
        st.attestations = empty
        rs.replace("attestations", empty)
        st.balances[:] = rng.integers(0, 1 << 40, 1000).astype(np.uint64)
        rs.update("balances", np.arange(1000), st.balances)
        st.eth1_votes = np.concatenate([st.eth1_votes, donor.eth1_votes[:1]])
        st.eth1_vote_counts = np.concatenate([st.eth1_vote_counts, donor.eth1_vote_counts[:1]])
        rs.append("eth1_votes", ST.pack_eth1_votes(donor.eth1_votes[:1], donor.eth1_vote_counts[:1]))
        st.seeds = donor.seeds.copy()
        rs.set_seeds(bytes(st.seeds[0]), bytes(st.seeds[1]))
        out["epoch"] = root() + (st.tree_hash_ssz(), _oracle(st))
        # an index beyond the list raises and changes nothing
        with pytest.raises(IndexError):
            rs.update("balances", [3, 1000], np.array([1, 2], dtype=np.uint64))
        with pytest.raises(IndexError):
            rs.update("registry", [rs.count("registry")], R.synthetic_registry(1, 1).records)
        out["after bad update"] = root()
    finally:
        D.trees_update = real
    return out


def test_eight_slots(slots):
    got, ncalls, mirror = slots["assign"]
    assert got == mirror and ncalls == 1
    for s, (got, ncalls, mirror) in enumerate(slots["steps"]):
        assert got == mirror, f"slot {s}"
    assert slots["steps"][-1][0] == slots["after slots"], "the oracle after the last slot"


def test_epoch_step(slots):
    got, ncalls, mirror, oracle = slots["epoch"]
    assert got == mirror
    assert got == oracle


def test_bad_index_changes_nothing(slots):
    assert slots["after bad update"][0] == slots["epoch"][0]


def test_one_trees_update_per_root(slots):
    counts = [slots["assign"][1]] + [x[1] for x in slots["steps"]] + [slots["epoch"][1], slots["after bad update"][1]]
    assert counts == [1] * len(counts)


def test_attestation_outgrows_its_slot(gpu):
    """A bitfield longer than the slot capacity repacks the resident records and rebuilds the tree."""
    from prysm_amd import state as ST

    st = _state(37, 3, 1, 1, 5)
    rs = ST.ResidentBeaconState(gpu)
    rs.assign(st)
    one = _one_attestation(_state(8, 2, 0, 0, 5, salt=9), 0)
    one.aggregation_bitfield = [bytes(range(70))]
    _append_attestation(st, one)
    rs.append("attestations", one)
    assert rs.root() == _oracle(st)
