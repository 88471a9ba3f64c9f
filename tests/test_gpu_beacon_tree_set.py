"""prysm_amd.state.beacon_tree_set(): a whole BeaconState behind one
mk_tree_set handle -- the ten trees of RESIDENT_TREES at CONTAINER_OFF in the
536-B state message.  Every root is held against the oracle's reflective
TreeHash of the same state (oracle/ssz_ref.py); the states and the slot change
set are test_gpu_resident_state.py's."""
import numpy as np
import pytest

from prysm_amd import _lib
from tests.test_gpu_resident_state import _append_attestation, _one_attestation, _oracle, _state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


@pytest.mark.parametrize("shape", [(37, 3, 1, 1, 5), (1000, 128, 16, 4, 8192)])
def test_assign_then_three_slots(gpu, shape):
    from prysm_amd import listtree as LT
    from prysm_amd import state as ST

    st = _state(*shape)
    nv, _, _, _, lists = shape
    donor = _state(64, 16, 0, 4, 64, salt=77)
    ts = ST.beacon_tree_set(st)
    assert isinstance(ts, LT.TreeSet) and len(ts) == len(ST.RESIDENT_TREES) == 10
    assert ts.container_len == ST.CONTAINER_LEN
    want = _oracle(st)
    assert ts.root() == want
    assert ts.root() == want  # nothing dirty: the same root again
    rng = np.random.default_rng(5)
    for slot in range(3):
        at = (st.scalars["Slot"] + slot) % lists
        new32 = donor.randao_mixes[2 * slot:2 * slot + 2]
        st.latest_block_roots[at], st.randao_mixes[at] = new32[0], new32[1]
        ts.update("latest_block_roots", [at], new32[0:1])
        ts.update("randao_mixes", [at], new32[1:2])
        bi = rng.choice(nv, 3, replace=False)
        bv = rng.integers(0, 1 << 40, 3).astype(np.uint64)
        st.balances[bi] = bv
        ts.update("balances", bi, bv.astype("<u8"))
        vi = rng.choice(nv, 2, replace=False)
        vr = donor.registry.records[4 * slot:4 * slot + 2]
        st.registry.records[vi] = vr
        ts.update("registry", vi, vr)
        one = _one_attestation(donor, slot)
        _append_attestation(st, one)
        n_att = ts.count("attestations")
        ts.append("attestations", one)
        assert ts.count("attestations") == n_att + 1
        ci = int(rng.integers(0, min(1024, lists)))
        st.crosslink_epochs[ci] = 7000 + slot
        st.crosslink_roots[ci] = donor.index_roots[slot]
        ts.update("crosslinks", [ci], ST.pack_crosslinks(st.crosslink_epochs[ci:ci + 1],
                                                        st.crosslink_roots[ci:ci + 1]))
        st.scalars["Slot"] += 1
        ts.set_scalar("Slot", st.scalars["Slot"])
        assert ts.root() == _oracle(st), f"slot {slot}"
    assert ts.tree_root("balances") == ts.tree_root(ST.RESIDENT_TREES.index(
        next(t for t in ST.RESIDENT_TREES if t[0] == "balances")))
    assert np.array_equal(ts.items("balances").reshape(-1).view("<u8"), st.balances)
