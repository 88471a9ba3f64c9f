"""hashutil.RepeatHash on the device: batched chains, hash
onions and the RANDAO check, in both kernel forms (one chain per GPU lane, one
chain per wave) and as MK_REPEAT_AUTO picks, bit for bit against the oracle's
loop (tests/repeat_hash_ref.py).  <= 64 layers everywhere."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from prysm_amd import _lib
from tests import repeat_hash_ref as RH

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000000 + 7100
FORMS = [_lib.MK_REPEAT_LANE, _lib.MK_REPEAT_WAVE, _lib.MK_REPEAT_AUTO]
FORM_IDS = ["lane", "wave", "auto"]
NS = [1, 3, 4, 5, 63, 64, 65, 257]
NMAX, LMAX = 257, 33


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def onions():
    """Every expected chain value of this file, computed once: seed kind ->
    (NMAX, LMAX + 1, 32), row t of chain i = RepeatHash(seed i, t)."""
    seeds = {
        "zero": np.zeros((NMAX, 32), dtype=np.uint8),
        "ff": np.full((NMAX, 32), 0xFF, dtype=np.uint8),
        "random": O.splitmix_bytes(NMAX * 32, SEED).reshape(NMAX, 32).copy(),
    }
    out = {k: RH.onion(v, LMAX) for k, v in seeds.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def _patterns(n: int):
    i = np.arange(n)
    one33 = np.zeros(n, dtype=np.int64)
    one33[n // 2] = 33
    return {"zeros": np.zeros(n, np.int64), "ones": np.ones(n, np.int64), "twos": np.full(n, 2), "threes": np.full(n, 3),
            "mod8": i % 8, "one33": one33, "uniform25": np.full(n, 25)}


def _dev_chain(gpu, seeds, layers, max_layers, form):
    import torch

    from prysm_amd import device as D

    n = len(layers)
    d_seeds = torch.from_numpy(np.array(seeds, dtype=np.uint8).reshape(-1)).to(gpu)
    d_lay = torch.from_numpy(np.asarray(layers, dtype=np.int64).astype(np.int32)).to(gpu)
    out, status = D.repeat_hash(d_seeds, d_lay, n, max_layers, form)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n, 32), int(status.cpu().numpy()[0])


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("n", NS)
def test_chains(gpu, onions, form, n):
    for kind, on in onions.items():
        for name, lay in _patterns(n).items():
            got, status = _dev_chain(gpu, on[:n, 0], lay, 64, form)
            want = on[np.arange(n), lay]
            assert status == 0, (kind, name)
            assert np.array_equal(got, want), (kind, name, np.nonzero((got != want).any(axis=1))[0][:8])


def test_auto_above_the_wave_form(gpu):
    """More chains than MK_REPEAT_AUTO gives to the one-chain-per-wave form: the
    choice changes nothing."""
    n = (1 << 14) + 3
    seeds = O.splitmix_bytes(n * 32, SEED + 1).reshape(n, 32)
    lay = np.arange(n) % 3
    want = RH.chains(seeds, lay)
    got, status = _dev_chain(gpu, seeds, lay, 2, _lib.MK_REPEAT_AUTO)
    assert status == 0 and np.array_equal(got, want)
    got, status = _dev_chain(gpu, seeds, lay, 2, _lib.MK_REPEAT_LANE)
    assert status == 0 and np.array_equal(got, want)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("n", [1, 5, 65])
@pytest.mark.parametrize("layers", [0, 1, 5])
def test_onions(gpu, onions, form, n, layers):
    import torch

    from prysm_amd import device as D

    on = onions["random"]
    d_seeds = torch.from_numpy(on[:n, 0].copy().reshape(-1)).to(gpu)
    out = D.hash_onion(d_seeds, n, layers, form)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(n, layers + 1, 32)
    assert np.array_equal(got[:, 0], on[:n, 0])  # row 0 is the seed
    assert np.array_equal(got, on[:n, :layers + 1])
    chain, _ = _dev_chain(gpu, on[:n, 0], np.full(n, layers), 64, form)
    assert np.array_equal(got[:, layers], chain)  # the last row is the chain's result


def test_host_entries(gpu, onions):
    from prysm_amd import hashutil as H

    on = onions["random"]
    x = on[0, 0].tobytes()
    for k in (0, 1, 7):
        assert H.RepeatHash(x, k) == RH.repeat(x, k) == on[0, k].tobytes()
    lay = np.arange(65) % 8
    assert np.array_equal(H.repeat_hash_batch(on[:65, 0], lay, max_layers=7), on[np.arange(65), lay])
    assert np.array_equal(H.repeat_hash_batch(on[:5, 0], 4), on[:5, 4])
    assert np.array_equal(H.hash_onion(on[:65, 0], 5), on[:65, :6])
    assert H.repeat_hash_batch(np.zeros((0, 32), np.uint8), []).shape == (0, 32)
    with pytest.raises(_lib.MerkleError) as e:
        H.RepeatHash(x, _lib.MK_REPEAT_MAX_LAYERS + 1)
    assert e.value.code == _lib.MK_EINVAL
    with pytest.raises(_lib.MerkleError) as e:
        H.hash_onion(on[:2, 0], _lib.MK_REPEAT_MAX_LAYERS + 1)
    assert e.value.code == _lib.MK_EINVAL


# ---- the cap ----------------------------------------------------------------------------------------
def test_cap_host_entry_refuses_and_touches_nothing(gpu, onions):
    seeds = np.ascontiguousarray(onions["random"][:5, 0])
    lay = np.array([1, 2, 9, 3, 10], dtype=np.uint32)
    out = np.full((5, 32), 0xAA, dtype=np.uint8)
    call = _lib.Call(-1, 0, b"")
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = _lib.load().mk_repeat_hash_batch(ctypes.byref(call), vp(seeds), vp(lay), 5, 8, vp(out))
    assert rc == _lib.MK_EINVAL and call.code == _lib.MK_EINVAL
    assert b"layers[2]" in call.err  # the first offender
    assert (out == 0xAA).all()
    rc = _lib.load().mk_repeat_hash_batch(ctypes.byref(call), vp(seeds), vp(lay), 5, 10, vp(out))
    assert rc == _lib.MK_OK
    assert np.array_equal(out, onions["random"][np.arange(5), lay])
    # null pointers
    rc = _lib.load().mk_repeat_hash_batch(ctypes.byref(call), None, vp(lay), 5, 10, vp(out))
    assert rc == _lib.MK_EINVAL
    rc = _lib.load().mk_repeat_hash_batch(ctypes.byref(call), None, None, 0, 10, None)
    assert rc == _lib.MK_OK


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_cap_device_entry_zeroes_the_chain_and_flags(gpu, onions, form):
    on = onions["random"]
    n = 65
    lay = np.arange(n) % 8
    lay[3] = 9          # above max_layers 8
    lay[64] = 1 << 30   # far above: must not run
    got, status = _dev_chain(gpu, on[:n, 0], lay, 8, form)
    assert status == 1
    good = np.ones(n, dtype=bool)
    good[[3, 64]] = False
    assert not got[~good].any()
    assert np.array_equal(got[good], on[np.arange(n)[good], lay[good]])
    # the word is the caller's: a call sets it and never clears it
    import torch

    from prysm_amd import device as D

    d_seeds = torch.from_numpy(on[:n, 0].copy().reshape(-1)).to(gpu)
    status = torch.zeros(1, dtype=torch.int32, device=gpu)
    for layers, want in ((np.arange(n) % 8, 0), (lay, 1), (np.arange(n) % 8, 1)):
        D.repeat_hash(d_seeds, torch.from_numpy(layers.astype(np.int32)).to(gpu), n, 8, form, status=status)
        torch.cuda.synchronize()
        assert int(status.item()) == want


def test_cap_above_the_library_constant_is_refused(gpu, onions):
    import torch

    from prysm_amd import device as D

    big = _lib.MK_REPEAT_MAX_LAYERS + 1
    d_seeds = torch.from_numpy(onions["random"][:4, 0].copy().reshape(-1)).to(gpu)
    d_lay = torch.zeros(4, dtype=torch.int32, device=gpu)
    d_idx = torch.zeros(4, dtype=torch.int64, device=gpu)
    rec = torch.zeros(4 * 160, dtype=torch.uint8, device=gpu)
    p_seeds = ctypes.c_void_p(d_seeds.data_ptr())
    for f in (lambda: D.repeat_hash(d_seeds, d_lay, 4, big),
              # the entry point itself: the wrapper would size an output for 2^20 + 2 rows first
              lambda: _lib.invoke("mk_dev_hash_onion", p_seeds, 4, big, _lib.MK_REPEAT_AUTO, p_seeds, None),
              lambda: D.verify_repeat_hash(rec, 4, 160, 80, 112, d_idx, d_seeds, 4, big)):
        with pytest.raises(_lib.MerkleError) as e:
            f()
        assert e.value.code == _lib.MK_EINVAL
    # an unknown form, too
    with pytest.raises(_lib.MerkleError) as e:
        D.repeat_hash(d_seeds, d_lay, 4, 8, form=7)
    assert e.value.code == _lib.MK_EINVAL
    # the cap itself is accepted
    out, status = D.repeat_hash(d_seeds, d_lay, 4, _lib.MK_REPEAT_MAX_LAYERS)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(4, 32), onions["random"][:4, 0])


# ---- verify against flat records -----------------------------------------------------------------------
N_REC, M, MAXL = 300, 70, 9


def _flat_case(stride: int, commit_off: int, layers_off: int, seed: int):
    """300 records, 70 proposals and what each must answer."""
    rec = O.splitmix_bytes(N_REC * stride, seed).reshape(N_REC, stride).copy()
    reveals_of = O.splitmix_bytes(N_REC * 32, seed + 1).reshape(N_REC, 32).copy()
    layers = np.arange(N_REC) % 10  # 0 .. 9; 0: the reveal is the commitment
    commit = RH.chains(reveals_of, layers)
    rec[:, commit_off:commit_off + 32] = commit
    rec[:, layers_off:layers_off + 8] = layers.astype("<u8").view(np.uint8).reshape(N_REC, 8)
    # record 101: one changed commitment byte; 102: layers max + 1; 103: 2^32 + 1 layers whose low word would verify
    rec[101, commit_off + 31] ^= 0x01
    rec[102, layers_off:layers_off + 8] = np.frombuffer((MAXL + 1).to_bytes(8, "little"), np.uint8)
    rec[103, layers_off:layers_off + 8] = np.frombuffer(((1 << 32) + 1).to_bytes(8, "little"), np.uint8)
    rec[103, commit_off:commit_off + 32] = np.frombuffer(RH.repeat(reveals_of[103].tobytes(), 1), np.uint8)
    idx = [int(v) for v in (np.arange(M) * 37) % 100]            # 0 .. 99, layers 0 .. 9
    idx[10:14] = [20, 20, 30, 30]                                # repeats (layers 0)
    idx[20], idx[21], idx[22], idx[23] = 101, 102, 103, 299
    reveals = reveals_of[idx].copy()
    reveals[5, 17] ^= 0x10                                       # one bit of one reveal
    want = np.ones(M, dtype=np.uint8)
    want[5] = 0
    want[20] = 0
    want[21] = 2
    want[22] = 2
    assert np.array_equal(RH.verify(rec, stride, commit_off, layers_off, idx, reveals, MAXL), want)
    return rec, np.array(idx, dtype=np.uint64), reveals, want


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("layout", [(160, 80, 112), (77, 3, 37)], ids=["validator", "unaligned"])
def test_verify_flat(gpu, form, layout):
    import torch

    from prysm_amd import device as D

    stride, coff, loff = layout
    rec, idx, reveals, want = _flat_case(stride, coff, loff, SEED + 10 + stride)
    # through the device entry two more proposals: indices past the records
    idx_d = np.concatenate([idx, np.array([N_REC, 1 << 40], dtype=np.uint64)])
    rev_d = np.concatenate([reveals, reveals[:2]])
    want_d = np.concatenate([want, np.array([3, 3], dtype=np.uint8)])
    d_rec = torch.from_numpy(rec.reshape(-1)).to(gpu)
    d_idx = torch.from_numpy(idx_d.view(np.int64)).to(gpu)
    d_rev = torch.from_numpy(rev_d.reshape(-1)).to(gpu)
    ok = D.verify_repeat_hash(d_rec, N_REC, stride, coff, loff, d_idx, d_rev, M + 2, MAXL, form)
    torch.cuda.synchronize()
    assert ok.cpu().numpy().tolist() == want_d.tolist()
    if form != _lib.MK_REPEAT_AUTO:
        return
    # the host entry: the same verdicts; an index past the records and an offset past the stride are refused
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    got = np.full(M, 0xAA, dtype=np.uint8)
    args = (vp(rec), N_REC, stride, coff, loff, vp(idx), vp(reveals), M, MAXL, vp(got))
    _lib.invoke("mk_verify_repeat_hash", *args)
    assert got.tolist() == want.tolist()
    got[:] = 0xAA
    with pytest.raises(_lib.MerkleError) as e:
        _lib.invoke("mk_verify_repeat_hash", vp(rec), N_REC, stride, coff, loff, vp(idx_d), vp(rev_d), M + 2, MAXL,
                    vp(got))
    assert e.value.code == _lib.MK_EINVAL and (got == 0xAA).all()
    for bad in ((stride - 31, loff), (coff, stride - 7)):
        with pytest.raises(_lib.MerkleError) as e:
            _lib.invoke("mk_verify_repeat_hash", vp(rec), N_REC, stride, bad[0], bad[1], vp(idx), vp(reveals), M, MAXL,
                        vp(got))
        assert e.value.code == _lib.MK_EINVAL
    _lib.invoke("mk_verify_repeat_hash", None, 0, stride, coff, loff, None, None, 0, MAXL, None)  # m == 0


# ---- verify against the records a resident tree owns --------------------------------------------------------
def _commit(records, reveals_of, layers):
    """records (VALIDATOR_DTYPE) with layers[i] and RepeatHash(reveals_of[i], layers[i]) as their RANDAO fields."""
    records["randao_layers"] = layers
    records["randao_commitment_hash32"] = RH.chains(reveals_of, layers)


def test_verify_struct_list_tree(gpu):
    from prysm_amd import registry as RG
    from prysm_amd.listtree import StructListTree

    n = 300
    records = RG.synthetic_registry(n, SEED + 20).records.copy()
    reveals_of = O.splitmix_bytes(n * 32, SEED + 21).reshape(n, 32).copy()
    layers = np.arange(n) % 7
    _commit(records, reveals_of, layers)
    records["randao_layers"][200] = MAXL + 1
    tree = StructListTree(160, RG.VALIDATOR_FIELDS, capacity=n)
    tree.assign(records)
    root, audit = tree.root(), tree.audit()
    idx = [(11 * j) % 199 for j in range(40)] + [200, 7, 7]
    rev = reveals_of[idx].copy()
    rev[3, 0] ^= 0x80
    want = np.ones(len(idx), dtype=np.uint8)
    want[3], want[40] = 0, 2
    coff, loff = RG.RANDAO_COMMITMENT_OFF, RG.RANDAO_LAYERS_OFF
    assert (coff, loff) == (80, 112)
    assert tree.verify_repeat_hash(idx, rev, coff, loff, MAXL).tolist() == want.tolist()
    # proposer 7 reveals a layer (the state transition stores the reveal as the new commitment, one layer less)
    new = records[7:8].copy()
    new["randao_layers"] = 4
    new_reveal = O.splitmix_bytes(32, SEED + 22)
    new["randao_commitment_hash32"] = np.frombuffer(RH.repeat(new_reveal.tobytes(), 4), np.uint8)
    tree.update([7], new)
    got = tree.verify_repeat_hash([7, 7, 8], np.stack([reveals_of[7], new_reveal, reveals_of[8]]), coff, loff, MAXL)
    assert got.tolist() == [0, 1, 1]
    # read-only
    records[7] = new[0]
    assert tree.root() == RG.struct_list_root(records) != root
    assert tree.audit() == audit
    r2 = tree.root()
    tree.verify_repeat_hash(idx, rev, coff, loff, MAXL)
    assert tree.root() == r2 and tree.audit() == audit
    assert np.array_equal(tree.records(), records.view(np.uint8).reshape(n, 160))
    # refused with nothing done: an index past the list, offsets past the record, a cap above the constant
    for args in (([n], reveals_of[:1], coff, loff, MAXL), ([0], reveals_of[:1], 129, loff, MAXL),
                 ([0], reveals_of[:1], coff, 153, MAXL), ([0], reveals_of[:1], coff, loff, _lib.MK_REPEAT_MAX_LAYERS + 1)):
        with pytest.raises(_lib.MerkleError) as e:
            tree.verify_repeat_hash(*args)
        assert e.value.code == _lib.MK_EINVAL
    assert tree.verify_repeat_hash([], np.zeros((0, 32), np.uint8), coff, loff, MAXL).size == 0


def test_lone_handle_of_another_kind_is_refused(gpu):
    """The handles of the three kinds share one core (csrc/tree_handle.cpp), and the verify asks it for the
    kind: a list tree's handle behind the struct tree's entry point is refused, not read as records."""
    from prysm_amd.listtree import ListTree

    lt = ListTree(32, capacity=4)
    lt.assign(np.zeros((4, 32), np.uint8))
    root = lt.root()
    idx, rev, ok = np.zeros(1, np.uint64), np.zeros(32, np.uint8), np.full(1, 0xAA, np.uint8)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    with pytest.raises(_lib.MerkleError) as e:
        _lib.invoke("mk_struct_list_tree_verify_repeat_hash", lt._handle, 0, 8, vp(idx), vp(rev), 1, MAXL, vp(ok))
    assert e.value.code == _lib.MK_EINVAL and "struct list tree" in str(e.value)
    assert ok[0] == 0xAA and lt.root() == root


def test_verify_randao_on_a_beacon_tree_set(gpu):
    from prysm_amd import state as ST

    n = 300
    st = ST.synthetic_state(n, SEED + 30, n_attestations=5, n_batched=3, n_votes=2, lists_len=64, shards=64)
    reveals_of = O.splitmix_bytes(n * 32, SEED + 31).reshape(n, 32).copy()
    layers = np.arange(n) % 6
    _commit(st.registry.records, reveals_of, layers)
    ts = ST.beacon_tree_set(st)
    assert ts.root() == st.tree_hash_ssz()
    audit = ts.audit()
    idx = [(13 * j) % n for j in range(33)]
    rev = reveals_of[idx].copy()
    rev[9, 31] ^= 0x01
    want = np.ones(33, dtype=np.uint8)
    want[9] = 0
    assert ts.verify_randao(idx, rev, max_layers=MAXL).tolist() == want.tolist()
    assert ts.verify_randao(idx, rev, max_layers=4).tolist() == \
        [2 if layers[i] > 4 else int(w) for i, w in zip(idx, want)]
    # a pending update is seen: nothing asks for the root between the update and the check
    new = st.registry.records[13:14].copy()
    new_reveal = O.splitmix_bytes(32, SEED + 32)
    new["randao_layers"] = 9
    new["randao_commitment_hash32"] = np.frombuffer(RH.repeat(new_reveal.tobytes(), 9), np.uint8)
    st.registry.records[13] = new[0]
    ts.update("registry", [13], new)
    got = ts.verify_randao([13, 13, 26], np.stack([reveals_of[13], new_reveal, reveals_of[26]]), max_layers=MAXL)
    assert got.tolist() == [0, 1, 1]
    root = ts.root()
    assert root == st.tree_hash_ssz()
    ts.verify_randao(idx, rev, max_layers=MAXL)
    assert ts.root() == root and ts.audit() == audit
    # refused: an index past the registry, an offset past the record, a tree that holds no records
    with pytest.raises(_lib.MerkleError) as e:
        ts.verify_randao([n], reveals_of[:1], max_layers=MAXL)
    assert e.value.code == _lib.MK_EINVAL
    with pytest.raises(_lib.MerkleError) as e:
        ts.verify_repeat_hash("registry", [0], reveals_of[:1], 130, 112, MAXL)
    assert e.value.code == _lib.MK_EINVAL
    for other in ("balances", "randao_mixes"):
        with pytest.raises(_lib.MerkleError) as e:
            ts.verify_repeat_hash(other, [0], reveals_of[:1], 0, 0, MAXL)
        assert e.value.code == _lib.MK_EINVAL
    assert ts.root() == root
