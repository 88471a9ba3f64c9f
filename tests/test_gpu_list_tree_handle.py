"""prysm_amd.listtree.ListTree (the mk_list_tree handle a cgo caller holds)
against the oracle's merkleHash, and the registry composed with it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000000 + 2200


@pytest.fixture(scope="module")
def gpu():
    import torch

    from prysm_amd import _lib

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def _rand(nbytes, salt):
    from oracle import oracle as O

    return O.splitmix_bytes((nbytes + 7) // 8 * 8, SEED + salt)[:nbytes].copy()


def _want(buf, n, L):
    from oracle import oracle as O

    return O.merkle_hash_flat(np.ascontiguousarray(buf).reshape(-1)[:n * L], n, L)


@pytest.mark.parametrize("L", [32, 8, 48])
def test_handle_against_oracle(gpu, L):
    from prysm_amd import _lib
    from prysm_amd.listtree import ListTree

    t = ListTree(L, capacity=30_000)
    assert len(t) == 0 and t.root() == _want(np.zeros(0, np.uint8), 0, L)  # merkleHash([])
    n = 25_001
    buf = _rand(80_000 * L, L).reshape(-1, L)
    t.assign(buf[:n])
    assert len(t) == n and t.root() == _want(buf, n, L)
    # unsorted indices with repeats: the last value of an index wins
    idx = np.array([700, 3, 25_000, 3, 1999, 700, 0, 3], dtype=np.uint64)
    vals = _rand(idx.size * L, 10 + L).reshape(-1, L)
    for i, v in zip(idx, vals):
        buf[int(i)] = v
    t.update(idx, vals)
    assert t.root() == _want(buf, n, L)
    assert np.array_equal(t.items(), buf[:n])
    assert np.array_equal(t.items(1998, 3), buf[1998:2001])
    # an index >= count is refused and changes nothing
    with pytest.raises(_lib.MerkleError) as e:
        t.update([1, n], _rand(2 * L, 11).reshape(2, L))
    assert e.value.code == _lib.MK_EINVAL
    assert t.root() == _want(buf, n, L) and np.array_equal(t.items(0, 2), buf[:2])
    # appends: a few (the climb), many (a rebuild pays), then past the capacity twice (grow + rebuild)
    for k in (7, 498, 5000, 40_000):
        t.append(buf[n:n + k])
        n += k
        assert len(t) == n and t.root() == _want(buf, n, L), k
    # an update large enough to rebuild instead of climbing
    idx = np.arange(0, n, 3, dtype=np.uint64)
    vals = _rand(idx.size * L, 12 + L).reshape(-1, L)
    buf[idx.astype(np.int64)] = vals
    t.update(idx, vals)
    assert t.root() == _want(buf, n, L)
    # and a small one after it climbs the rebuilt levels
    t.update([n - 1], buf[0:1])
    buf[n - 1] = buf[0]
    assert t.root() == _want(buf, n, L)
    assert np.array_equal(t.items(), buf[:n])


def test_registry_composition(gpu):
    """10 000 validators, 37 records change: their struct roots on the device
    (mk_dev_ssz_struct_roots) update a 32-B-item tree; the root equals the
    struct list's TreeHash of the changed registry."""
    import torch

    from oracle import oracle as O
    from prysm_amd import device as D
    from prysm_amd import registry as R
    from prysm_amd.listtree import ListTree

    n, k = 10_000, 37
    reg = R.synthetic_registry(n, SEED + 1)
    rec = reg.records.view(np.uint8).reshape(n, 160).copy()
    t = ListTree(32, capacity=n)
    t.assign(O.struct_roots(rec.reshape(-1), n, 160, R.VALIDATOR_FIELDS))
    assert t.root() == O.merkle_hash_flat(O.struct_roots(rec.reshape(-1), n, 160, R.VALIDATOR_FIELDS).reshape(-1), n, 32)
    idx = np.sort(np.random.default_rng(3).choice(n, k, replace=False))
    other = R.synthetic_registry(k, SEED + 2).records.view(np.uint8).reshape(k, 160)
    rec[idx] = other
    changed = torch.from_numpy(rec[idx].reshape(-1).copy()).to(gpu)
    roots = D.struct_roots(changed, k, 160, R.VALIDATOR_FIELDS)
    torch.cuda.synchronize()
    t.update(idx, roots.cpu().numpy()[:32 * k])
    want = O.merkle_hash_flat(O.struct_roots(rec.reshape(-1), n, 160, R.VALIDATOR_FIELDS).reshape(-1), n, 32)
    assert t.root() == want
