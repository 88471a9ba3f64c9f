"""verifyDeposit for a batch (k_verify_deposits: mk_verify_deposits,
mk_dev_verify_deposits): the deposit data hashed, folded through
its branch and compared on the device.  Expected: oracle.verify_merkle_branch
over oracle.keccak256(data), for every item.  The data lengths sit on both
sides of the sponge's 136-byte rate and its multiples, and follow one another
unaligned in one buffer."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000000 + 0xDE9
LENS = (1, 16, 135, 136, 137, 271, 272, 273, 600)
DEPTH = 32


@pytest.fixture(scope="module")
def gpu():
    import torch

    from prysm_amd import _lib

    assert torch.cuda.is_available()
    _lib.init(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def world(gpu):
    """300 deposits of the mixed lengths in a resident trie, and per n in
    {1, 16, 300}: the branches of all n as of n deposits and that root."""
    from oracle import oracle as O
    from prysm_amd import trieutil as T

    raw = O.splitmix_bytes(300 * 600, SEED)
    deps = [bytes(raw[600 * i:600 * i + LENS[(i * 5 + i // 9) % len(LENS)]]) for i in range(300)]
    assert {len(d) for d in deps[:16]} == set(LENS)
    t = T.DepositTrie.build(deps)
    at = {n: (t.generate_merkle_branches(list(range(n)), n), t.root_at(n)) for n in (1, 16, 300)}
    return deps, t, at


def _flip(b: bytes, bit: int) -> bytes:
    a = bytearray(b)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


def _oracle(datas, branches, indices, roots, depth=DEPTH, tree_depth=32):
    from oracle import oracle as O

    return [O.verify_merkle_branch(O.keccak256(d), [bytes(b[k]) for k in range(depth)], depth, i, r, tree_depth)
            for d, b, i, r in zip(datas, branches, indices, roots)]


@pytest.mark.parametrize("n", [1, 16, 300])
def test_positive_shared_and_per_item_roots(world, n):
    from prysm_amd import trieutil as T

    deps, t, at = world
    br, root = at[n]
    idx = list(range(n))
    want = _oracle(deps[:n], br, idx, [root] * n)
    assert all(want)
    assert T.verify_deposits(deps[:n], br, idx, root, DEPTH) == want  # root_stride 0, the (k, depth, 32) array
    lists = [[bytes(br[j, d]) for d in range(DEPTH)] for j in range(n)]
    assert T.verify_deposits(deps[:n], lists, idx, [root] * n, DEPTH) == want  # root_stride 32, lists of lists
    if n < 300:  # an older root than the trie's own: the case verifyDeposit meets
        assert root != t.root()
        assert not any(T.verify_deposits(deps[:n], br, idx, t.root(), DEPTH))


@pytest.mark.parametrize("n", [1, 16, 300])
def test_negatives_per_item(world, n):
    """Per item, next to the intact one: one flipped bit in the data, in the
    level-0 sibling, in the level-31 sibling, the index off by one, a wrong root."""
    from prysm_amd import trieutil as T

    deps, _, at = world
    br, root = at[n]
    rng = np.random.default_rng(n)
    datas, branches, indices, roots, kind = [], [], [], [], []
    for i in range(n):
        b = br[i]
        for v in range(6):
            d, bb, ix, r = deps[i], b, i, root
            if v == 1:
                d = _flip(d, int(rng.integers(0, 8 * len(d))))
            elif v in (2, 3):
                bb = b.copy()
                bb[0 if v == 2 else 31, int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
            elif v == 4:
                ix = i + 1
            elif v == 5:
                r = _flip(root, int(rng.integers(0, 256)))
            datas.append(d)
            branches.append(bb)
            indices.append(ix)
            roots.append(r)
            kind.append(v)
    want = _oracle(datas, branches, indices, roots)
    assert want == [v == 0 for v in kind]
    got = T.verify_deposits(datas, np.stack(branches), indices, roots, DEPTH)
    assert got == want
    # root_stride 0 over the same items (every root but the wrong-root variant's is the shared one)
    keep = [j for j, v in enumerate(kind) if v != 5]
    got0 = T.verify_deposits([datas[j] for j in keep], np.stack([branches[j] for j in keep]),
                             [indices[j] for j in keep], root, DEPTH)
    assert got0 == [want[j] for j in keep]


def test_depth_below_tree_depth(world):
    """depth < tree_depth folds only the first `depth` siblings of index +
    2^tree_depth: the same rule as the existing verifier and the oracle."""
    from oracle import oracle as O
    from prysm_amd import trieutil as T

    deps, t, at = world
    n, depth = 16, 5
    br = at[16][0][:, :depth, :].copy()
    idx = list(range(n))
    roots = []
    for i in range(n):  # the level-5 ancestor of leaf i, folded on the host
        v, ix = O.keccak256(deps[i]), i
        for d in range(depth):
            s = bytes(br[i, d])
            v = O.keccak256(s + v) if ix & 1 else O.keccak256(v + s)
            ix >>= 1
        roots.append(v)
    for tree_depth in (32, 5, 2):
        want = _oracle(deps[:n], br, idx, roots, depth, tree_depth)
        leaves = [O.keccak256(d) for d in deps[:n]]
        lists = [[bytes(br[j, d]) for d in range(depth)] for j in range(n)]
        assert T.verify_merkle_branches(leaves, lists, depth, idx, roots, tree_depth) == want
        assert T.verify_deposits(deps[:n], br, idx, roots, depth, tree_depth) == want
        if tree_depth >= depth:
            assert all(want)
    assert not all(_oracle(deps[:n], br, idx, roots, depth, 2))


def test_device_form(gpu, world):
    """mk_dev_verify_deposits over tensors, both root strides; a bad stride is refused."""
    import torch

    from prysm_amd import _lib
    from prysm_amd import device as D

    deps, _, at = world
    n = 300
    br, root = at[n]
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(d) for d in deps])
    data = torch.from_numpy(np.frombuffer(b"".join(deps), dtype=np.uint8).copy()).to(gpu)
    d_offs = torch.from_numpy(offs).to(gpu)
    d_br = torch.from_numpy(br.reshape(-1).copy()).to(gpu)
    pick = list(range(n))
    pick[7], pick[8] = 8, 7  # two wrong indices
    d_idx = torch.tensor(pick, dtype=torch.int64, device=gpu)
    d_root = torch.from_numpy(np.frombuffer(root, dtype=np.uint8).copy()).to(gpu)
    want = _oracle(deps, br, pick, [root] * n)
    assert want.count(False) == 2
    ok0 = D.verify_deposits(data, d_offs, d_br, d_idx, n, DEPTH, d_root, 0)
    ok32 = D.verify_deposits(data, d_offs, d_br, d_idx, n, DEPTH, d_root.repeat(n), 32)
    torch.cuda.synchronize()
    assert [bool(x) for x in ok0.cpu().numpy()] == want and [bool(x) for x in ok32.cpu().numpy()] == want
    with pytest.raises(_lib.MerkleError) as ei:
        D.verify_deposits(data, d_offs, d_br, d_idx, n, DEPTH, d_root.repeat(n), 16)
    assert ei.value.code == _lib.MK_EINVAL
