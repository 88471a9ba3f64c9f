"""Stateful fuzz of the resident deposit trie's handle: about 60 random steps
of append / truncate / clone / copy_from / fork_point / audit / branches on two
handles, against oracle.DictTrie models (the literal restatement of
deposit_trie.go) rebuilt from the deposit sequences the steps leave behind
(DESIGN.md §5p).  Counts stay at or below 3000."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CLEAN = (0, 0xFFFFFFFF, 2**64 - 1)
LIMIT = 3000


@pytest.fixture(autouse=True)
def _collect_handles():
    """A trie handle caught in a reference cycle (a frame kept by pytest.raises) is freed here, not by a
    collection in the middle of some later test's graph capture, where freeing device memory is an error."""
    yield
    import gc

    gc.collect()


@pytest.fixture(scope="module")
def gpu():
    import torch

    from prysm_amd import _lib

    assert torch.cuda.is_available()
    _lib.init(0)
    return torch.device("cuda:0")


class Model:
    """A deposit sequence and the DictTrie over it, rebuilt only after the sequence shrank or was replaced."""

    def __init__(self, depth):
        from oracle import oracle as O

        self.O, self.depth, self.seq = O, depth, []
        self.trie = O.DictTrie(depth)

    def append(self, ds):
        for d in ds:
            self.trie.update(d)
        self.seq += ds

    def reset(self, seq):
        self.seq = list(seq)
        self.trie = self.O.DictTrie(self.depth)
        for d in self.seq:
            self.trie.update(d)


@pytest.mark.parametrize("seed,depth", [(1, 10), (2, 32)])
def test_handle_fuzz(gpu, seed, depth):
    from oracle import oracle as O
    from prysm_amd import trieutil as T

    rng = np.random.default_rng(seed)
    full = min(1 << depth, LIMIT)
    fresh = iter(range(1 << 30))

    def new_deposits(k):
        return [bytes(O.splitmix_bytes(200 + 8 * (i % 11), 0x5EED0000 + seed, 64 * i)) for i in (next(fresh) for _ in range(k))]

    tries = [T.DepositTrie(depth), T.DepositTrie(depth, capacity=40)]
    models = [Model(depth), Model(depth)]
    audits = 0
    for step in range(60):
        w = int(rng.integers(2))
        t, m = tries[w], models[w]
        op = int(rng.integers(8)) if step > 3 else 0
        if op <= 1:  # append: one, a few, or many (the wide forms)
            k = int(rng.choice([1, 3, 17, 300, 1100]))
            k = min(k, full - len(m.seq))
            ds = new_deposits(k)
            for d in ds:
                t.update_deposit_trie(d)
            m.append(ds)
        elif op == 2:  # roll back
            n = len(m.seq)
            c = int(rng.choice([0, n, max(n - 1, 0), n // 2, int(rng.integers(n + 1)), 1 << max(n.bit_length() - 2, 0)]))
            c = min(c, n)
            t.truncate(c)
            m.reset(m.seq[:c])
        elif op == 3:  # clone replaces the other handle
            tries[1 - w] = t.clone()
            models[1 - w].reset(m.seq)
        elif op == 4:  # copy_from
            tries[1 - w].copy_from(t)
            models[1 - w].reset(m.seq)
        elif op == 5:  # fork point
            a, b = models[0].seq, models[1].seq
            mm = min(len(a), len(b))
            want = next((i for i in range(mm) if a[i] != b[i]), mm)
            assert tries[0].fork_point(tries[1]) == want == tries[1].fork_point(tries[0]), step
        elif op == 6:  # branches now and as of an older count
            n = len(m.seq)
            if n:
                idx = [int(i) for i in rng.integers(0, n, size=4)] + [n - 1]
                got = t.generate_merkle_branches(idx).tobytes()
                assert got == b"".join(b"".join(m.trie.branch(i)) for i in idx), step
                old = int(rng.integers(1, n + 1))
                past = O.DictTrie(depth)
                for d in m.seq[:old]:
                    past.update(d)
                assert t.root_at(old) == past.root(), (step, old)
                assert t.generate_merkle_branches(idx, old).tobytes() == \
                    b"".join(b"".join(past.branch(i)) for i in idx), (step, old)
        if op == 7 or step % 5 == 4:
            for x in tries:
                assert x.audit() == CLEAN, step
            audits += 1
        assert t.root() == m.trie.root() and t.deposit_count == len(m.seq), (step, op)
    for x, mm in zip(tries, models):
        assert x.root() == mm.trie.root() and x.audit() == CLEAN
    assert audits >= 10
