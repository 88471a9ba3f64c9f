"""The expected values of the RepeatHash tests (tests/repeat_hash_ref.py)
pinned on the CPU: the helper is hashutil.RepeatHash (hash.go:29-34) by the
oracle's Keccak-256, nothing else."""
import numpy as np

from oracle import oracle as O
from tests import repeat_hash_ref as RH

ZERO32 = bytes(32)


def _x(seed: int) -> bytes:
    return O.splitmix_bytes(32, 0x5EED000000000000 + seed).tobytes()


def test_zero_times_is_the_value():
    for x in (ZERO32, b"\xff" * 32, _x(1)):
        assert RH.repeat(x, 0) == x


def test_one_time_is_hash():
    # the commitment the reference's own tests use (block_operations_test.go:51)
    assert RH.repeat(ZERO32, 1) == O.keccak256(ZERO32)
    x = _x(2)
    assert RH.repeat(x, 1) == O.keccak256(x)
    assert RH.repeat(x, 3) == O.keccak256(O.keccak256(O.keccak256(x)))


def test_counts_add():
    x = _x(3)
    for a, b in ((0, 5), (1, 1), (3, 4), (7, 0), (9, 16)):
        assert RH.repeat(x, a + b) == RH.repeat(RH.repeat(x, a), b)


def test_onion_and_chains_are_the_loop():
    seeds = O.splitmix_bytes(5 * 32, 0x5EED000000000000 + 4).reshape(5, 32)
    on = RH.onion(seeds, 6)
    assert on.shape == (5, 7, 32)
    for i in range(5):
        for t in range(7):
            assert on[i, t].tobytes() == RH.repeat(seeds[i].tobytes(), t)
    lay = [0, 6, 2, 1, 5]
    ch = RH.chains(seeds, lay)
    for i in range(5):
        assert ch[i].tobytes() == on[i, lay[i]].tobytes()
    assert np.array_equal(RH.chains(seeds, 3), on[:, 3])


def test_verify_codes():
    # two 48-byte records: commitment at 4, le64 layers at 40
    rec = np.zeros((2, 48), dtype=np.uint8)
    rev = np.stack([np.frombuffer(_x(5), np.uint8), np.frombuffer(_x(6), np.uint8)])
    rec[0, 4:36] = np.frombuffer(RH.repeat(rev[0].tobytes(), 3), np.uint8)
    rec[0, 40:48] = np.frombuffer((3).to_bytes(8, "little"), np.uint8)
    rec[1, 4:36] = rev[1]
    rec[1, 40:48] = np.frombuffer(((1 << 32) + 0).to_bytes(8, "little"), np.uint8)  # truncated: 0 layers
    got = RH.verify(rec, 48, 4, 40, [0, 1, 2, 0], np.stack([rev[0], rev[1], rev[0], rev[1]]), 8)
    assert got.tolist() == [1, 2, 3, 0]
    assert RH.verify(rec, 48, 4, 40, [0], rev[:1], 2).tolist() == [2]
